"""Build checks that need no GPU: both native extensions load (all symbols resolve) and expose
the kernels the framework calls."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = re.compile(r'^\s*(extern "C"\s+)?(int|void|long)\s+(fm_\w+)\(')


def _nm_fm(lib, which):
    out = subprocess.run(["nm", "-D", which, os.path.join(ROOT, "flexmi", lib)], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("fm_")}


def _declared_launchers():
    """fm_* functions declared with C linkage in csrc/kernels/*.h: `extern "C" T fm_x(...);` or a
    prototype inside an `extern "C" { ... }` block."""
    names = set()
    for path in glob.glob(os.path.join(ROOT, "csrc", "kernels", "*.h")):
        in_block = False
        for line in open(path):
            if line.startswith('extern "C" {'):
                in_block = True
            elif line.startswith("}"):
                in_block = False
            m = PROTO.match(line)
            if m and (m.group(1) or in_block):
                names.add(m.group(3))
    return names


def test_hip_extension_loads(native):
    import torch  # noqa: F401  (libtorch must be loaded first)
    import flexmi._C as C
    assert C.arch == "gfx950"
    for name in ("gemm", "embedding_fwd_multi", "embedding_bwd_multi", "dot_fwd", "dot_bwd", "sgd", "adam", "loss",
                 "im2col", "col2im", "transpose_batched", "pool_fwd", "pool_bwd", "bn_fwd", "bn_bwd", "skinny_fwd",
                 "skinny_bwd", "multi_copy", "softmax", "dropout", "permute", "init_fill",
                 "pool_last_form"):
        assert hasattr(C, name), name
    out = subprocess.run(["nm", "-D", "--undefined-only", C.__file__], capture_output=True, text=True).stdout
    assert "fm_" not in out, "unresolved kernel launcher symbols:\n" + out


def test_no_launcher_prototypes_outside_kernels(native):
    # callers include csrc/kernels/launchers.h; a hand-copied prototype is checked against nothing
    files = [p for p in glob.glob(os.path.join(ROOT, "csrc", "**", "*"), recursive=True)
             if os.path.isfile(p) and os.path.basename(os.path.dirname(p)) != "kernels"]
    files += glob.glob(os.path.join(ROOT, "tools", "*.hip"))
    assert any(p.endswith("hip_ops.cpp") for p in files) and any(p.endswith("native_hip.cc") for p in files)
    bad = [f"{os.path.relpath(p, ROOT)}:{i}: {line.strip()}" for p in files
           for i, line in enumerate(open(p, errors="replace"), 1) if PROTO.match(line)]
    assert not bad, "launcher prototypes outside csrc/kernels:\n" + "\n".join(bad)


def test_exported_launchers_are_the_declared_ones(native):
    exported, declared = _nm_fm("libflexmi_kernels.so", "--defined-only"), _declared_launchers()
    assert len(declared) > 80, "launcher declarations not found"
    assert exported == declared, (f"exported, not declared: {sorted(exported - declared)}; "
                                  f"declared, not exported: {sorted(declared - exported)}")


def test_native_c_library_resolves(native):
    missing = _nm_fm("libflexmi_native_c.so", "--undefined-only") - _nm_fm("libflexmi_kernels.so", "--defined-only")
    assert not missing, f"unresolved kernel launcher symbols: {sorted(missing)}"


def test_native_runtime_loads(native):
    import flexmi._native as N
    for name in ("load_strategy", "save_strategy", "encode_strategy", "decode_strategy", "Simulator"):
        assert hasattr(N, name), name
