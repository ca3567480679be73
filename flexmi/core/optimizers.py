"""SGD, Adam (``include/optimizer.h:26-74``, ``src/runtime/optimizer_kernel.cu``) and Adagrad.

Reference: one single-point Legion task per parameter gathers every gradient replica to one GPU,
sums them and applies the update (``optimizer_kernel.cu:44-110``).  flexmi: gradients are
reduced by RCCL all-reduce (bucketed, overlapped with backward), then ONE multi-tensor kernel
updates every parameter shard of the rank in a single pass over flat fp32 buffers and
refreshes the bf16 compute copies in the same pass (``csrc/kernels/optim.hip``).  On the device
each rule's arithmetic is written once (``csrc/kernels/update_rule.h``) and shared by the
optimizer launches and the dW GEMMs that fuse the SGD step; here each optimizer holds its rule
as ``update_torch`` and its launch as ``update_hip``, and the executor calls ``update``.
Update rules are bit-for-bit the reference's:

  SGD : g = ∇ + wd·W; V = μV + g; g = nesterov ? g + μV : V (only if μ>0); W -= lr·g
  Adam: β1ᵗ,β2ᵗ updated in ``next()``; α_t = α·sqrt(1-β2ᵗ)/(1-β1ᵗ);
        g = ∇ + wd·W; m = β1 m + (1-β1) g; v = β2 v + (1-β2) g²; W -= α_t·m/(sqrt(v)+ε)

Adagrad is a flexmi extension (the reference has none) with ``torch.optim.Adagrad``'s rule at
``lr_decay = 0``:

  Adagrad: g = ∇ + wd·W; H += g·g (H starts at ``initial_accumulator_value``); W -= lr·g/(sqrt(H)+ε)

Sparse embedding updates (no dense gradient buffer) need the update of an untouched row to be
the identity.  SGD without momentum / weight decay and Adagrad without weight decay qualify
(``sparse_capable``): under Adagrad a non-replicated table keeps an accumulator ``h`` of its own
shape and every step updates only the looked-up rows, duplicates summed BEFORE the gradient is
squared (``csrc/kernels/embedding.hip`` fm_sdp_coalesce + fm_emb_adagrad_apply) -- equal to dense
Adagrad.  Replicated tables under Adagrad take the dense path (``sparse_dp_capable`` is False:
applying the replicas' segments one by one is not Adagrad of the summed gradient).

Row-wise Adagrad (``RowwiseAdagradOptimizer``) is the form DLRM-class models are trained with:
dense parameters as under Adagrad, every embedding table sparsely with ONE accumulator per row
(``G[r,:]`` = the row's gradient of the step, duplicate lookups summed over the batch and the
replicas; ``D`` = the table's embedding dim):

  h[r] += (1/D)·Σ_c G[r,c]²  (h starts at ``initial_accumulator_value``); W[r,c] -= lr·G[r,c]/(sqrt(h[r])+ε)

``h`` is stored ``[rows held, 1]`` (1/D of the element-wise accumulator), an untouched row keeps
``h`` and ``W``.  Whole tables and row-range shards apply their coalesced payload with
fm_emb_rowwise_adagrad_apply; tables replicated over R ranks all-gather the payloads as sparse
data parallelism does, merge the R segments in replica-rank order (summed BEFORE squaring, the
same fp32 operations on every replica) and apply the merged payload, so the replicas' ``W`` and
``h`` stay bit-identical.  Rejected at compile: column-split tables (a row's sum of squares would
span ranks), host-placed tables, ``weight_decay != 0`` with a table in the model, and replicated
tables with ``FLEXMI_SPARSE_DP=0``.

Which of these paths trains a table is decided in one function, ``Embedding.table_rule``
(``flexmi/ops/embedding.py``): it alone reads ``sparse_capable``, ``sparse_dp_capable``,
``sparse_dp_always``, ``epsilon`` and ``weight_decay`` and answers a ``TableRule`` (kind, epsilon,
replica set, host placement; the shape of the table's state), ``None`` for the dense path, or the
reason a placement is rejected.  The executor trains by that answer and the strategy search
prices it.

Not provided: host-placed tables under either Adagrad, ``lr_decay``, and Adagrad in the native
C++ engine.
"""
from __future__ import annotations

import math

import torch


class Optimizer:
    def __init__(self, ffmodel=None):
        self.model = ffmodel

    def next(self):
        pass

    def state_names(self):
        return []

    def state_init(self, name):
        """Initial value of every element of the state buffer ``name`` (the executor fills the
        dense groups, the ZeRO shards and the sparse tables' state with it)."""
        return 0.0

    # replicated tables trained by touched-row exchange (Embedding.sdp_*): an SGD form only
    sparse_dp_capable = False

    # ---- the dense update.  A rule answers two things: update_torch(w, g, state, step=None), the
    # update as torch arithmetic, and update_hip(w, g, state, comp, step, zero_grad), its HIP launch
    # (bf16 mirror ``comp`` or None; zero_grad: the kernel leaves the consumed gradient zeroed).
    # ``step`` is the device scalar the executor steps with; without one update_torch uses the
    # host value.
    def device_step(self, ex):
        """The device scalar of executor ``ex`` this rule steps with."""
        return ex.lr_tensor

    def advance_device(self, counters):
        """Advance the executor's device-side step counters (only Adam keeps any)."""

    def update(self, ex, w, g, state, comp, zero_grad):
        """One step of executor ``ex`` over flat fp32 master ``w``, gradient ``g`` and ``state``."""
        step = self.device_step(ex)
        if ex.backend == "hip":
            self.update_hip(w, g, state, comp, step, zero_grad)
        else:
            self.update_torch(w, g, state, step)
            if comp is not None:
                comp.copy_(w)

    def state_dict(self):
        return {}

    def load_state_dict(self, d):
        pass


class SGDOptimizer(Optimizer):
    def __init__(self, ffmodel=None, lr=0.01, momentum=0.0, nesterov=False, weight_decay=0.0):
        super().__init__(ffmodel)
        self.lr = float(lr)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        self.weight_decay = float(weight_decay)

    def set_learning_rate(self, learning_rate):
        self.lr = float(learning_rate)
        if self.model is not None and getattr(self.model, "executor", None) is not None:
            self.model.executor.set_lr(self.lr)

    def state_names(self):
        return ["v"] if self.momentum > 0 else []

    @property
    def sparse_capable(self):
        """Embedding rows can be updated in place (no dense grad) iff the update of an
        untouched row is the identity: no weight decay, no momentum."""
        return self.momentum == 0.0 and self.weight_decay == 0.0

    @property
    def sparse_dp_capable(self):
        return self.sparse_capable

    def update_torch(self, w, g, state, step=None):
        gt = g + self.weight_decay * w
        if self.momentum > 0:
            v = state["v"]
            v.mul_(self.momentum).add_(gt)
            gt = gt + self.momentum * v if self.nesterov else v
        w.sub_((self.lr if step is None else step) * gt)

    @property
    def constants(self):
        """(weight decay, momentum, nesterov): the rule's constants as every SGD launch takes them."""
        return self.weight_decay, self.momentum, self.nesterov

    def update_hip(self, w, g, state, comp, step, zero_grad, segs=None):
        """segs: update only these (offset, length) ranges of the flat buffers, in one launch."""
        from flexmi.ops import _kernels as K
        v = state.get("v") if self.momentum > 0 else None
        if segs is None:
            K.sgd_update(w, g, v, comp, step, *self.constants, zero_grad=zero_grad)
        else:
            K.C().sgd_segs(w, g, v, comp, step, [s[0] for s in segs], [s[1] for s in segs], *self.constants, zero_grad)

    def state_dict(self):
        return {"lr": self.lr}

    def load_state_dict(self, d):
        self.lr = d.get("lr", self.lr)


class AdamOptimizer(Optimizer):
    def __init__(self, ffmodel=None, alpha=0.001, beta1=0.9, beta2=0.999, weight_decay=0.0, epsilon=1e-8):
        super().__init__(ffmodel)
        self.alpha = float(alpha)
        self.beta1 = float(beta1)
        self.beta2 = float(beta2)
        self.weight_decay = float(weight_decay)
        self.epsilon = float(epsilon)
        self.beta1_t = 1.0
        self.beta2_t = 1.0
        self.alpha_t = self.alpha

    @property
    def lr(self):
        return self.alpha

    def set_learning_rate(self, learning_rate):
        self.alpha = float(learning_rate)

    sparse_capable = False

    def next(self):
        """``AdamOptimizer::next`` (``src/runtime/optimizer.cc:167-173``)."""
        self.beta1_t *= self.beta1
        self.beta2_t *= self.beta2
        self.alpha_t = self.alpha * math.sqrt(1 - self.beta2_t) / (1 - self.beta1_t)

    def state_names(self):
        return ["m", "v"]

    def device_step(self, ex):
        return ex.adam_state[2:3]

    def advance_device(self, counters):
        """``next()`` on the executor's device-side ``[β1ᵗ, β2ᵗ, α_t]``: three in-place tensor ops,
        so the step stays graph-capturable."""
        counters[0:1].mul_(self.beta1)
        counters[1:2].mul_(self.beta2)
        counters[2:3].copy_(self.alpha * torch.sqrt(1 - counters[1:2]) / (1 - counters[0:1]))

    def update_torch(self, w, g, state, step=None):
        gt = g + self.weight_decay * w
        m, v = state["m"], state["v"]
        m.mul_(self.beta1).add_((1 - self.beta1) * gt)
        v.mul_(self.beta2).add_((1 - self.beta2) * gt * gt)
        w.sub_((self.alpha_t if step is None else step) * m / (v.sqrt() + self.epsilon))

    def update_hip(self, w, g, state, comp, step, zero_grad):
        from flexmi.ops import _kernels as K
        K.adam_update(w, g, state["m"], state["v"], comp, step, self.beta1, self.beta2, self.weight_decay, self.epsilon,
                      zero_grad=zero_grad)

    def state_dict(self):
        return {"alpha": self.alpha, "beta1_t": self.beta1_t, "beta2_t": self.beta2_t, "alpha_t": self.alpha_t}

    def load_state_dict(self, d):
        for k, v in d.items():
            setattr(self, k, v)


class AdagradOptimizer(Optimizer):
    """Element-wise Adagrad, ``torch.optim.Adagrad`` with ``lr_decay = 0``."""

    def __init__(self, ffmodel=None, lr=0.01, epsilon=1e-10, weight_decay=0.0, initial_accumulator_value=0.0):
        super().__init__(ffmodel)
        self.lr = float(lr)
        self.epsilon = float(epsilon)
        self.weight_decay = float(weight_decay)
        self.initial_accumulator_value = float(initial_accumulator_value)
        if self.initial_accumulator_value < 0:
            raise ValueError("initial_accumulator_value must be >= 0")

    def set_learning_rate(self, learning_rate):
        self.lr = float(learning_rate)
        if self.model is not None and getattr(self.model, "executor", None) is not None:
            self.model.executor.set_lr(self.lr)

    def state_names(self):
        return ["h"]

    def state_init(self, name):
        return self.initial_accumulator_value

    @property
    def sparse_capable(self):
        """A row no lookup touched has gradient 0 and keeps H and W iff there is no weight decay."""
        return self.weight_decay == 0.0

    # replicated tables stay dense: the replica all-reduce sums the gradients before they are squared
    sparse_dp_capable = False

    def update_torch(self, w, g, state, step=None):
        gt = g + self.weight_decay * w
        h = state["h"]
        h.addcmul_(gt, gt)
        w.sub_((self.lr if step is None else step) * gt / (h.sqrt() + self.epsilon))

    def update_hip(self, w, g, state, comp, step, zero_grad):
        from flexmi.ops import _kernels as K
        K.adagrad_update(w, g, state["h"], comp, step, self.weight_decay, self.epsilon, zero_grad=zero_grad)

    def state_dict(self):
        return {"lr": self.lr}

    def load_state_dict(self, d):
        self.lr = d.get("lr", self.lr)


class RowwiseAdagradOptimizer(AdagradOptimizer):
    """Row-wise Adagrad: dense parameters exactly as :class:`AdagradOptimizer`; every embedding
    table sparsely with one fp32 accumulator per row, ``h[r] += mean_c(G[r,c]^2)``,
    ``W[r,:] -= lr * G[r,:] / (sqrt(h[r]) + eps)`` (module docstring)."""

    # a table has no dense path under this optimizer: it is always sparse, replicated ones by the
    # merged touched-row exchange
    sparse_capable = True
    sparse_dp_capable = True
    sparse_dp_always = True     # whatever the byte comparison of Embedding.sdp_prefer_sparse says

    def table_pc_ok(self, op, pc):
        """False for a table placement ``Embedding.table_rule`` rejects (its ``colsplit`` input) -- a
        column split (a row's sum of squares would span ranks)."""
        return op._grid(pc)[1] == 1

    def table_state_bytes(self, rows, cols):
        """Optimizer state of a table shard of ``rows x cols``: one fp32 per row."""
        return 4.0 * rows
