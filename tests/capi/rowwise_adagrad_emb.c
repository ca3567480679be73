/* An MLP with an embedding bag trained for two steps with row-wise Adagrad through flexmi_c.h;
 * prints every parameter with nine significant digits (exact for fp32) for
 * tests/test_capi_rowwise_adagrad.py to compare with the Python API run.  Data:
 * x[i][j] = ((31 i + 17 j) mod 97) / 97, idx[i][k] = (5 i + 3 k) mod 20 (rows repeat within the
 * batch), label[i] = 7 i mod 4. */
#include <stdio.h>
#include <stdlib.h>

#include "flexmi_c.h"

#define CHECK(x)                                                             \
  do {                                                                       \
    if (!(x)) {                                                              \
      fprintf(stderr, "%s failed: %s\n", #x, flexmi_last_error());           \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main(int argc, char** argv) {
  CHECK(flexmi_init(argc, argv) == 0);
  flexmi_config_t cfg = flexmi_config_create();
  CHECK(cfg);
  CHECK(flexmi_config_parse_args_default(cfg) == 0);
  const int B = 16, F = 12, C = 4, N = 32, ROWS = 20, D = 8, BAG = 2;
  CHECK(flexmi_config_set_batch_size(cfg, B) == 0);
  CHECK(flexmi_config_set_device(cfg, "cpu") == 0);

  flexmi_model_t m = flexmi_model_create(cfg);
  CHECK(m);
  int dims[2] = {B, F};
  flexmi_tensor_t x = flexmi_tensor_create(m, 2, dims, 40, 1, "input");
  CHECK(x);
  int idims[2] = {B, BAG};
  flexmi_tensor_t idx = flexmi_tensor_create(m, 2, idims, 42, 0, "indices");
  CHECK(idx);
  flexmi_tensor_t t = flexmi_model_add_dense(m, x, D, 11, 1, NULL, NULL, "dense1");
  CHECK(t);
  flexmi_tensor_t e = flexmi_model_add_embedding(m, idx, ROWS, D, 21, NULL, "table");
  CHECK(e);
  t = flexmi_model_add_add(m, t, e, "add");
  CHECK(t);
  t = flexmi_model_add_dense(m, t, C, 10, 1, NULL, NULL, "dense2");
  t = flexmi_model_add_softmax(m, t, "softmax");
  CHECK(t);
  flexmi_optimizer_t opt = flexmi_rowwise_adagrad_optimizer_create(m, 0.1, 1e-10, 0.0, 0.1);
  CHECK(opt);
  CHECK(flexmi_model_set_adagrad_optimizer(m, opt) == 0);
  int metrics[1] = {1001};
  CHECK(flexmi_model_compile(m, opt, 51, metrics, 1) == 0);
  CHECK(flexmi_model_init_layers(m) == 0);
  CHECK(flexmi_optimizer_set_lr(opt, 0.05) == 0);

  float* xs = (float*)malloc(sizeof(float) * N * F);
  int* ys = (int*)malloc(sizeof(int) * N);
  int* is = (int*)malloc(sizeof(int) * N * BAG);
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < F; ++j) xs[i * F + j] = (float)((31 * i + 17 * j) % 97) / 97.0f;
    for (int k = 0; k < BAG; ++k) is[i * BAG + k] = (5 * i + 3 * k) % ROWS;
    ys[i] = (7 * i) % 4;
  }
  flexmi_tensor_t label = flexmi_model_get_label_tensor(m);
  flexmi_dataloader_t dx = flexmi_single_dataloader_create(m, x, xs, N, 40);
  flexmi_dataloader_t dy = flexmi_single_dataloader_create(m, label, ys, N, 42);
  flexmi_dataloader_t di = flexmi_single_dataloader_create(m, idx, is, N, 42);
  CHECK(dx && dy && di);
  for (int it = 0; it < 2; ++it) {
    CHECK(flexmi_dataloader_next_batch(dx, m) == 0);
    CHECK(flexmi_dataloader_next_batch(dy, m) == 0);
    CHECK(flexmi_dataloader_next_batch(di, m) == 0);
    CHECK(flexmi_model_forward(m) == 0);
    CHECK(flexmi_model_zero_gradients(m) == 0);
    CHECK(flexmi_model_backward(m) == 0);
    CHECK(flexmi_model_update(m) == 0);
  }
  for (int p = 0; p < 5; ++p) {
    flexmi_parameter_t w = flexmi_model_get_parameter_by_id(m, p);
    CHECK(w);
    const int n = flexmi_parameter_get_num_elements(w);
    float* buf = (float*)malloc(sizeof(float) * n);
    CHECK(flexmi_parameter_get_weights_float(w, m, buf, (size_t)n) == 0);
    printf("param %d %d", p, n);
    for (int i = 0; i < n; ++i) printf(" %.9g", buf[i]);
    printf("\n");
    free(buf);
    flexmi_parameter_destroy(w);
  }
  flexmi_dataloader_destroy(dx);
  flexmi_dataloader_destroy(dy);
  flexmi_dataloader_destroy(di);
  flexmi_tensor_destroy(label);
  flexmi_optimizer_destroy(opt);
  flexmi_model_destroy(m);
  flexmi_config_destroy(cfg);
  flexmi_finalize();
  free(xs);
  free(ys);
  free(is);
  return 0;
}
