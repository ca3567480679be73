// The one declaration of every public kernel launcher of csrc/kernels/*.hip.  The launchers are
// extern "C", so nothing but a shared prototype checks a caller against a definition: every .hip
// file sees this header through common.h (a definition that disagrees with it is a "conflicting
// types" error), and the callers (csrc/bindings/hip_ops.cpp, csrc/native/native_hip.cc) include it
// and declare nothing themselves.  Plain C++, for hipcc and for g++ -D__HIP_PLATFORM_AMD__=1.
// The kernel-internal launchers fm_gemm_x3v2_launch / _grouped take kernel-private parameter
// structs and are declared with them in gemm_epilogue.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include "../runtime/gemm_group_plan.h"

extern "C" {

// gemm.hip
int fm_gemm(const void* A, long lda, long sA, int a_kcontig, const void* B, long ldb, long sB, int b_kcontig, void* C,
            long ldc, long sC, int c_fp32, const float* bias, int M, int N, int K, int batch, float alpha, int beta,
            int act, float* ws, long ws_bytes, int ksplit_req, const void* act_y, long lday, int bwd_act, float* colsum,
            float* rowsum_a, hipStream_t stream);
int fm_gemm_dw_sgd(const void* A, long lda, const void* B, long ldb, float* W, long ldw, unsigned short* Wc, float* V,
                   const float* lr, float wd, float mom, int nesterov, int M, int N, int K, float* ws, long ws_bytes,
                   float* rowsum_a, int cfg, hipStream_t stream);
void fm_skinny_fwd(const void* x, long ldx, const void* w, const float* bias, void* y, long ldy, long B, int K, int act,
                   hipStream_t s);
// bact (also in fm_skinny_bwd_f32_launch): activation backward of the layer below (output x) fused into dX; 10 = none
void fm_skinny_bwd(const void* x, long ldx, const void* w, const void* y, long ldy, const void* dy, long lddy, void* dx,
                   long lddx, int dx_acc, float* dw, float* db, long B, int K, int act, int bact, hipStream_t s);

// gemm_f32.hip
void fm_gemm_f32_set_split(int on);
void fm_gemm_set_dma(int on);
int fm_gemm_dma_enabled();   // as in gemm_common.h, which the kernels call it through
int fm_gemm_f32_get_split();
int fm_gemm_f32_last_form();
int fm_gemm_f32(const float* A, long lda, long sA, int a_kcontig, const float* B, long ldb, long sB, int b_kcontig,
                float* C, long ldc, long sC, const float* bias, int M, int N, int K, int batch, float alpha, int beta,
                int act, float* ws, long ws_bytes, int ksplit_req, const float* act_y, long lday, int bwd_act,
                float* colsum, float* rowsum_a, hipStream_t stream);
int fm_gemm_f32_dw_sgd(const float* A, long lda, const float* B, long ldb, float* W, long ldw, unsigned short* Wc,
                       float* V, const float* lr, float wd, float mom, int nesterov, int M, int N, int K, float* ws,
                       long ws_bytes, float* rowsum_a, int cfg, hipStream_t stream);
long fm_gemm_f32_grouped_count();
int fm_gemm_f32_grouped(const flexmi::GemmGroupItem* items, int n, int a_kcontig, int b_kcontig, float* ws,
                        long ws_bytes, int force, int cus, int* ks_out, hipStream_t stream);
void fm_skinny_fwd_f32_launch(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, long B,
                              int K, int act, hipStream_t s);
void fm_skinny_bwd_f32_launch(const float* x, long ldx, const float* w, const float* y, long ldy, const float* dy,
                              long lddy, float* dx, long lddx, int dx_acc, float* dw, float* db, long B, int K, int act,
                              int bact, hipStream_t s);

// gemm_small.hip
int fm_smallk_fwd_launch(const void* x, long ldx, const void* w, const float* bias, void* y, long ldy, long M, int K,
                         int N, int act, int bf16, hipStream_t s);
int fm_smallk_dw_launch(const void* dpre, long ldd, const void* x, long ldx, float* dw, float* db, long M, int K, int N,
                        float* ws, long ws_bytes, float* V, unsigned short* Wc, const float* lr, float wd, float mom,
                        int nesterov, int bf16, hipStream_t s);

// embedding.hip
void fm_embedding_fwd_multi(int n, const float* const* W, const void* const* idx, const int* idx64, void* const* out,
                            const long* ldo, const long* lo, const int* rows, const int* D, const int* bag,
                            const float* scale, int out_bf16, long B, hipStream_t st);
void fm_embedding_set_fwd_mode(int mode);
void fm_embedding_fwd_last_form(int* out);
// claim, optional per table: owner (int32 [rows], -1 filled), dups (int32 [B * bag]), ndup (int32 [1])
void fm_embedding_bwd_multi(int n, float* const* W, const void* const* idx, const int* idx64, const void* const* dy,
                            const long* ldg, const long* lo, const int* rows, const int* D, const int* bag,
                            const float* scale, int dy_bf16, const float* lr, long B, int* const* owner,
                            int* const* dups, int* const* ndup, hipStream_t st);
void fm_embedding_fwd(const void* idx, int idx64, const float* W, void* out, int out_bf16, long B, int bag, int rows,
                      int D, long ldo, float scale, hipStream_t s);
void fm_embedding_bwd(const void* idx, int idx64, const void* dy, int dy_bf16, float* W, const float* lr, long B,
                      int bag, int rows, int D, long ldg, float scale, hipStream_t s);
void fm_sdp_coalesce(int n, const void* const* idx, const int* idx64, const void* const* dy, const long* ldg,
                     const long* lo, const int* rows, const int* D, const int* bag, const float* scale, int dy_bf16,
                     long B, int* const* slot, int* const* cid, int* const* ids, float* const* g, int* const* count,
                     hipStream_t st);
void fm_sdp_apply_segments(int n, int segs, int own_seg, float* const* W, const int* D, const int* const* seg_ids,
                           const float* const* seg_g, const int* const* seg_count, int* const* slot,
                           int* const* own_count, const int* nmax, const float* lr, hipStream_t st);
void fm_emb_adagrad_apply(int n, float* const* W, float* const* H, const int* D, const int* const* ids,
                          const float* const* g, int* const* count, int* const* slot, const int* nmax, const float* lr,
                          float eps, hipStream_t st);
void fm_emb_rowwise_adagrad_apply(int n, float* const* W, float* const* h, const int* D, const int* const* ids,
                                  const float* const* g, int* const* count, int* const* slot, const int* nmax,
                                  const float* lr, float eps, hipStream_t st);
void fm_sdp_rowwise_merge_segments(int n, int segs, const int* rows, const int* D, const int* const* seg_ids,
                                   const float* const* seg_g, const int* const* seg_count, const int* const* own_ids,
                                   int* const* own_count, int* const* slot, int* const* mids, float* const* mg,
                                   int* const* mcount, const int* nmax, const int* mcap, hipStream_t st);

// interaction.hip
void fm_dot_interaction_fwd_f32(const float* const* z, int F, long ldz, float* out, long ldo, long B, int D, int W,
                                int self, hipStream_t s);
// act0: activation backward of feature 0's producer applied to dz[0]; 10 = none
void fm_dot_interaction_bwd_f32(const float* const* z, int F, long ldz, const float* dout, long ldo, float* const* dz,
                                long lddz, unsigned acc_mask, long B, int D, int self, int act0, hipStream_t s);
void fm_dot_interaction_fwd(const void* const* z, int F, long ldz, void* out, long ldo, long B, int D, int W, int self,
                            hipStream_t s);
void fm_dot_interaction_bwd(const void* const* z, int F, long ldz, const void* dout, long ldo, void* const* dz,
                            long lddz, unsigned acc_mask, long B, int D, int self, hipStream_t s);

// cross.hip
void fm_cross_forward(const void* x0, const void* t, const void* x, void* y, long n, int bf16, hipStream_t s);
void fm_cross_backward(const void* dy, const void* x0, const void* t, void* dt, void* dx0, void* dx, long n, int acct,
                       int acc0, int accx, int self, int bf16, hipStream_t s);

// optim.hip
void fm_sgd_update(float* W, float* G, float* V, unsigned short* Wc, const float* lr, long n, float wd, float mom,
                   int nesterov, int zero_g, hipStream_t s);
void fm_sgd_update_segs(float* W, float* G, float* V, unsigned short* Wc, const float* lr, const long* off,
                        const long* len, int nseg, float wd, float mom, int nesterov, int zero_g, hipStream_t s);
void fm_adam_update(float* W, float* G, float* M, float* V, unsigned short* Wc, long n, const float* alpha_t, float b1,
                    float b2, float wd, float eps, int zero_g, hipStream_t s);
void fm_adagrad_update(float* W, float* G, float* H, unsigned short* Wc, const float* lr, long n, float wd, float eps,
                       int zero_g, hipStream_t s);
void fm_cast_bf16(const float* src, unsigned short* dst, long n, hipStream_t s);

// loss.hip
void fm_loss_fwd_bwd(const void* logits, int logits_bf16, const void* labels, void* grad, int grad_bf16, long B, int C,
                     int loss_type, float scale, float* acc, int mask, float clamp_t, hipStream_t s);

// auc.hip
void fm_auc_hist_variant(const void* scores, int scores_bf16, const float* labels, long B, long long* hist,
                         long long* invalid, int shift, int rounds, hipStream_t s);

// elementwise.hip
void fm_unary_forward(int code, const void* x, void* y, long n, int bf16, hipStream_t s);
void fm_unary_backward(int code, const void* x, const void* y, const void* dy, void* dx, long n, int acc, int bf16,
                       hipStream_t s);
void fm_binary_forward(int code, const void* a, const void* b, void* y, long n, int relu, int bf16, hipStream_t s);
void fm_binary_backward(int code, const void* a, const void* b, const void* dy, const void* ymask, void* da, void* db,
                        long n, int acca, int accb, int bf16, hipStream_t s);
void fm_act_bwd_bias(const void* y, const void* dy, void* dpre, float* db, long B, int N, int act, int bf16,
                     hipStream_t s);
void fm_multi_copy2d(int n, const void* const* src, void* const* dst, const long* rows, const long* cols,
                     const long* lds, const long* ldd, int add_mask, int elem_bytes, hipStream_t s);
void fm_permute_nd(const void* x, void* y, int nd, const long* out_dims, const long* in_strides_perm, int acc, int bf16,
                   hipStream_t s);
void fm_reverse_axis(const void* x, void* y, long outer, long len, long inner, int acc, int bf16, hipStream_t s);
void fm_softmax_fwd(const void* x, void* y, long rows, int C, int bf16, hipStream_t s);
void fm_dropout_apply(const void* x, void* y, long n, float rate, unsigned seed, unsigned step, int acc, int bf16,
                      hipStream_t s);

// init.hip
void fm_init_fill(float* out, long rows, long cols, long r0, long c0, long ldg, int kind, unsigned seed, float a,
                  float b, hipStream_t s);

// image.hip
void fm_image_normalize(const unsigned char* src, void* dst, long N, int H, int W, const float* mean, const float* stdv,
                        int bf16, hipStream_t s);

// cnn.hip
void fm_im2col(const void* x, void* col, int N, int C, int H, int W, int R, int S, int P, int Q, int sh, int sw, int pt,
               int pl, int ldcol, int bf16, hipStream_t st);
void fm_col2im(const void* dcol, void* dx, int N, int C, int H, int W, int R, int S, int P, int Q, int sh, int sw,
               int pt, int pl, int ldcol, int acc, int bf16, hipStream_t st);
void fm_transpose_batched(const void* in, const void* yin, void* out, int N, int A, int B, int act, int mode, int bf16,
                          hipStream_t st);
void fm_pool_fwd(const void* x, void* y, unsigned char* code, int N, int C, int H, int W, int P, int Q, int kh, int kw,
                 int sh, int sw, int pt, int pl, int is_max, int act, int bf16, hipStream_t st);
void fm_pool_bwd(const void* x, const void* y, const void* dy, void* dx, unsigned char* code, int code_ready, int N,
                 int C, int H, int W, int P, int Q, int kh, int kw, int sh, int sw, int pt, int pl, int is_max, int act,
                 int acc, int bf16, hipStream_t st);
void fm_pool_last_form(int* out);
void fm_bn_fwd(const void* x, void* y, const float* gamma, const float* beta, float* stats, float* meaninv, int N,
               int C, int HW, float eps, int relu, int bf16, hipStream_t st);
void fm_bn_bwd(const void* x, const void* y, const void* dy, const float* meaninv, const float* gamma, float* gsum,
               float* dgamma, float* dbeta, void* dx, int N, int C, int HW, int relu, int acc, int bf16,
               hipStream_t st);
void fm_pad_rows(const void* src, void* dst, int K, int n, int ldp, int bf16, hipStream_t st);
void fm_strided_copy4_run(const void* src, void* dst, int bf16, const int* d, const long* ss, const long* ts, long so,
                          long to, int acc, hipStream_t st);
void fm_compact_rows(const float* src, float* dst, int K, int n, int ldp, int acc, hipStream_t st);

// conv_igemm.hip
int fm_conv_lda(int cols);
int fm_conv_fwd(const void* x, const void* w, void* wpad, const float* bias, void* y, int bf16, int N, int C, int H,
                int W, int K, int R, int S, int P, int Q, int sh, int sw, int pt, int pl, int act, hipStream_t s);
int fm_conv_dgrad(const void* g, const void* w, void* wt, void* dx, int accum, int bf16, int N, int C, int H, int W,
                  int K, int R, int S, int P, int Q, int sh, int sw, int pt, int pl, hipStream_t s);
int fm_conv_wgrad(const void* g, const void* x, float* dw, int bf16, int N, int C, int H, int W, int K, int R, int S,
                  int P, int Q, int sh, int sw, int pt, int pl, hipStream_t s);
void fm_conv_act_bwd(const void* dy, const void* y, void* g, float* db, int bf16, int N, int K, int PQ, int act,
                     hipStream_t s);
void fm_conv_s2d_run(const void* x, void* xs, int bf16, int N, int C, int H, int W, int s, int pt, int pl, int Hs,
                     int Ws, int inv, int acc, hipStream_t st);
void fm_conv_w_s2d_run(const void* w, void* ws, const float* dws, float* dw, int bf16, int K, int C, int R, int S,
                       int s, int Rs, int Ss, int inv, hipStream_t st);

// conv_stem.hip
int fm_stem_supported(int C, int K, int R, int S, int sh, int sw);
long fm_stem_wf_elems(int C, int K, int R, int S, int s);
long fm_stem_wgrad_ws(int C, int K, int R, int S, int s);
int fm_stem_fwd_run(const void* x, const void* w, void* wf, const float* bias, void* y, int N, int C, int H, int W,
                    int R, int S, int P, int Q, int s, int pt, int pl, int act, hipStream_t st);
int fm_stem_wgrad_run(const void* x, const void* y, const void* dy, float* dw, float* db, float* ws, int N, int C,
                      int H, int W, int R, int S, int P, int Q, int s, int pt, int pl, int act, hipStream_t st);

// conv_nhwc.hip
void fm_conv_nhwc_set_shape(int mode, int shape);
void fm_nhwc_stage_run(const void* src, void* dst, int N, int C, int H, int W, int Cp, int Hp, int Wp, int top,
                       int left, int dh, int dw, hipStream_t s);
void fm_nhwc_stage_grad_run(const void* dy, const void* y, void* dst, int act, int N, int C, int H, int W, int Cp,
                            int Hp, int Wp, int top, int left, int dh, int dw, hipStream_t s);
void fm_cnhwc_wprep_run(const void* w, void* out, void* out2, const float* g2, float* dw, int K, int C, int R, int S,
                        int Cp, int Kp, int mode, int nsplit, hipStream_t s);
void fm_cnhwc_wprep_multi_run(int n, const void* const* w, void* const* out, void* const* out2, const int* K,
                              const int* C, const int* R, const int* S, const int* Cp, const int* Kp, hipStream_t s);
long fm_conv_nhwc_wgrad_ws(int N, int K, int P, int Q, int R, int S, int Cp);
void fm_conv_nhwc_fwd(const void* xs, long xs_bytes, const void* wf, const float* bias, void* y, int N, int K, int P,
                      int Q, int R, int S, int Cp, int Hp, int Wp, int sh, int sw, int act, void* out2, int H2, int W2,
                      int C2, int t2, int l2, int d2h, int d2w, int write_nchw, hipStream_t s);
void fm_conv_nhwc_dgrad(const void* gs, long gs_bytes, const void* wd, void* dx, int accum, int N, int C, int H, int W,
                        int R, int S, int Kp, int Hg, int Wg, void* out2, int H2, int W2, int C2, int t2, int l2,
                        int d2h, int d2w, int write_nchw, hipStream_t s);
int fm_conv_nhwc_wgrad(const void* gs, long gs_bytes, const void* xs, long xs_bytes, float* g2, float* db, int N, int K,
                       int Kp, int P, int Q, int Hg, int Wg, int gt, int gl, int gsh, int gsw, int R, int S, int Cp,
                       int Hp, int Wp, int sh, int sw, int* ptab, int build_tab, hipStream_t s);
void fm_conv_nhwc_dgrad_strided(const void* gs, long gs_bytes, const void* w, void* wsub, void* dx, int accum, int N,
                                int C, int H, int W, int K, int R, int S, int Kp, int Hg, int Wg, int gt, int gl,
                                int sh, int sw, void* out2, int H2, int W2, int C2, int t2, int l2, int d2h, int d2w,
                                int write_nchw, hipStream_t s);

// lstm.hip
void fm_lstm_init(const void* h0, const void* c0, void* hprev, long ldhp, float* cinit, int B, int H, int bf16,
                  hipStream_t s);
void fm_lstm_cell_fwd(float* G, long ldg, const float* c_prev, long ldcp, float* c_out, long ldc, void* y, long ldy,
                      void* hprev_next, long ldhp, void* hT, void* cT, int B, int H, int bf16, hipStream_t s);
void fm_lstm_cell_bwd(const float* A, long lda, const float* c_t, long ldc, const float* c_prev, long ldcp,
                      const void* dy, long ldy, const float* dh, float* dc, void* dG, long lddg, int B, int H, int bf16,
                      hipStream_t s);

}  // extern "C"
