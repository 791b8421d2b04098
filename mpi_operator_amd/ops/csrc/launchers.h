// The one declaration of every extern "C" entry point of the kernel TUs.
// Pure HIP/C++ (no torch headers). Every .hip file and bindings.cpp include
// it: extern "C" symbols are not mangled, so a caller's declaration that
// disagreed with the definition in arity, order or a struct field would link
// cleanly and run with shifted arguments — with one shared declaration the
// compiler rejects the disagreement instead. Parameter names are those of
// the definitions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Per-tensor descriptors of the multi-tensor optimizer launches (passed by
// value inside the kernels' argument blocks: the field order is device ABI).
struct SgdDesc {
  const void *grad;
  float *master;
  float *mom;
  uint16_t *out; // nullptr if the param itself is fp32 (master IS the param)
  long numel;
};

struct OptDesc {
  const void *grad;
  float *master;
  float *m;
  float *v;
  uint16_t *out; // nullptr if the param itself is fp32 (master IS the param)
  long numel;
};

extern "C" {

// ---- elementwise.hip ----
hipError_t add_bf16(const void *a, const void *b, void *c, long n,
                    hipStream_t s);
hipError_t add_relu_fwd(const void *a, const void *b, void *y, long n,
                        hipStream_t s);
hipError_t add_relu_bwd_add_mask(const void *dy, const void *mask,
                                 const void *dx0, void *dxt, long n,
                                 hipStream_t s);
hipError_t add_relu_bwd_add(const void *dy, const void *y, const void *dx0,
                            void *dxt, long n, hipStream_t s);
hipError_t add_relu_bwd(const void *dy, const void *y, void *dx, long n,
                        hipStream_t s);
hipError_t gap_fwd(const void *x, void *y, int N, int HW, int C,
                   hipStream_t s);
hipError_t gap_bwd(const void *dy, void *dx, int N, int HW, int C,
                   hipStream_t s);
hipError_t sgd_step_launch(const SgdDesc *descs, int nt, int grad_is_bf16,
                           float lr, float mu, float wd, int nesterov,
                           hipStream_t s);
hipError_t bias_add(void *y, const float *b, long M, int N, hipStream_t s);
int colsum_chunks(long M, int N);
hipError_t colsum_bf16(const void *dy, float *partial, float *db, long M,
                       int N, long ld, hipStream_t s);

// ---- batchnorm.hip ----
hipError_t bn_fwd_train_launch(const void *x, const void *res,
                               const float *gamma, const float *beta,
                               float eps, int relu, void *y,
                               uint8_t *relu_mask, float *mean, float *invstd,
                               float *scale, float *shift, float *partial,
                               float *running_mean, float *running_var,
                               float momentum, long M, int C, hipStream_t s);
hipError_t bn_fwd_train_pre_launch(const float *pre_partial, int pre_grid,
                                   const void *x, const void *res,
                                   const float *gamma, const float *beta,
                                   float eps, int relu, void *y,
                                   uint8_t *relu_mask, float *mean,
                                   float *invstd, float *scale, float *shift,
                                   float *running_mean, float *running_var,
                                   float momentum, long M, int C,
                                   hipStream_t s);
hipError_t bn_fwd_eval_launch(const void *x, const float *scale,
                              const float *shift, int relu, void *y, long M,
                              int C, hipStream_t s);
hipError_t bn_bwd_launch(const void *dy, const void *x, const void *y,
                         const uint8_t *relu_mask, const float *gamma,
                         const float *mean, const float *invstd, int relu,
                         void *dx, float *dgamma, float *dbeta, float *k1,
                         float *k2, float *k3, float *partial, long M, int C,
                         hipStream_t s);
int bn_stats_grid(long M, int C);
// process-wide A/B switches (each returns the previous value): pipelined
// statistics producers, line-coalesced finalize, and the finalize slice width
// override tools/bn_bench.py uses (0 table, -1 bands, 8 or 16; -2 = rejected)
int bn_set_pipelined(int on);
int bn_set_finalize_coalesced(int on);
int bn_set_finalize_ch(int ch);
hipError_t bn_reduce_stats_fwd_launch(const float *slabs, int splits, void *y,
                                      float *partial, long M, int C,
                                      hipStream_t s);
hipError_t bn_reduce_stats_bwd_launch(const float *slabs, int splits, void *dy,
                                      const void *x, const void *y,
                                      const uint8_t *relu_mask,
                                      const float *mean, const float *invstd,
                                      int relu, float *partial, long M, int C,
                                      hipStream_t s);
hipError_t bn_join_stats_launch(const void *a, const uint8_t *jmask,
                                const void *b, void *dxt, const uint8_t *cmask,
                                const void *x, const float *mean,
                                const float *invstd, float *partial,
                                const void *xd, const float *mean_d,
                                const float *invstd_d, float *partial_d,
                                long M, int C, hipStream_t s);
hipError_t bn_bwd_pre_launch(const float *pre_partial, int pre_grid,
                             const void *dy, const void *x, const void *y,
                             const uint8_t *relu_mask, const float *gamma,
                             const float *mean, const float *invstd, int relu,
                             void *dx, float *dgamma, float *dbeta, float *k1,
                             float *k2, float *k3, long M, int C,
                             hipStream_t s);

// ---- pooling.hip ----
hipError_t maxpool_fwd_launch(const void *x, void *y, uint8_t *idx, int N,
                              int H, int W, int HO, int WO, int C, int K,
                              int stride, int pad, hipStream_t s);
hipError_t maxpool_bwd_launch(const void *dy, const uint8_t *idx, void *dx,
                              int N, int H, int W, int HO, int WO, int C,
                              int K, int stride, int pad, hipStream_t s);

// ---- softmax_xent.hip ----
hipError_t softmax_xent_fwd_launch(const void *logits, const long *target,
                                   float *probs, float *loss, int B, int V,
                                   hipStream_t s);
hipError_t softmax_xent_bwd_launch(const float *probs, const long *target,
                                   void *dlogits, int B, int V,
                                   const float *dscale, hipStream_t s);

// ---- masked_xent.hip ----
hipError_t masked_xent_fwd_launch(const void *logits, const long *target,
                                  float *stats, float *out, int B, int V,
                                  long ld, long ignore_index, hipStream_t s);
hipError_t masked_xent_bwd_launch(const void *logits, const long *target,
                                  const float *stats, const float *out,
                                  const float *dscale, void *dlogits, int B,
                                  int V, long ld, long ignore_index,
                                  hipStream_t s);

// ---- attention.hip ----
hipError_t attn_fwd_launch(const void *qkv, void *ctx, void *probs,
                           const float *mask, int B, int S, int H, float scale,
                           hipStream_t strm);
hipError_t attn_bwd_launch(const void *qkv, const void *dctx,
                           const void *probs, void *dqkv, int B, int S, int H,
                           float scale, hipStream_t strm);
// dropout on P (philox.h attention scheme): state is the device (seed,
// offset) pair, thr and rs from dropout_thr_scale(p); probs carries bf16(P)
// with the sign bit set where dropped and is all the backward needs
hipError_t attn_drop_fwd_launch(const void *qkv, void *ctx, void *probs,
                                const float *mask, const int64_t *state,
                                uint32_t site, uint32_t thr, float rs, int B,
                                int S, int H, float scale, hipStream_t strm);
hipError_t attn_drop_bwd_launch(const void *qkv, const void *dctx,
                                const void *probs, void *dqkv, float rs, int B,
                                int S, int H, float scale, hipStream_t strm);

// ---- flash_attention.hip ----
hipError_t flash_attn_fwd_launch(const void *qkv, void *ctx, float *lse,
                                 const float *mask, int B, int S, int H,
                                 float scale, hipStream_t strm);
hipError_t flash_attn_bwd_launch(const void *qkv, const void *ctx,
                                 const void *dctx, const float *lse,
                                 float *delta, const float *mask, void *dqkv,
                                 int B, int S, int H, float scale,
                                 hipStream_t strm);
// the same with dropout on P; the backward draws the forward's masks again
// from the same (state, site), so state must hold what the forward read
hipError_t flash_attn_drop_fwd_launch(const void *qkv, void *ctx, float *lse,
                                      const float *mask, const int64_t *state,
                                      uint32_t site, uint32_t thr, float rs,
                                      int B, int S, int H, float scale,
                                      hipStream_t strm);
hipError_t flash_attn_drop_bwd_launch(const void *qkv, const void *ctx,
                                      const void *dctx, const float *lse,
                                      float *delta, const float *mask,
                                      const int64_t *state, uint32_t site,
                                      uint32_t thr, float rs, void *dqkv,
                                      int B, int S, int H, float scale,
                                      hipStream_t strm);
// packed ("varlen") forms: N sequence slots back to back in T-row buffers,
// qkv/dqkv [T,3,H,64], ctx/dctx [T,H*64], lse/delta [H,T], cu_seqlens device
// int32 [N+1] (cu[0] = 0, non-decreasing, cu[N] <= T, no length above
// max_seqlen: documented, not checked). max_seqlen sizes the grid only.
// ctx, lse and dqkv rows at or past cu[N] are written as zeros.
hipError_t flash_attn_varlen_fwd_launch(const void *qkv, void *ctx, float *lse,
                                        const int *cu_seqlens, int N, int T,
                                        int max_seqlen, int H, float scale,
                                        hipStream_t strm);
hipError_t flash_attn_varlen_bwd_launch(const void *qkv, const void *ctx,
                                        const void *dctx, const float *lse,
                                        float *delta, const int *cu_seqlens,
                                        void *dqkv, int N, int T,
                                        int max_seqlen, int H, float scale,
                                        hipStream_t strm);
// with dropout on P: sequence n draws the masks of batch row n of a dense
// [N, max_seqlen] batch (philox.h)
hipError_t flash_attn_varlen_drop_fwd_launch(
    const void *qkv, void *ctx, float *lse, const int *cu_seqlens,
    const int64_t *state, uint32_t site, uint32_t thr, float rs, int N, int T,
    int max_seqlen, int H, float scale, hipStream_t strm);
hipError_t flash_attn_varlen_drop_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const int *cu_seqlens, const int64_t *state, uint32_t site,
    uint32_t thr, float rs, void *dqkv, int N, int T, int max_seqlen, int H,
    float scale, hipStream_t strm);

// ---- gemm.hip ----
hipError_t gemm_nt(const void *a, const void *b, void *c, int M, int N, int K,
                   long lda, long ldb, long ldc, int c_f32, hipStream_t s);
hipError_t gemm_nt_bias(const void *a, const void *b, const float *bias,
                        void *c, int M, int N, int K, long lda, long ldb,
                        long ldc, hipStream_t s);
int gemm_fwd_splits(int M, int N, int K);
hipError_t gemm_nt_bias_sk(const void *a, const void *b, const float *bias,
                           float *partial, void *c, int M, int N, int K,
                           long lda, long ldb, long ldc, int splits,
                           hipStream_t s);
hipError_t gemm_nt_gelu_bias(const void *x, const void *w, const float *bias,
                             void *deriv, void *g, int M, int N, int K,
                             long lda, long ldb, long ldc, hipStream_t s);
int gemm_gelubwd_wants_wt(int M, int N, int K);
hipError_t gemm_nt_tn_gelubwd(const void *dy, const void *w, const void *deriv,
                              void *dh, int M, int N, int K, long lda,
                              long ldb, long ldc, void *wt_buf, hipStream_t s);
hipError_t gemm_nt_tn_acc(const void *a, const void *b, void *c, int M, int N,
                          int K, long lda, long ldb, long ldc, hipStream_t s);
hipError_t gemm_nt_tn(const void *a, const void *b, void *c, int M, int N,
                      int K, long lda, long ldb, long ldc, int c_f32,
                      hipStream_t s);
int gemm_nt_tn_splits(int M, int N, int K);
hipError_t gemm_nt_tn_sk(const void *a, const void *b, float *partial, void *c,
                         int M, int N, int K, long lda, long ldb, long ldc,
                         int splits, hipStream_t s);
hipError_t gemm_tn_tn(const void *a, const void *b, void *c, int M, int N,
                      int K, long lda, long ldb, long ldc, int c_f32,
                      hipStream_t s);
int gemm_tn_tn_splits(int M, int N, int K);
hipError_t gemm_tn_tn_sk(const void *a, const void *b, float *partial, void *c,
                         int M, int N, int K, long lda, long ldb, long ldc,
                         int splits, int out_bf16, hipStream_t s);
hipError_t transpose2d_bf16(const void *in, void *out, int R, int C, long ldo,
                            hipStream_t s);
hipError_t mfma_probe(const void *a, const void *b, float *d, hipStream_t s);
int gemm_set_epilogue_vec(int on); // returns the previous value
int gemm_nt_route_id(int M, int N, int K, int splits);

// ---- conv.hip ----
hipError_t conv_fwd(const void *x, const void *w, void *y, int N, int H, int W,
                    int C, int Kout, int R, int S, int stride, int pad, int HO,
                    int WO, int splits, float *partial, hipStream_t strm);
int conv_fwd_bn_rows(long M, int C, int Kout, int R, int S, int stride,
                     int pad, int splits);
hipError_t conv_fwd_bn(const void *x, const void *w, void *y, int N, int H,
                       int W, int C, int Kout, int R, int S, int stride,
                       int pad, int HO, int WO, int splits, float *partial,
                       float *bn_slab, hipStream_t strm);
hipError_t conv_dgrad_1x1_acc(const void *dy, const void *w, void *dx_acc,
                              long M, int C, int Kout, hipStream_t strm);
hipError_t conv_dgrad(const void *dy, const void *w, void *dx, int N, int H,
                      int W, int C, int Kout, int R, int S, int stride,
                      int pad, int HO, int WO, int splits, float *partial,
                      hipStream_t strm);
int conv_dgrad_bn_rows(long M, int C, int Kout, int R, int S, int stride,
                       int splits);
hipError_t conv_dgrad_bn(const void *dy, const void *w, void *dx, int N, int H,
                         int W, int C, int Kout, int R, int S, int pad, int HO,
                         int WO, int splits, float *partial, const void *bx,
                         const void *by, const uint8_t *mask,
                         const float *mean, const float *invstd, int relu,
                         float *bn_slab, hipStream_t strm);
hipError_t splitk_bias_reduce(const float *partial, int splits, long len,
                              int N, const float *bias, void *out,
                              hipStream_t s);
hipError_t slab_colreduce(const float *partial, float *out, int chunks, long N,
                          hipStream_t s);
hipError_t splitk_reduce(const float *partial, int splits, long len, void *out,
                         int out_bf16, hipStream_t s);
hipError_t conv_wgrad_implicit(const void *dy, const void *x, float *partial,
                               void *dw, int N, int H, int W, int C, int Kout,
                               int R, int S, int stride, int pad, int HO,
                               int WO, int splits, int dw_bf16,
                               hipStream_t strm);

// ---- layernorm.hip ----
hipError_t ln_fwd(const void *x, const float *gamma, const float *beta,
                  void *y, float *mean, float *rstd, long M, int N, float eps,
                  hipStream_t s);
hipError_t ln_fwd_add(const void *a, const void *b, const float *gamma,
                      const float *beta, void *sum_out, void *y, float *mean,
                      float *rstd, long M, int N, float eps, hipStream_t s);
hipError_t ln_bwd(const void *dy, const void *x, const float *gamma,
                  const float *mean, const float *rstd, void *dx,
                  float *partial, float *dgamma_dbeta, long M, int N,
                  int *grid_out, hipStream_t s);
hipError_t ln_fwd_drop_add(const void *a, const void *b, const float *gamma,
                           const float *beta, const int64_t *state,
                           uint32_t site, uint32_t thr, float scale,
                           void *sum_out, void *y, float *mean, float *rstd,
                           uint8_t *mask, long M, int N, float eps,
                           hipStream_t s);
hipError_t ln_bwd_drop(const void *dy, const void *x, const float *gamma,
                       const float *mean, const float *rstd,
                       const uint8_t *mask, float scale, void *da, void *db,
                       float *partial, float *dgamma_dbeta, long M, int N,
                       int *grid_out, hipStream_t s);

// ---- dropout.hip ----
// state: the device (seed, offset) pair of philox.h; thr and scale from
// dropout_thr_scale(p); mask: one keep byte per octet
hipError_t rng_tick(int64_t *state, hipStream_t s);
hipError_t dropout_fwd(const void *x, const int64_t *state, uint32_t site,
                       uint32_t thr, float scale, void *y, uint8_t *mask,
                       long n, hipStream_t s);
hipError_t dropout_bwd(const void *dy, const uint8_t *mask, float scale,
                       void *dx, long n, hipStream_t s);

// ---- optimizer.hip ----
int optim_block_count(const OptDesc *descs, int nt);
hipError_t optim_tick_launch(float *scalars, const float *partials,
                             int nblocks, double beta1, double beta2,
                             double max_grad_norm, hipStream_t s);
hipError_t l2norm_partials_launch(const OptDesc *descs, int nt,
                                  int grad_is_bf16, float *partials,
                                  int block_base, hipStream_t s);
hipError_t adam_step_launch(const OptDesc *descs, int nt, int grad_is_bf16,
                            const float *scalars, double beta1, double beta2,
                            double eps, double wd, int adam_w_mode,
                            hipStream_t s);
hipError_t lamb_step_launch(const OptDesc *descs, int nt, int grad_is_bf16,
                            const float *scalars, float *part_w, float *part_u,
                            int block_base, float *ratio, int tensor_base,
                            double beta1, double beta2, double eps, double wd,
                            int adam_w_mode, hipStream_t s);

} // extern "C"
