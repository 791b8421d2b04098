// Fused BatchNorm(+ReLU) for NHWC bf16 activations, fp32 statistics.
// Training fwd = {partial per-channel sum/sumsq (deterministic, no atomics)
// → finalize (mean/invstd/scale/shift) → normalize+ReLU apply}.
// Backward = {partial sum(dy·mask), sum(dy·mask·xhat) → finalize coeffs →
// elementwise dx}. ReLU is folded into both directions (mask from y>0).
// Reference op being replaced: the external image's cuDNN BN+ReLU
// (SURVEY.md §2.3 N7).
#include "common.h"
#include "knobs.h"
#include "launchers.h"
#include <atomic>

// Per-thread fixed channel-group ownership: thread t owns channel block
// cb = t % C8 and row-lane t / C8 — consecutive lanes read consecutive
// 16 B groups (fully coalesced); accumulation stays in registers.
// Requires C8 = C/8 <= 256 (C <= 2048 — every ResNet/BERT channel width).
template <int WHAT> // 0: fwd stats (sum, sumsq); 1: bwd stats (dy*m, dy*m*xhat)
__global__ void bn_partials_k(const ushort8 *__restrict__ x,
                              const ushort8 *__restrict__ dy,
                              const ushort8 *__restrict__ y,
                              const uint8_t *__restrict__ mask,
                              const float *__restrict__ mean,
                              const float *__restrict__ invstd,
                              float *__restrict__ partial, // [grid][2][C]
                              long M, int C8, int relu) {
  int C = C8 * 8;
  int cb = threadIdx.x % C8;
  int row_lane = threadIdx.x / C8;
  int rows_per_block = blockDim.x / C8;
  float a0[8] = {0}, a1[8] = {0};
  float mn[8], is[8];
  if (WHAT == 1 && row_lane < rows_per_block) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mn[j] = mean[cb * 8 + j];
      is[j] = invstd[cb * 8 + j];
    }
  }
  if (row_lane < rows_per_block) {
    long stride = (long)gridDim.x * rows_per_block;
    // two rows per iteration: two independent load chains in flight
    // (single-chain version sat ~80% wave-parked on HBM latency)
    for (long row = (long)blockIdx.x * rows_per_block + row_lane; row < M;
         row += 2 * stride) {
      long r2 = row + stride;
      bool has2 = r2 < M;
      long off = row * C8 + cb, off2 = r2 * C8 + cb;
      float fx[8], fx2[8];
      ushort8 vx = x[off];
      ushort8 vx2 = has2 ? x[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
      bf8_to_f8(vx, fx);
      bf8_to_f8(vx2, fx2);
      if (WHAT == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a0[j] += fx[j] + fx2[j];
          a1[j] += fx[j] * fx[j] + fx2[j] * fx2[j];
        }
      } else {
        ushort8 vdy = dy[off];
        ushort8 vdy2 = has2 ? dy[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
        float fdy[8], fdy2[8];
        bf8_to_f8(vdy, fdy);
        bf8_to_f8(vdy2, fdy2);
        if (relu) {
          if (mask) {
            int m1 = mask[off], m2 = has2 ? mask[off2] : 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              if (!(m1 & (1 << j))) fdy[j] = 0.f;
              if (!(m2 & (1 << j))) fdy2[j] = 0.f;
            }
          } else {
            ushort8 vy = y[off];
            ushort8 vy2 = has2 ? y[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              if (!(bf2f(vy[j]) > 0.f)) fdy[j] = 0.f;
              if (!(bf2f(vy2[j]) > 0.f)) fdy2[j] = 0.f;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a0[j] += fdy[j] + fdy2[j];
          a1[j] += fdy[j] * ((fx[j] - mn[j]) * is[j]) +
                   fdy2[j] * ((fx2[j] - mn[j]) * is[j]);
        }
      }
    }
  }
  // block reduce across row lanes via LDS
  __shared__ float lds[2][256 * 8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    lds[0][threadIdx.x * 8 + j] = a0[j];
    lds[1][threadIdx.x * 8 + j] = a1[j];
  }
  __syncthreads();
  if (row_lane == 0) {
    for (int rl = 1; rl < rows_per_block; ++rl) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a0[j] += lds[0][(rl * C8 + cb) * 8 + j];
        a1[j] += lds[1][(rl * C8 + cb) * 8 + j];
      }
    }
    float *p0 = partial + (long)blockIdx.x * 2 * C + cb * 8;
    float *p1 = p0 + C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p0[j] = a0[j];
      p1[j] = a1[j];
    }
  }
}

// Accumulation steps and the block tail of bn_partials_k above, restated for
// the split-K reduce+stats kernels below: same row assignment, same order,
// same roundings, so a statistic computed there is bit-identical to the one
// bn_partials_k computes from the same (rounded) tensor
// (tests/test_conv_bn_fused_gpu.py asserts equality). bn_partials_k keeps its
// own text so its code, and with it every unfused result, stays as it was.
DEV_INLINE void bn_acc_fwd(float *a0, float *a1, const float *fx,
                           const float *fx2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a0[j] += fx[j] + fx2[j];
    a1[j] += fx[j] * fx[j] + fx2[j] * fx2[j];
  }
}

// fdy/fdy2 are gated in place by the ReLU mask (bitmask if given, else y>0)
DEV_INLINE void bn_acc_bwd(float *a0, float *a1, const float *fx,
                           const float *fx2, float *fdy, float *fdy2,
                           const ushort8 *__restrict__ y,
                           const uint8_t *__restrict__ mask, long off,
                           long off2, bool has2, int relu, const float *mn,
                           const float *is) {
  if (relu) {
    if (mask) {
      int m1 = mask[off], m2 = has2 ? mask[off2] : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!(m1 & (1 << j))) fdy[j] = 0.f;
        if (!(m2 & (1 << j))) fdy2[j] = 0.f;
      }
    } else {
      ushort8 vy = y[off];
      ushort8 vy2 = has2 ? y[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!(bf2f(vy[j]) > 0.f)) fdy[j] = 0.f;
        if (!(bf2f(vy2[j]) > 0.f)) fdy2[j] = 0.f;
      }
    }
  }
  // roundings spelled out as bn_partials_k<1> compiles them (one fma per
  // channel: dy·x̂ + the second row's rounded product), so the contraction
  // does not depend on the surrounding code
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a0[j] += fdy[j] + fdy2[j];
    float xh = __fmul_rn(__fsub_rn(fx[j], mn[j]), is[j]);
    float xh2 = __fmul_rn(__fsub_rn(fx2[j], mn[j]), is[j]);
    a1[j] = __fadd_rn(a1[j], __fmaf_rn(fdy[j], xh, __fmul_rn(fdy2[j], xh2)));
  }
}

// block reduce across row lanes via LDS, row lane 0 stores the slab entry
DEV_INLINE void bn_block_store(float *a0, float *a1,
                               float *__restrict__ partial, int C8, int cb,
                               int row_lane, int rows_per_block) {
  int C = C8 * 8;
  __shared__ float lds[2][256 * 8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    lds[0][threadIdx.x * 8 + j] = a0[j];
    lds[1][threadIdx.x * 8 + j] = a1[j];
  }
  __syncthreads();
  if (row_lane == 0) {
    for (int rl = 1; rl < rows_per_block; ++rl) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a0[j] += lds[0][(rl * C8 + cb) * 8 + j];
        a1[j] += lds[1][(rl * C8 + cb) * 8 + j];
      }
    }
    float *p0 = partial + (long)blockIdx.x * 2 * C + cb * 8;
    float *p1 = p0 + C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p0[j] = a0[j];
      p1[j] = a1[j];
    }
  }
}

// Split-K reduce fused with the BN partials pass, in bn_partials_k's exact
// geometry (a thread owns one 8-channel group, the block strides over rows,
// grid from bn_geom). Per row: sum the `splits` fp32 slabs in
// splitk_reduce_k's order, round ONCE to bf16, write the tensor, and
// accumulate the statistics of the ROUNDED values — so the tensor is
// bit-identical to splitk_reduce's and the slab to bn_partials_k's, while
// the activation is never re-read.
//   WHAT 0 (forward):  out = conv output y;  slab = Σy, Σy²
//   WHAT 1 (backward): out = dgrad output dy; slab = Σ(dy·m), Σ(dy·m·x̂)
//     with x = the consumer BN's saved pre-BN activation.
template <int WHAT, int SPLITS>
__global__ void bn_reduce_stats_k(const float4v *__restrict__ slabs,
                                  int splits_rt, long len4,
                                  ushort8 *__restrict__ out,
                                  const ushort8 *__restrict__ x,
                                  const ushort8 *__restrict__ y,
                                  const uint8_t *__restrict__ mask,
                                  const float *__restrict__ mean,
                                  const float *__restrict__ invstd,
                                  float *__restrict__ partial, // [grid][2][C]
                                  long M, int C8, int relu) {
  int cb = threadIdx.x % C8;
  int row_lane = threadIdx.x / C8;
  int rows_per_block = blockDim.x / C8;
  float a0[8] = {0}, a1[8] = {0};
  float mn[8], is[8];
  if (WHAT == 1 && row_lane < rows_per_block) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mn[j] = mean[cb * 8 + j];
      is[j] = invstd[cb * 8 + j];
    }
  }
  if (row_lane < rows_per_block) {
    long stride = (long)gridDim.x * rows_per_block;
    for (long row = (long)blockIdx.x * rows_per_block + row_lane; row < M;
         row += 2 * stride) {
      long r2 = row + stride;
      bool has2 = r2 < M;
      long off = row * C8 + cb, off2 = r2 * C8 + cb;
      // 8 channels = two float4 slab lanes per row; both rows' chains issue
      // before either is consumed
      float4v s0 = splitk_sum4<SPLITS>(slabs, splits_rt, len4, off * 2);
      float4v s1 = splitk_sum4<SPLITS>(slabs, splits_rt, len4, off * 2 + 1);
      float4v t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
      if (has2) {
        t0 = splitk_sum4<SPLITS>(slabs, splits_rt, len4, off2 * 2);
        t1 = splitk_sum4<SPLITS>(slabs, splits_rt, len4, off2 * 2 + 1);
      }
      ushort8 vo, vo2 = ushort8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vo[j] = f2bf(s0[j]);
        vo[4 + j] = f2bf(s1[j]);
      }
      out[off] = vo;
      if (has2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          vo2[j] = f2bf(t0[j]);
          vo2[4 + j] = f2bf(t1[j]);
        }
        out[off2] = vo2;
      }
      float fo[8], fo2[8];
      bf8_to_f8(vo, fo);
      bf8_to_f8(vo2, fo2);
      if (WHAT == 0) {
        bn_acc_fwd(a0, a1, fo, fo2);
      } else {
        float fx[8], fx2[8];
        ushort8 vx = x[off];
        ushort8 vx2 = has2 ? x[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
        bf8_to_f8(vx, fx);
        bf8_to_f8(vx2, fx2);
        bn_acc_bwd(a0, a1, fx, fx2, fo, fo2, y, mask, off, off2, has2, relu,
                   mn, is);
      }
    }
  }
  bn_block_store(a0, a1, partial, C8, cb, row_lane, rows_per_block);
}

// Residual-join gradient fused with the BN partials pass of the BN layer(s)
// that take the result as their dy, again in bn_partials_k's exact geometry.
// A bottleneck's backward ends by forming dxt, the gradient of its input;
// the previous block's bn3 (and downsample BN) then start by re-reading it
// for Σ(dy·m), Σ(dy·m·x̂). Here dxt is formed with the roundings of the
// streaming kernel it replaces, written, and the statistics of the ROUNDED
// values are accumulated before they leave the registers.
//   JOIN 1: dxt = f2bf((jmask bit ? a : 0) + b)   (add_relu_bwd_add_mask_k)
//   JOIN 0: dxt = f2bf(a + b)                     (add_bf16_k)
//   NSTAT 2: a second consumer (the downsample BN) with its own x/mean/invstd
//     and slab; both consumers gate dy by the same bitmask cmask (the
//     consumer block's join mask).
// The accumulator sets are separate named arrays (compile-time slots): an
// array of sets indexed by a loop variable is what sent BnStatsWriter to
// scratch. __launch_bounds__(256): the launcher's block size; without it the
// NSTAT 2 form is held to 128 VGPRs and spills 84 B/lane, while a grid of at
// most 512 blocks never has more than two waves per SIMD to place anyway.
template <int JOIN, int NSTAT>
__global__ void __launch_bounds__(256)
bn_join_stats_k(const ushort8 *__restrict__ a,
                const uint8_t *__restrict__ jmask,
                const ushort8 *__restrict__ b, ushort8 *__restrict__ dxt,
                const uint8_t *__restrict__ cmask,
                const ushort8 *__restrict__ x, const float *__restrict__ mean,
                const float *__restrict__ invstd,
                float *__restrict__ partial, // [grid][2][C]
                const ushort8 *__restrict__ xd,
                const float *__restrict__ mean_d,
                const float *__restrict__ invstd_d,
                float *__restrict__ partial_d, long M, int C8) {
  int cb = threadIdx.x % C8;
  int row_lane = threadIdx.x / C8;
  int rows_per_block = blockDim.x / C8;
  float a0[8] = {0}, a1[8] = {0}, d0[8] = {0}, d1[8] = {0};
  float mn[8], is[8], mnd[8], isd[8];
  if (row_lane < rows_per_block) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mn[j] = mean[cb * 8 + j];
      is[j] = invstd[cb * 8 + j];
      if (NSTAT == 2) {
        mnd[j] = mean_d[cb * 8 + j];
        isd[j] = invstd_d[cb * 8 + j];
      }
    }
  }
  if (row_lane < rows_per_block) {
    long stride = (long)gridDim.x * rows_per_block;
    for (long row = (long)blockIdx.x * rows_per_block + row_lane; row < M;
         row += 2 * stride) {
      long r2 = row + stride;
      bool has2 = r2 < M;
      long off = row * C8 + cb, off2 = r2 * C8 + cb;
      const ushort8 z = ushort8{0, 0, 0, 0, 0, 0, 0, 0};
      // every load of both rows issues before any is consumed
      ushort8 va = a[off], vb = b[off], vx = x[off];
      ushort8 va2 = has2 ? a[off2] : z, vb2 = has2 ? b[off2] : z;
      ushort8 vx2 = has2 ? x[off2] : z;
      ushort8 vxd = z, vxd2 = z;
      if (NSTAT == 2) {
        vxd = xd[off];
        if (has2) vxd2 = xd[off2];
      }
      int jm = 0, jm2 = 0;
      if (JOIN == 1) {
        jm = jmask[off];
        jm2 = has2 ? jmask[off2] : 0;
      }
      ushort8 vo, vo2 = z;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (JOIN == 1) {
          float g = (jm & (1 << j)) ? bf2f(va[j]) : 0.f;
          float g2 = (jm2 & (1 << j)) ? bf2f(va2[j]) : 0.f;
          vo[j] = f2bf(g + bf2f(vb[j]));
          if (has2) vo2[j] = f2bf(g2 + bf2f(vb2[j]));
        } else {
          vo[j] = f2bf(bf2f(va[j]) + bf2f(vb[j]));
          if (has2) vo2[j] = f2bf(bf2f(va2[j]) + bf2f(vb2[j]));
        }
      }
      dxt[off] = vo;
      if (has2) dxt[off2] = vo2;
      float fo[8], fo2[8], fx[8], fx2[8];
      bf8_to_f8(vo, fo);
      bf8_to_f8(vo2, fo2);
      bf8_to_f8(vx, fx);
      bf8_to_f8(vx2, fx2);
      // gates fo/fo2 in place by cmask; the second consumer takes the gated
      // values (same mask, gating again changes nothing)
      bn_acc_bwd(a0, a1, fx, fx2, fo, fo2, nullptr, cmask, off, off2, has2, 1,
                 mn, is);
      if (NSTAT == 2) {
        float fxd[8], fxd2[8];
        bf8_to_f8(vxd, fxd);
        bf8_to_f8(vxd2, fxd2);
        bn_acc_bwd(d0, d1, fxd, fxd2, fo, fo2, nullptr, cmask, off, off2, has2,
                   1, mnd, isd);
      }
    }
  }
  bn_block_store(a0, a1, partial, C8, cb, row_lane, rows_per_block);
  if (NSTAT == 2) {
    // bn_block_store's LDS array is one static allocation: row lane 0 must
    // finish reading the first reduction before anyone overwrites it
    __syncthreads();
    bn_block_store(d0, d1, partial_d, C8, cb, row_lane, rows_per_block);
  }
}

// finalize: 8 lanes cooperate per channel (grid entries split across lanes,
// shfl-reduced) — the serial-per-channel version was one-wave latency-bound
// at 124 µs/call and 31% of the whole step.
DEV_INLINE void lane8_sums(const float *__restrict__ partial, int grid, int C,
                           int c, int lane8, float &s0, float &s1) {
  s0 = 0.f;
  s1 = 0.f;
  for (int g = lane8; g < grid; g += 32) {
    s0 += partial[(long)g * 2 * C + c];
    s1 += partial[(long)g * 2 * C + C + c];
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    s0 += __shfl_down(s0, off, 32);
    s1 += __shfl_down(s1, off, 32);
  }
}

// fwd: mean/invstd + scale/shift + fused running-stats update (saves ~5 eager
// tensor ops per BN layer per step on the torch side).
__global__ void bn_finalize_fwd_k(const float *__restrict__ partial, int grid,
                                  int C, const float *__restrict__ gamma,
                                  const float *__restrict__ beta, float inv_m,
                                  float eps, float *__restrict__ mean,
                                  float *__restrict__ invstd,
                                  float *__restrict__ scale,
                                  float *__restrict__ shift,
                                  float *__restrict__ running_mean,
                                  float *__restrict__ running_var,
                                  float momentum, float unbias) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  int c = t / 32, lane8 = t % 32;
  if (c >= C) return;
  float s, sq;
  lane8_sums(partial, grid, C, c, lane8, s, sq);
  if (lane8 != 0) return;
  float mu = s * inv_m;
  float var = fmaxf(sq * inv_m - mu * mu, 0.f);
  float is = rsqrtf(var + eps);
  mean[c] = mu;
  invstd[c] = is;
  float sc = gamma[c] * is;
  scale[c] = sc;
  shift[c] = beta[c] - mu * sc;
  if (running_mean) {
    running_mean[c] = running_mean[c] * (1.f - momentum) + mu * momentum;
    running_var[c] = running_var[c] * (1.f - momentum) + var * unbias * momentum;
  }
}

// bwd: dbeta/dgamma + the three per-channel dx coefficients
__global__ void bn_finalize_bwd_k(const float *__restrict__ partial, int grid,
                                  int C, const float *__restrict__ gamma,
                                  const float *__restrict__ invstd, float inv_m,
                                  float *__restrict__ dbeta,
                                  float *__restrict__ dgamma,
                                  float *__restrict__ k1, // gamma*invstd
                                  float *__restrict__ k2, // k1*dbeta/m
                                  float *__restrict__ k3) { // k1*dgamma/m (×xhat in apply)
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  int c = t / 32, lane8 = t % 32;
  if (c >= C) return;
  float s0, s1;
  lane8_sums(partial, grid, C, c, lane8, s0, s1);
  if (lane8 != 0) return;
  dbeta[c] = s0;
  dgamma[c] = s1;
  float g_is = gamma[c] * invstd[c];
  k1[c] = g_is;
  k2[c] = g_is * s0 * inv_m;
  k3[c] = g_is * s1 * inv_m;
}

__global__ void bn_finalize_fwd_bands_k(
    const float *__restrict__ partial, int grid, int C,
    const float *__restrict__ gamma, const float *__restrict__ beta,
    float inv_m, float eps, float *__restrict__ mean,
    float *__restrict__ invstd, float *__restrict__ scale,
    float *__restrict__ shift, float *__restrict__ running_mean,
    float *__restrict__ running_var, float momentum,
    float unbias); // defined below (shared with the conv-epilogue pre path)

// bwd finalize, bands layout: one 256-thread block per channel striding
// the slab rows — the lane8 version gave each channel only 32 lanes and
// just C/8 blocks of parallelism (8 blocks at C=64), and its strided
// cross-XCD slab reads ran ~8 us/call x 104 BN layers x both directions.
__global__ void bn_finalize_bwd_bands_k(
    const float *__restrict__ partial, int grid, int C,
    const float *__restrict__ gamma, const float *__restrict__ invstd,
    float inv_m, float *__restrict__ dbeta, float *__restrict__ dgamma,
    float *__restrict__ k1, float *__restrict__ k2, float *__restrict__ k3) {
  int c = blockIdx.x;
  if (c >= C) return;
  // thread 0's per-channel loads issue before the slab loop instead of after
  // the reduction (same arithmetic; 6.31 -> 6.22 us mean per call)
  float ga = 0.f, iv = 0.f;
  if (threadIdx.x == 0) {
    ga = gamma[c];
    iv = invstd[c];
  }
  float s0 = 0.f, s1 = 0.f;
  for (int g = threadIdx.x; g < grid; g += 256) {
    s0 += partial[(long)g * 2 * C + c];
    s1 += partial[(long)g * 2 * C + C + c];
  }
  __shared__ float red[2][256 / WAVE];
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[0][threadIdx.x / WAVE] = s0;
    red[1][threadIdx.x / WAVE] = s1;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  s0 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  s1 = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  dbeta[c] = s0;
  dgamma[c] = s1;
  float g_is = ga * iv;
  k1[c] = g_is;
  k2[c] = g_is * s0 * inv_m;
  k3[c] = g_is * s1 * inv_m;
}

// apply scale/shift (+optional residual add) (+ReLU): fwd-train, fwd-eval
// and the bottleneck-join fusion (res != nullptr folds the skip connection
// into this pass — one fewer full activation read+write per block).
__global__ void bn_apply_k(const ushort8 *__restrict__ x,
                           const ushort8 *__restrict__ res,
                           const float *__restrict__ scale,
                           const float *__restrict__ shift,
                           ushort8 *__restrict__ y,
                           uint8_t *__restrict__ mask, // y>0 bits, [M][C8]
                           long M, int C8, int relu) {
  int cb = threadIdx.x % C8;
  int row_lane = threadIdx.x / C8;
  int rows_per_block = blockDim.x / C8;
  if (row_lane >= rows_per_block) return;
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = scale[cb * 8 + j];
    sh[j] = shift[cb * 8 + j];
  }
  long stride = (long)gridDim.x * rows_per_block;
  for (long row = (long)blockIdx.x * rows_per_block + row_lane; row < M;
       row += 2 * stride) {
    long r2 = row + stride;
    long off = row * C8 + cb, off2 = r2 * C8 + cb;
    ushort8 v = x[off];
    ushort8 v2 = r2 < M ? x[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
    float f[8], f2[8], g[8] = {0}, g2[8] = {0};
    bf8_to_f8(v, f);
    bf8_to_f8(v2, f2);
    if (res) {
      ushort8 w = res[off];
      ushort8 w2 = r2 < M ? res[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
      bf8_to_f8(w, g);
      bf8_to_f8(w2, g2);
    }
    int m1 = 0, m2 = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = f[j] * sc[j] + sh[j] + g[j];
      f2[j] = f2[j] * sc[j] + sh[j] + g2[j];
      if (relu) {
        // mask records the PRE-clamp sign so backward's dy gating matches
        // the y>0 test it replaces (bf16-rounded y>0 iff f>0 here: rounding
        // keeps sign and relu output is never negative)
        if (f[j] > 0.f) m1 |= 1 << j;
        if (f2[j] > 0.f) m2 |= 1 << j;
        f[j] = fmaxf(f[j], 0.f);
        f2[j] = fmaxf(f2[j], 0.f);
      }
    }
    y[off] = f8_to_bf8(f);
    if (r2 < M) y[off2] = f8_to_bf8(f2);
    if (relu && mask) {
      mask[off] = (uint8_t)m1;
      if (r2 < M) mask[off2] = (uint8_t)m2;
    }
  }
}

// dx = k1*dy·mask - k2 - k3*xhat, xhat = (x-mean)*invstd
__global__ void bn_bwd_apply_k(const ushort8 *__restrict__ dy,
                               const ushort8 *__restrict__ x,
                               const ushort8 *__restrict__ y,
                               const uint8_t *__restrict__ mask,
                               const float *__restrict__ mean,
                               const float *__restrict__ invstd,
                               const float *__restrict__ k1,
                               const float *__restrict__ k2,
                               const float *__restrict__ k3,
                               ushort8 *__restrict__ dx, long M, int C8,
                               int relu) {
  int cb = threadIdx.x % C8;
  int row_lane = threadIdx.x / C8;
  int rows_per_block = blockDim.x / C8;
  if (row_lane >= rows_per_block) return;
  float mn[8], is[8], a[8], b[8], c3[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int c = cb * 8 + j;
    mn[j] = mean[c];
    is[j] = invstd[c];
    a[j] = k1[c];
    b[j] = k2[c];
    c3[j] = k3[c];
  }
  long stride = (long)gridDim.x * rows_per_block;
  for (long row = (long)blockIdx.x * rows_per_block + row_lane; row < M;
       row += 2 * stride) {
    long r2 = row + stride;
    long off = row * C8 + cb, off2 = r2 * C8 + cb;
    ushort8 vdy = dy[off], vx = x[off];
    ushort8 vdy2 = r2 < M ? dy[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
    ushort8 vx2 = r2 < M ? x[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
    float fdy[8], fx[8], fdy2[8], fx2[8];
    bf8_to_f8(vdy, fdy);
    bf8_to_f8(vx, fx);
    bf8_to_f8(vdy2, fdy2);
    bf8_to_f8(vx2, fx2);
    if (relu) {
      if (mask) { // 1-byte relu mask replaces the 16-byte y re-read
        int m1 = mask[off], m2 = r2 < M ? mask[off2] : 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (!(m1 & (1 << j))) fdy[j] = 0.f;
          if (!(m2 & (1 << j))) fdy2[j] = 0.f;
        }
      } else {
        ushort8 vy = y[off];
        ushort8 vy2 = r2 < M ? y[off2] : ushort8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (!(bf2f(vy[j]) > 0.f)) fdy[j] = 0.f;
          if (!(bf2f(vy2[j]) > 0.f)) fdy2[j] = 0.f;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      fdy[j] = a[j] * fdy[j] - b[j] - c3[j] * ((fx[j] - mn[j]) * is[j]);
      fdy2[j] = a[j] * fdy2[j] - b[j] - c3[j] * ((fx2[j] - mn[j]) * is[j]);
    }
    dx[off] = f8_to_bf8(fdy);
    if (r2 < M) dx[off2] = f8_to_bf8(fdy2);
  }
}

// ---------------------------------------------------------------------------
// Software-pipelined forms of the statistics producers above that gate dy by
// a ReLU bitmask (MPIAMD_BN_PIPELINED): bn_partials_k<1> with a mask and
// bn_join_stats_k<1, *>. Geometry, row assignment, the per-thread serial
// chain a += f(row) + f(row + stride) and the block tail are the ones above;
// only the memory schedule differs: the loads of the next BN_PIPE_DEPTH
// pair-iterations are in flight while the current one is consumed. A grid of
// at most 512 blocks puts two waves on a SIMD, so nothing else covers the HBM
// latency between a thread's iterations. The other forms (forward statistics,
// no ReLU, the y > 0 gate, JOIN 0, the split-K reduces, which never run more
// than two pair-iterations) measured no faster pipelined and keep the kernels
// above; profiles/BENCH_HISTORY.md has the figures.
//
// How a prefetch stays inside its tensor: every tensor is read (and dxt
// written) through a buffer descriptor whose extent is exactly the tensor's
// byte size, and a lane whose row is >= M is given the offset BN_OOB, which
// is past every extent the launchers admit (< 2^31 bytes, bn_pipe_ok). The
// hardware range check returns zero for such a lane without a memory access
// (the zero `has2` substitutes above) and drops such a store. So the last
// iterations need no special case: the loads for rows M .. M + depth·step
// come back as zeros, their accumulation is discarded by the `ok` select,
// and nothing outside [base, base + bytes) is ever addressed. An operand a
// form does not have (xd, jmask) gets a zero-extent descriptor.
//
// Why descriptors rather than `row < M ? p[off] : 0`: a conditional load is a
// branch, and after a branch that may skip a load the compiler has to wait
// for all outstanding loads (it counts them statically), which undoes the
// pipeline. With range-checked loads one group of BN_PIPE_DEPTH + 1
// iterations has no branch around a load and the waits are counted. The
// sched_barriers keep the compiler from sinking an iteration's prefetch below
// the arithmetic of the iterations that follow it in the block (it did).
#ifndef MPIAMD_BN_PIPE_DEPTH
// 1 measured better than 2 (tools/bn_bench.py); 3 leaves the NSTAT 2 form one
// wave per SIMD (256 VGPRs and AGPR spills), half of what its grid needs
#define MPIAMD_BN_PIPE_DEPTH 1
#endif
constexpr int BN_PD = MPIAMD_BN_PIPE_DEPTH;
constexpr unsigned BN_OOB = 0x80000000u;
typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;
typedef __amdgpu_buffer_rsrc_t bn_rsrc_t;

DEV_INLINE bn_rsrc_t bn_rsrc(const void *p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, (int)bytes,
                                           0x00020000);
}
DEV_INLINE ushort8 bn_ld16(bn_rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(
      ushort8, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
DEV_INLINE int bn_ld1(bn_rsrc_t r, unsigned byte_off) {
  return (int)__builtin_amdgcn_raw_buffer_load_b8(r, byte_off, 0, 0);
}
DEV_INLINE void bn_st16(bn_rsrc_t r, unsigned byte_off, ushort8 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4v, v), r,
                                         byte_off, 0, 0);
}
// index of the 16 B group (row, cb), or BN_OOB for a row past the end; the
// mask's byte offset as it is, the activations' after bn_off16
DEV_INLINE unsigned bn_off(long row, long M, int C8, int cb) {
  return row < M ? (unsigned)(row * C8 + cb) : BN_OOB;
}
DEV_INLINE unsigned bn_off16(unsigned e) {
  return e == BN_OOB ? BN_OOB : e * 16;
}

// bn_acc_bwd's accumulation step (fdy/fdy2 already gated); `ok` false leaves
// the accumulators as they were
DEV_INLINE void bn_acc_bwd_sel(float *a0, float *a1, const float *fx,
                               const float *fx2, const float *fdy,
                               const float *fdy2, const float *mn,
                               const float *is, bool ok) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float n0 = __fadd_rn(a0[j], __fadd_rn(fdy[j], fdy2[j]));
    float xh = __fmul_rn(__fsub_rn(fx[j], mn[j]), is[j]);
    float xh2 = __fmul_rn(__fsub_rn(fx2[j], mn[j]), is[j]);
    float n1 =
        __fadd_rn(a1[j], __fmaf_rn(fdy[j], xh, __fmul_rn(fdy2[j], xh2)));
    a0[j] = ok ? n0 : a0[j];
    a1[j] = ok ? n1 : a1[j];
  }
}

// ReLU gate of one row by its bitmask
DEV_INLINE void bn_gate(float *fdy, int m) {
#pragma unroll
  for (int j = 0; j < 8; ++j) fdy[j] = (m & (1 << j)) ? fdy[j] : 0.f;
}

struct BnPartialsStage {
  ushort8 x, x2, dy, dy2;
  int m, m2;
};

// bn_partials_k<1> with relu and a bitmask
__global__ void __launch_bounds__(256)
bn_partials_bwd_pipe_k(const ushort8 *__restrict__ x,
                       const ushort8 *__restrict__ dy,
                       const uint8_t *__restrict__ mask,
                       const float *__restrict__ mean,
                       const float *__restrict__ invstd,
                       float *__restrict__ partial, // [grid][2][C]
                       long M, int C8) {
  int cb = threadIdx.x % C8;
  int row_lane = threadIdx.x / C8;
  int rows_per_block = blockDim.x / C8;
  float a0[8] = {0}, a1[8] = {0};
  float mn[8], is[8];
  if (row_lane < rows_per_block) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mn[j] = mean[cb * 8 + j];
      is[j] = invstd[cb * 8 + j];
    }
  }
  if (row_lane < rows_per_block) {
    const long stride = (long)gridDim.x * rows_per_block, step = 2 * stride;
    const long nb = M * C8 * 16;
    const bn_rsrc_t rx = bn_rsrc(x, nb), rdy = bn_rsrc(dy, nb);
    const bn_rsrc_t rm = bn_rsrc(mask, M * C8);
    auto load = [&](BnPartialsStage &b, long r) {
      unsigned e = bn_off(r, M, C8, cb), e2 = bn_off(r + stride, M, C8, cb);
      b.x = bn_ld16(rx, bn_off16(e));
      b.x2 = bn_ld16(rx, bn_off16(e2));
      b.dy = bn_ld16(rdy, bn_off16(e));
      b.dy2 = bn_ld16(rdy, bn_off16(e2));
      b.m = bn_ld1(rm, e);
      b.m2 = bn_ld1(rm, e2);
    };
    BnPartialsStage buf[BN_PD + 1];
    long row = (long)blockIdx.x * rows_per_block + row_lane;
#pragma unroll
    for (int k = 0; k < BN_PD; ++k) load(buf[k], row + k * step);
    while (row < M) {
#pragma unroll
      for (int k = 0; k <= BN_PD; ++k) {
        load(buf[(k + BN_PD) % (BN_PD + 1)], row + BN_PD * step);
        __builtin_amdgcn_sched_barrier(0);
        const BnPartialsStage &b = buf[k];
        float fx[8], fx2[8], fdy[8], fdy2[8];
        bf8_to_f8(b.x, fx);
        bf8_to_f8(b.x2, fx2);
        bf8_to_f8(b.dy, fdy);
        bf8_to_f8(b.dy2, fdy2);
        bn_gate(fdy, b.m);
        bn_gate(fdy2, b.m2);
        bn_acc_bwd_sel(a0, a1, fx, fx2, fdy, fdy2, mn, is, row < M);
        row += step;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  bn_block_store(a0, a1, partial, C8, cb, row_lane, rows_per_block);
}

struct BnJoinStage {
  ushort8 a, a2, b, b2, x, x2, xd, xd2;
  int jm, jm2, cm, cm2;
};

// bn_join_stats_k<1, NSTAT>
template <int NSTAT>
__global__ void __launch_bounds__(256)
bn_join_stats_pipe_k(const ushort8 *__restrict__ a,
                     const uint8_t *__restrict__ jmask,
                     const ushort8 *__restrict__ b, ushort8 *__restrict__ dxt,
                     const uint8_t *__restrict__ cmask,
                     const ushort8 *__restrict__ x,
                     const float *__restrict__ mean,
                     const float *__restrict__ invstd,
                     float *__restrict__ partial, // [grid][2][C]
                     const ushort8 *__restrict__ xd,
                     const float *__restrict__ mean_d,
                     const float *__restrict__ invstd_d,
                     float *__restrict__ partial_d, long M, int C8) {
  int cb = threadIdx.x % C8;
  int row_lane = threadIdx.x / C8;
  int rows_per_block = blockDim.x / C8;
  float a0[8] = {0}, a1[8] = {0}, d0[8] = {0}, d1[8] = {0};
  float mn[8], is[8], mnd[8], isd[8];
  if (row_lane < rows_per_block) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mn[j] = mean[cb * 8 + j];
      is[j] = invstd[cb * 8 + j];
      if (NSTAT == 2) {
        mnd[j] = mean_d[cb * 8 + j];
        isd[j] = invstd_d[cb * 8 + j];
      }
    }
  }
  if (row_lane < rows_per_block) {
    const long stride = (long)gridDim.x * rows_per_block, step = 2 * stride;
    const long nb = M * C8 * 16;
    const bn_rsrc_t ra = bn_rsrc(a, nb), rb = bn_rsrc(b, nb);
    const bn_rsrc_t rx = bn_rsrc(x, nb), ro = bn_rsrc(dxt, nb);
    const bn_rsrc_t rxd = bn_rsrc(xd, NSTAT == 2 ? nb : 0);
    const bn_rsrc_t rjm = bn_rsrc(jmask, M * C8), rcm = bn_rsrc(cmask, M * C8);
    auto load = [&](BnJoinStage &s, long r) {
      unsigned e = bn_off(r, M, C8, cb), e2 = bn_off(r + stride, M, C8, cb);
      unsigned o = bn_off16(e), o2 = bn_off16(e2);
      s.a = bn_ld16(ra, o);
      s.b = bn_ld16(rb, o);
      s.x = bn_ld16(rx, o);
      s.a2 = bn_ld16(ra, o2);
      s.b2 = bn_ld16(rb, o2);
      s.x2 = bn_ld16(rx, o2);
      if (NSTAT == 2) {
        s.xd = bn_ld16(rxd, o);
        s.xd2 = bn_ld16(rxd, o2);
      }
      s.jm = bn_ld1(rjm, e);
      s.jm2 = bn_ld1(rjm, e2);
      s.cm = bn_ld1(rcm, e);
      s.cm2 = bn_ld1(rcm, e2);
    };
    BnJoinStage buf[BN_PD + 1];
    long row = (long)blockIdx.x * rows_per_block + row_lane;
#pragma unroll
    for (int k = 0; k < BN_PD; ++k) load(buf[k], row + k * step);
    while (row < M) {
#pragma unroll
      for (int k = 0; k <= BN_PD; ++k) {
        load(buf[(k + BN_PD) % (BN_PD + 1)], row + BN_PD * step);
        __builtin_amdgcn_sched_barrier(0);
        const BnJoinStage &s = buf[k];
        ushort8 vo, vo2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float g = (s.jm & (1 << j)) ? bf2f(s.a[j]) : 0.f;
          float g2 = (s.jm2 & (1 << j)) ? bf2f(s.a2[j]) : 0.f;
          vo[j] = f2bf(g + bf2f(s.b[j]));
          vo2[j] = f2bf(g2 + bf2f(s.b2[j]));
        }
        // a row >= M has the offset BN_OOB: the store is dropped
        bn_st16(ro, bn_off16(bn_off(row, M, C8, cb)), vo);
        bn_st16(ro, bn_off16(bn_off(row + stride, M, C8, cb)), vo2);
        float fo[8], fo2[8], fx[8], fx2[8];
        bf8_to_f8(vo, fo);
        bf8_to_f8(vo2, fo2);
        bf8_to_f8(s.x, fx);
        bf8_to_f8(s.x2, fx2);
        bn_gate(fo, s.cm);
        bn_gate(fo2, s.cm2);
        bn_acc_bwd_sel(a0, a1, fx, fx2, fo, fo2, mn, is, row < M);
        if (NSTAT == 2) {
          float fxd[8], fxd2[8];
          bf8_to_f8(s.xd, fxd);
          bf8_to_f8(s.xd2, fxd2);
          bn_acc_bwd_sel(d0, d1, fxd, fxd2, fo, fo2, mnd, isd, row < M);
        }
        row += step;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  bn_block_store(a0, a1, partial, C8, cb, row_lane, rows_per_block);
  if (NSTAT == 2) {
    __syncthreads(); // one static LDS array, as in bn_join_stats_k
    bn_block_store(d0, d1, partial_d, C8, cb, row_lane, rows_per_block);
  }
}

// ---------------------------------------------------------------------------
// Line-coalesced finalize (MPIAMD_BN_FINALIZE_COALESCED): a 256-thread block
// owns CH consecutive channels (8 or 16), lane = channel within the slice, so
// a load instruction reads CH·4 contiguous bytes of each slab row it touches
// where the bands kernels read 4 B of 64 different lines. The summation tree
// is the bands kernels', bit for bit:
//   chains   s_t = Σ p[g], g ≡ t (mod 256) ascending, t = 0..255;
//   butterfly over each 64 consecutive t, offsets 32, 16, 8, 4, 2, 1;
//   ((r0 + r1) + r2) + r3.
// Thread (ch, rg), rg = tid / CH, holds the CH chains t = rg + k·RG
// (RG = 256/CH), i.e. wave w = k / (CH/4), lane-in-wave rg + RG·(k % (CH/4)):
// the butterfly levels >= RG pair registers of one thread, the levels < RG
// pair row groups and go through LDS. Addition commutes, so which partner
// holds the result does not matter, only the tree.
// The slab is read through a range-checked descriptor (see above): a (g, c)
// outside [0, grid) x [0, C) reads nothing and is not accumulated.
template <int CH>
DEV_INLINE bool bn_fin_co_sums(const float *__restrict__ partial, int grid,
                               int C, float &r0, float &r1) {
  constexpr int RG = 256 / CH, KK = CH / 4;
  const int ch = threadIdx.x % CH, rg = threadIdx.x / CH;
  const int c = blockIdx.x * CH + ch;
  const bn_rsrc_t rp = bn_rsrc(partial, (long)grid * 2 * C * 4);
  float p0[CH], p1[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) p0[k] = p1[k] = 0.f;
  for (int base = 0; base < grid; base += 256) {
    float v0[CH], v1[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      int g = base + rg + k * RG;
      bool ok = g < grid && c < C;
      unsigned o = ok ? ((unsigned)g * 2 * C + c) * 4 : BN_OOB;
      unsigned o1 = ok ? ((unsigned)g * 2 * C + C + c) * 4 : BN_OOB;
      v0[k] = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rp, o, 0, 0));
      v1[k] = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rp, o1, 0, 0));
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      bool ok = base + rg + k * RG < grid;
      p0[k] = ok ? p0[k] + v0[k] : p0[k];
      p1[k] = ok ? p1[k] + v1[k] : p1[k];
    }
  }
  __shared__ float red[2 * 4 * 256]; // [stat][wave][rg][ch]
  __shared__ float red2[2 * 4 * CH]; // [stat][wave][ch]
#pragma unroll
  for (int w = 0; w < 4; ++w) {
#pragma unroll
    for (int off = KK / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int kk = 0; kk < off; ++kk) {
        p0[w * KK + kk] += p0[w * KK + kk + off];
        p1[w * KK + kk] += p1[w * KK + kk + off];
      }
    }
    red[((0 * 4 + w) * RG + rg) * CH + ch] = p0[w * KK];
    red[((1 * 4 + w) * RG + rg) * CH + ch] = p1[w * KK];
  }
  __syncthreads();
  if (threadIdx.x < 8 * CH) { // one thread per (stat, wave, channel)
    const int q = threadIdx.x / CH;
    float v[RG];
#pragma unroll
    for (int r = 0; r < RG; ++r) v[r] = red[(q * RG + r) * CH + ch];
#pragma unroll
    for (int off = RG / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int r = 0; r < off; ++r) v[r] += v[r + off];
    }
    red2[q * CH + ch] = v[0];
  }
  __syncthreads();
  if (threadIdx.x >= CH || c >= C) return false;
  r0 = red2[0 * CH + ch] + red2[1 * CH + ch] + red2[2 * CH + ch] +
       red2[3 * CH + ch];
  r1 = red2[4 * CH + ch] + red2[5 * CH + ch] + red2[6 * CH + ch] +
       red2[7 * CH + ch];
  return true;
}

// The per-channel epilogues below restate the bands kernels' with the
// roundings spelled as the parent build compiles them (var and shift are one
// fma each, the running statistics two rounded products added).
template <int CH>
__global__ void __launch_bounds__(256) bn_finalize_fwd_co_k(
    const float *__restrict__ partial, int grid, int C,
    const float *__restrict__ gamma, const float *__restrict__ beta,
    float inv_m, float eps, float *__restrict__ mean,
    float *__restrict__ invstd, float *__restrict__ scale,
    float *__restrict__ shift, float *__restrict__ running_mean,
    float *__restrict__ running_var, float momentum, float unbias) {
  const int c = blockIdx.x * CH + threadIdx.x;
  // per-channel loads issue before the slab loop
  float ga = 0.f, be = 0.f, rm = 0.f, rv = 0.f;
  if (threadIdx.x < CH && c < C) {
    ga = gamma[c];
    be = beta[c];
    if (running_mean) {
      rm = running_mean[c];
      rv = running_var[c];
    }
  }
  float s, sq;
  if (!bn_fin_co_sums<CH>(partial, grid, C, s, sq)) return;
  float mu = __fmul_rn(s, inv_m);
  float var = fmaxf(__fmaf_rn(-mu, mu, __fmul_rn(sq, inv_m)), 0.f);
  float is = rsqrtf(__fadd_rn(var, eps));
  mean[c] = mu;
  invstd[c] = is;
  float sc = __fmul_rn(ga, is);
  scale[c] = sc;
  shift[c] = __fmaf_rn(-mu, sc, be);
  if (running_mean) {
    float keep = __fsub_rn(1.f, momentum);
    running_mean[c] =
        __fadd_rn(__fmul_rn(rm, keep), __fmul_rn(mu, momentum));
    running_var[c] = __fadd_rn(
        __fmul_rn(rv, keep), __fmul_rn(__fmul_rn(var, unbias), momentum));
  }
}

template <int CH>
__global__ void __launch_bounds__(256) bn_finalize_bwd_co_k(
    const float *__restrict__ partial, int grid, int C,
    const float *__restrict__ gamma, const float *__restrict__ invstd,
    float inv_m, float *__restrict__ dbeta, float *__restrict__ dgamma,
    float *__restrict__ k1, float *__restrict__ k2, float *__restrict__ k3) {
  const int c = blockIdx.x * CH + threadIdx.x;
  float ga = 0.f, iv = 0.f;
  if (threadIdx.x < CH && c < C) {
    ga = gamma[c];
    iv = invstd[c];
  }
  float s0, s1;
  if (!bn_fin_co_sums<CH>(partial, grid, C, s0, s1)) return;
  dbeta[c] = s0;
  dgamma[c] = s1;
  float g_is = __fmul_rn(ga, iv);
  k1[c] = g_is;
  k2[c] = __fmul_rn(__fmul_rn(g_is, s0), inv_m);
  k3[c] = __fmul_rn(__fmul_rn(g_is, s1), inv_m);
}

// Process-wide switches, set through the extension's set_bn_pipelined() and
// set_bn_finalize_coalesced(); the Python side owns MPIAMD_BN_PIPELINED and
// MPIAMD_BN_FINALIZE_COALESCED and calls these once at load.
static std::atomic<bool> g_bn_pipelined{true};
static std::atomic<bool> g_bn_finalize_co{true};
static std::atomic<int> g_bn_finalize_ch{0}; // 0: bn_fin_ch()'s table

extern "C" int bn_set_pipelined(int on) {
  return g_bn_pipelined.exchange(on != 0) ? 1 : 0;
}
extern "C" int bn_set_finalize_coalesced(int on) {
  return g_bn_finalize_co.exchange(on != 0) ? 1 : 0;
}
// tools/bn_bench.py's lever: force the slice width (8 or 16) or the bands
// kernel (-1); 0 restores the table. Returns the previous value.
extern "C" int bn_set_finalize_ch(int ch) {
  if (ch != 0 && ch != -1 && ch != 8 && ch != 16) return -2;
  return g_bn_finalize_ch.exchange(ch);
}

// The pipelined producers address every tensor with 32-bit byte offsets (16 B
// per channel group at most) and need BN_OOB past every extent. They pay
// where a thread runs more than two pair-iterations (M > 2 steps of
// 2·grid·rows_per_block rows); below that there is nothing left to overlap
// and the longer prologue costs 4-20 % (tools/bn_bench.py).
static bool bn_pipe_ok(long M, int C8, int grid, int rows_per_block) {
  return g_bn_pipelined.load(std::memory_order_relaxed) &&
         M * C8 * 16 < (1L << 31) && M > 4L * grid * rows_per_block;
}

// Slice width per (channel count, slab rows), from tools/bn_bench.py
// (profiles/BENCH_HISTORY.md); 0 keeps the bands kernel for that class: below
// 256 channels C/CH blocks are too few and the bands kernel is as fast or
// faster. A width of 32 (whole 128 B lines) lost to 8 and 16 everywhere, its
// 64 loads per thread serialise, and has no instantiation.
static int bn_fin_ch(int C, int grid) {
  if (!g_bn_finalize_co.load(std::memory_order_relaxed)) return 0;
  if ((long)grid * 2 * C * 4 >= (1L << 31)) return 0;
  int forced = g_bn_finalize_ch.load(std::memory_order_relaxed);
  if (forced) return forced < 0 ? 0 : forced;
  if (C < 256) return 0;
  return C >= 2048 || (C >= 512 && grid > 1024) ? 16 : 8;
}

static void bn_finalize_fwd_dispatch(
    const float *partial, int grid, int C, const float *gamma,
    const float *beta, float inv_m, float eps, float *mean, float *invstd,
    float *scale, float *shift, float *running_mean, float *running_var,
    float momentum, float unbias, hipStream_t s) {
#define BN_FIN_FWD(CH)                                                         \
  bn_finalize_fwd_co_k<CH><<<(C + CH - 1) / CH, 256, 0, s>>>(                  \
      partial, grid, C, gamma, beta, inv_m, eps, mean, invstd, scale, shift,   \
      running_mean, running_var, momentum, unbias)
  switch (bn_fin_ch(C, grid)) {
  case 8: BN_FIN_FWD(8); break;
  case 16: BN_FIN_FWD(16); break;
  default:
    bn_finalize_fwd_bands_k<<<C, 256, 0, s>>>(
        partial, grid, C, gamma, beta, inv_m, eps, mean, invstd, scale, shift,
        running_mean, running_var, momentum, unbias);
  }
#undef BN_FIN_FWD
}

static void bn_finalize_bwd_dispatch(const float *partial, int grid, int C,
                                     const float *gamma, const float *invstd,
                                     float inv_m, float *dbeta, float *dgamma,
                                     float *k1, float *k2, float *k3,
                                     hipStream_t s) {
#define BN_FIN_BWD(CH)                                                         \
  bn_finalize_bwd_co_k<CH><<<(C + CH - 1) / CH, 256, 0, s>>>(                  \
      partial, grid, C, gamma, invstd, inv_m, dbeta, dgamma, k1, k2, k3)
  switch (bn_fin_ch(C, grid)) {
  case 8: BN_FIN_BWD(8); break;
  case 16: BN_FIN_BWD(16); break;
  default:
    bn_finalize_bwd_bands_k<<<C, 256, 0, s>>>(partial, grid, C, gamma, invstd,
                                              inv_m, dbeta, dgamma, k1, k2, k3);
  }
#undef BN_FIN_BWD
}

// partials grid, capped by knobs.h bn_grid_cap()
static void bn_geom(long M, int C8, int &grid, int &rows_per_block) {
  rows_per_block = 256 / C8;
  long g = (M + rows_per_block - 1) / rows_per_block;
  long cap = bn_grid_cap();
  grid = (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

// apply-pass grid, capped by knobs.h bn_apply_grid_cap()
static int bn_apply_grid(long M, int C8) {
  const long cap = bn_apply_grid_cap();
  int rpb = 256 / C8;
  long g = (M + rpb - 1) / rpb;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

extern "C" hipError_t bn_fwd_train_launch(
    const void *x, const void *res, const float *gamma, const float *beta,
    float eps, int relu, void *y, uint8_t *relu_mask, float *mean,
    float *invstd, float *scale, float *shift, float *partial,
    float *running_mean, float *running_var, float momentum, long M, int C,
    hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256) return hipErrorInvalidValue;
  int grid, rpb;
  bn_geom(M, C8, grid, rpb);
  bn_partials_k<0><<<grid, 256, 0, s>>>((const ushort8 *)x, nullptr, nullptr,
                                        nullptr, nullptr, nullptr, partial, M,
                                        C8, 0);
  HIP_KERNEL_CHECK();
  float unbias = M > 1 ? (float)M / (float)(M - 1) : 1.f;
  bn_finalize_fwd_dispatch(partial, grid, C, gamma, beta, 1.f / (float)M, eps,
                           mean, invstd, scale, shift, running_mean,
                           running_var, momentum, unbias, s);
  HIP_KERNEL_CHECK();
  bn_apply_k<<<bn_apply_grid(M, C8), 256, 0, s>>>(
      (const ushort8 *)x, (const ushort8 *)res, scale, shift, (ushort8 *)y,
      relu_mask, M, C8, relu);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// Band-slab finalize: the conv-epilogue slab has ceil(M/64) entries (up to
// ~3.1k at ResNet stage-1 sizes) vs the partials path's ≤512 — the 32-lane
// lane8_sums loop went latency-bound there. 256 lanes per channel: 12
// iterations and a full-chip grid.
__global__ void bn_finalize_fwd_bands_k(
    const float *__restrict__ partial, int grid, int C,
    const float *__restrict__ gamma, const float *__restrict__ beta,
    float inv_m, float eps, float *__restrict__ mean,
    float *__restrict__ invstd, float *__restrict__ scale,
    float *__restrict__ shift, float *__restrict__ running_mean,
    float *__restrict__ running_var, float momentum, float unbias) {
  int c = blockIdx.x; // one block (256 threads) per channel
  if (c >= C) return;
  // thread 0's per-channel loads issue before the slab loop instead of after
  // the reduction (same arithmetic; 6.61 -> 6.29 us mean per call)
  float ga = 0.f, be = 0.f, rm = 0.f, rv = 0.f;
  if (threadIdx.x == 0) {
    ga = gamma[c];
    be = beta[c];
    if (running_mean) {
      rm = running_mean[c];
      rv = running_var[c];
    }
  }
  float s = 0.f, sq = 0.f;
  for (int g = threadIdx.x; g < grid; g += 256) {
    s += partial[(long)g * 2 * C + c];
    sq += partial[(long)g * 2 * C + C + c];
  }
  __shared__ float red[2][256 / WAVE];
  s = wave_sum(s);
  sq = wave_sum(sq);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[0][threadIdx.x / WAVE] = s;
    red[1][threadIdx.x / WAVE] = sq;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  sq = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  float mu = s * inv_m;
  float var = fmaxf(sq * inv_m - mu * mu, 0.f);
  float is = rsqrtf(var + eps);
  mean[c] = mu;
  invstd[c] = is;
  float sc = ga * is;
  scale[c] = sc;
  shift[c] = be - mu * sc;
  if (running_mean) {
    running_mean[c] = rm * (1.f - momentum) + mu * momentum;
    running_var[c] = rv * (1.f - momentum) + var * unbias * momentum;
  }
}

// Variant taking PRE-COMPUTED partials (the conv epilogue's BnStatsWriter
// slab, [pre_grid][2][C]) — skips bn_partials' full activation re-read.
extern "C" hipError_t bn_fwd_train_pre_launch(
    const float *pre_partial, int pre_grid, const void *x, const void *res,
    const float *gamma, const float *beta, float eps, int relu, void *y,
    uint8_t *relu_mask, float *mean, float *invstd, float *scale,
    float *shift, float *running_mean, float *running_var, float momentum,
    long M, int C, hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256) return hipErrorInvalidValue;
  float unbias = M > 1 ? (float)M / (float)(M - 1) : 1.f;
  bn_finalize_fwd_dispatch(pre_partial, pre_grid, C, gamma, beta,
                           1.f / (float)M, eps, mean, invstd, scale, shift,
                           running_mean, running_var, momentum, unbias, s);
  HIP_KERNEL_CHECK();
  bn_apply_k<<<bn_apply_grid(M, C8), 256, 0, s>>>(
      (const ushort8 *)x, (const ushort8 *)res, scale, shift, (ushort8 *)y,
      relu_mask, M, C8, relu);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t bn_fwd_eval_launch(const void *x, const float *scale,
                                         const float *shift, int relu, void *y,
                                         long M, int C, hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256) return hipErrorInvalidValue;
  int grid, rpb;
  bn_geom(M, C8, grid, rpb);
  bn_apply_k<<<bn_apply_grid(M, C8), 256, 0, s>>>(
      (const ushort8 *)x, nullptr, scale, shift, (ushort8 *)y, nullptr, M, C8,
      relu);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t bn_bwd_launch(const void *dy, const void *x,
                                    const void *y, const uint8_t *relu_mask,
                                    const float *gamma, const float *mean,
                                    const float *invstd, int relu, void *dx,
                                    float *dgamma, float *dbeta, float *k1,
                                    float *k2, float *k3, float *partial,
                                    long M, int C, hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256) return hipErrorInvalidValue;
  int grid, rpb;
  bn_geom(M, C8, grid, rpb);
  if (relu && relu_mask && bn_pipe_ok(M, C8, grid, rpb))
    bn_partials_bwd_pipe_k<<<grid, 256, 0, s>>>(
        (const ushort8 *)x, (const ushort8 *)dy, relu_mask, mean, invstd,
        partial, M, C8);
  else
    bn_partials_k<1><<<grid, 256, 0, s>>>((const ushort8 *)x, (const ushort8 *)dy,
                                          (const ushort8 *)y, relu_mask, mean,
                                          invstd, partial, M, C8, relu);
  HIP_KERNEL_CHECK();
  bn_finalize_bwd_dispatch(partial, grid, C, gamma, invstd, 1.f / (float)M,
                           dbeta, dgamma, k1, k2, k3, s);
  HIP_KERNEL_CHECK();
  bn_bwd_apply_k<<<bn_apply_grid(M, C8), 256, 0, s>>>(
      (const ushort8 *)dy, (const ushort8 *)x, (const ushort8 *)y, relu_mask,
      mean, invstd, k1, k2, k3, (ushort8 *)dx, M, C8, relu);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// slab rows ([rows][2][C]) of the reduce+stats kernels = the partials grid
extern "C" int bn_stats_grid(long M, int C) {
  int grid, rpb;
  bn_geom(M, C / 8, grid, rpb);
  return grid;
}

#define BN_RS_DISPATCH(WHAT, ...)                                              \
  do {                                                                         \
    switch (splits) {                                                          \
    case 2: bn_reduce_stats_k<WHAT, 2><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    case 3: bn_reduce_stats_k<WHAT, 3><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    case 4: bn_reduce_stats_k<WHAT, 4><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    case 5: bn_reduce_stats_k<WHAT, 5><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    case 6: bn_reduce_stats_k<WHAT, 6><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    case 8: bn_reduce_stats_k<WHAT, 8><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    case 16: bn_reduce_stats_k<WHAT, 16><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    default: bn_reduce_stats_k<WHAT, 0><<<grid, 256, 0, s>>>(__VA_ARGS__); break; \
    }                                                                          \
  } while (0)

// forward: slabs [splits][M][C] fp32 -> y bf16 + stats slab [grid][2][C]
extern "C" hipError_t bn_reduce_stats_fwd_launch(const float *slabs,
                                                 int splits, void *y,
                                                 float *partial, long M, int C,
                                                 hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256 || C % 8 != 0 || splits < 2)
    return hipErrorInvalidValue;
  int grid, rpb;
  bn_geom(M, C8, grid, rpb);
  long len4 = M * C / 4;
  BN_RS_DISPATCH(0, (const float4v *)slabs, splits, len4, (ushort8 *)y,
                 nullptr, nullptr, nullptr, nullptr, nullptr, partial, M, C8,
                 0);
  return hipGetLastError();
}

// backward: slabs -> dy bf16 + the slab bn_partials_k<1> would produce
extern "C" hipError_t bn_reduce_stats_bwd_launch(
    const float *slabs, int splits, void *dy, const void *x, const void *y,
    const uint8_t *relu_mask, const float *mean, const float *invstd, int relu,
    float *partial, long M, int C, hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256 || C % 8 != 0 || splits < 2)
    return hipErrorInvalidValue;
  int grid, rpb;
  bn_geom(M, C8, grid, rpb);
  long len4 = M * C / 4;
  BN_RS_DISPATCH(1, (const float4v *)slabs, splits, len4, (ushort8 *)dy,
                 (const ushort8 *)x, (const ushort8 *)y, relu_mask, mean,
                 invstd, partial, M, C8, relu);
  return hipGetLastError();
}
#undef BN_RS_DISPATCH

// residual-join gradient + the consumer BN's backward slab(s):
//   jmask != nullptr: dxt = (jmask ? a : 0) + b, else dxt = a + b;
//   xd != nullptr: also the downsample BN's slab into partial_d.
// Slabs are [bn_stats_grid(M, C)][2][C]; cmask is the consumers' ReLU bitmask.
extern "C" hipError_t bn_join_stats_launch(
    const void *a, const uint8_t *jmask, const void *b, void *dxt,
    const uint8_t *cmask, const void *x, const float *mean,
    const float *invstd, float *partial, const void *xd, const float *mean_d,
    const float *invstd_d, float *partial_d, long M, int C, hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256 || C % 8 != 0 || M < 1 || !cmask)
    return hipErrorInvalidValue;
  if (xd && (!mean_d || !invstd_d || !partial_d)) return hipErrorInvalidValue;
  int grid, rpb;
  bn_geom(M, C8, grid, rpb);
  const bool pipe = jmask && bn_pipe_ok(M, C8, grid, rpb); // JOIN 1 only
#define BN_JS_ARGS                                                             \
  (const ushort8 *)a, jmask, (const ushort8 *)b, (ushort8 *)dxt, cmask,        \
      (const ushort8 *)x, mean, invstd, partial, (const ushort8 *)xd, mean_d,  \
      invstd_d, partial_d, M, C8
#define BN_JS_LAUNCH(JOIN, NSTAT)                                              \
  do {                                                                         \
    if (pipe)                                                                  \
      bn_join_stats_pipe_k<NSTAT><<<grid, 256, 0, s>>>(BN_JS_ARGS);            \
    else                                                                       \
      bn_join_stats_k<JOIN, NSTAT><<<grid, 256, 0, s>>>(BN_JS_ARGS);           \
  } while (0)
  if (jmask) {
    if (xd) BN_JS_LAUNCH(1, 2);
    else BN_JS_LAUNCH(1, 1);
  } else {
    if (xd) BN_JS_LAUNCH(0, 2);
    else BN_JS_LAUNCH(0, 1);
  }
#undef BN_JS_LAUNCH
#undef BN_JS_ARGS
  return hipGetLastError();
}

// bn_bwd starting from a PRE-COMPUTED backward slab (the dgrad split-K
// reduce's, [pre_grid][2][C]) — skips bn_partials_k<1>'s dy/x re-read.
extern "C" hipError_t bn_bwd_pre_launch(
    const float *pre_partial, int pre_grid, const void *dy, const void *x,
    const void *y, const uint8_t *relu_mask, const float *gamma,
    const float *mean, const float *invstd, int relu, void *dx, float *dgamma,
    float *dbeta, float *k1, float *k2, float *k3, long M, int C,
    hipStream_t s) {
  int C8 = C / 8;
  if (C8 < 1 || C8 > 256) return hipErrorInvalidValue;
  bn_finalize_bwd_dispatch(pre_partial, pre_grid, C, gamma, invstd,
                           1.f / (float)M, dbeta, dgamma, k1, k2, k3, s);
  HIP_KERNEL_CHECK();
  bn_bwd_apply_k<<<bn_apply_grid(M, C8), 256, 0, s>>>(
      (const ushort8 *)dy, (const ushort8 *)x, (const ushort8 *)y, relu_mask,
      mean, invstd, k1, k2, k3, (ushort8 *)dx, M, C8, relu);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}
