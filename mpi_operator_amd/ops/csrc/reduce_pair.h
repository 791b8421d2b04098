// Bodies of the split-K reduce kernels, as __device__ functions of a block
// index and a grid size, and the kernel that runs two of them in one grid.
//
// splitk_reduce_k (conv.hip) and bn_reduce_stats_k (batchnorm.hip) are thin
// wrappers that pass blockIdx.x and gridDim.x. reduce_pair_k below gives the
// first blocks of one launch to one reduce and the rest to another: after a
// paired conv backward (pipe_mix.h pipe_mix8_pair_k) the dx reduce and the dw
// reduce read different slabs, write different tensors and depend only on
// the GEMM pair, so each workgroup does exactly what a workgroup of the
// separate launch does and the two bodies never communicate.
#pragma once
#include "common.h"

// float4 lanes; SPLITS is a template parameter for the common counts so
// the accumulation loop FULLY UNROLLS — the runtime-splits version issued
// its slab loads as a 2-chain serial loop and sat 73% wave-parked (PMC),
// 4.7x off bandwidth at the BERT dw shapes.
template <bool OUT_BF16, int SPLITS>
DEV_INLINE void splitk_reduce_body(const float4v *__restrict__ partial,
                                   int splits_rt, long len4,
                                   void *__restrict__ out, int bid, int nblk) {
  for (long i = bid * blockDim.x + threadIdx.x; i < len4;
       i += (long)nblk * blockDim.x) {
    // summation order lives in common.h (shared with the BN-stats reduces)
    float4v a = splitk_sum4<SPLITS>(partial, splits_rt, len4, i);
    if (OUT_BF16) {
      uint16_t *o = (uint16_t *)out + i * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = f2bf(a[j]);
    } else {
      ((float4v *)out)[i] = a;
    }
  }
}

// Accumulation steps and the block tail of bn_partials_k (batchnorm.hip),
// restated for the split-K reduce+stats and join+stats kernels: same row
// assignment, same order, same roundings, so a statistic computed there is
// bit-identical to the one bn_partials_k computes from the same (rounded)
// tensor (tests/test_conv_bn_fused_gpu.py asserts equality). bn_partials_k
// keeps its own text so its code, and with it every unfused result, stays as
// it was.
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

// block reduce across row lanes via LDS, row lane 0 stores slab entry `bid`
// (the block's index within its own problem). Every thread of the block must
// call it: it holds a __syncthreads.
DEV_INLINE void bn_block_store(float *a0, float *a1,
                               float *__restrict__ partial, int C8, int cb,
                               int row_lane, int rows_per_block, int bid) {
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
    float *p0 = partial + (long)bid * 2 * C + cb * 8;
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
DEV_INLINE void bn_reduce_stats_body(
    const float4v *__restrict__ slabs, int splits_rt, long len4,
    ushort8 *__restrict__ out, const ushort8 *__restrict__ x,
    const ushort8 *__restrict__ y, const uint8_t *__restrict__ mask,
    const float *__restrict__ mean, const float *__restrict__ invstd,
    float *__restrict__ partial, // [nblk][2][C]
    long M, int C8, int relu, int bid, int nblk) {
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
    long stride = (long)nblk * rows_per_block;
    for (long row = (long)bid * rows_per_block + row_lane; row < M;
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
  bn_block_store(a0, a1, partial, C8, cb, row_lane, rows_per_block, bid);
}

// ---- the dx reduce and the dw reduce of a conv backward pair, one grid ----
// dx side: slabs [splits][M][C] fp32 -> dx bf16; with STATS also the consumer
// BN's backward slab (bn_reduce_stats_body<1>), else splitk_reduce_body.
struct ReduceDxArgs {
  const float4v *slabs;
  long len4;
  void *out;
  const ushort8 *x, *y;
  const uint8_t *mask;
  const float *mean, *invstd;
  float *partial;
  long M;
  int C8, relu;
};
// dw side: slabs [splits][len] fp32 -> dw bf16 (splitk_reduce_body<true>)
struct ReduceDwArgs {
  const float4v *slabs;
  int splits; // read by the runtime-splits form (WS == 0) only
  long len4;
  void *out;
};

// Blocks [0, nb_dw) are the dw reduce's and [nb_dw, nb_dw + nb_dx) the dx
// reduce's; dx_first puts the dx blocks at the front. Each block runs its
// body with its index and grid size within its own problem, so the choice is
// block-uniform (bn_block_store synchronises the block through LDS).
template <bool STATS, int DS, int WS>
__global__ void __launch_bounds__(256)
reduce_pair_k(ReduceDxArgs dx, int nb_dx, ReduceDwArgs dw, int nb_dw,
              int dx_first) {
  int b = blockIdx.x;
  if (dx_first) b = b < nb_dx ? b + nb_dw : b - nb_dx;
  if (b < nb_dw) {
    splitk_reduce_body<true, WS>(dw.slabs, dw.splits, dw.len4, dw.out, b,
                                 nb_dw);
  } else if (STATS) {
    bn_reduce_stats_body<1, DS>(dx.slabs, DS, dx.len4, (ushort8 *)dx.out, dx.x,
                                dx.y, dx.mask, dx.mean, dx.invstd, dx.partial,
                                dx.M, dx.C8, dx.relu, b - nb_dw, nb_dx);
  } else {
    splitk_reduce_body<true, DS>(dx.slabs, DS, dx.len4, dx.out, b - nb_dw,
                                 nb_dx);
  }
}
