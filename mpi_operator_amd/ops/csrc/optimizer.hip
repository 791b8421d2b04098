// Fused multi-tensor AdamW / LAMB with device-side step state.
//
// Same launch structure as sgd_step_k (elementwise.hip): tensor descriptors
// travel in kernarg space, OPT_MAX_T tensors per launch, OPT_EPB elements per
// block, a first_block[] prefix maps a block to its tensor; interior blocks
// are fully unrolled 16 B accesses, tail blocks handle ragged numel.
//
// What differs from SGD: everything that depends on the step number lives in
// a per-group device scalar block, so a captured hipGraph replays a CORRECT
// step every time — a host-computed 1-beta^t would be frozen at capture.
//   scalars[OPT_STEP]  int32 step count (bit pattern in the fp32 tensor)
//   scalars[OPT_LR]    learning rate (host refreshes it outside capture)
//   scalars[OPT_BC1]   1 - beta1^step      scalars[OPT_BC2]  1 - beta2^step
//   scalars[OPT_CLIP]  min(1, max_grad_norm / (||g|| + 1e-6)), 1 if off
// optim_tick_k advances the block once per optimizer step, ahead of the
// update kernels on the same stream.
//
// All reductions (grad norm, LAMB per-tensor norms) go through a persistent
// partials slab with one slot per block, summed in index order: no atomics,
// bit-reproducible run to run.
#include "common.h"
#include "launchers.h"

constexpr int OPT_MAX_T = 40;
constexpr int OPT_BLOCK = 256;
constexpr int OPT_EPB = OPT_BLOCK * 32; // elements per block (8192)
constexpr int OPT_ROUND = OPT_BLOCK * 8; // elements per block per round

enum { OPT_STEP = 0, OPT_LR = 1, OPT_BC1 = 2, OPT_BC2 = 3, OPT_CLIP = 4 };

struct OptArgs {
  OptDesc d[OPT_MAX_T];
  int first_block[OPT_MAX_T + 1]; // prefix of per-tensor block counts
  int nt;
  int block_base;  // this launch's first slot in the partials slab
  int tensor_base; // this launch's first slot in ratio[]
};
static_assert(sizeof(OptArgs) <= 4096, "OptArgs must fit the kernarg segment");

// per-launch hyperparameters + the values read from the scalar block
// (1 - beta is formed in double on the host: in fp32, 1 - 0.999f is off by
// 1.3e-5 relative, which lands in exp_avg_sq and then in every update)
struct OptHp {
  float beta1, beta2, omb1, omb2, eps, wd; // omb = 1 - beta
  int adam_w_mode;
  float lr, bc1, bc2, clip;
  float step_size, sqrt_bc2, decay; // lr/bc1, sqrt(bc2), 1 - lr*wd
  float lr_ratio;                   // LAMB stage 2: lr * ratio[t]
};

DEV_INLINE void opt_read_scalars(const float *__restrict__ scalars, OptHp &hp) {
#pragma clang fp contract(off)
  hp.lr = scalars[OPT_LR];
  hp.bc1 = scalars[OPT_BC1];
  hp.bc2 = scalars[OPT_BC2];
  hp.clip = scalars[OPT_CLIP];
  hp.step_size = hp.lr / hp.bc1;
  hp.sqrt_bc2 = sqrtf(hp.bc2);
  hp.decay = 1.f - hp.lr * hp.wd;
  hp.lr_ratio = 0.f;
}

// ---- per-element updates ----
// Each op names the streams it touches; opt_octet moves only those.
// FP contraction is off in the update algebra: every multiply and add rounds
// as written, so the vector and the per-element paths (and any two compiler
// versions) give the same bits. The kernels are HBM-bound; the few extra
// VALU ops are free.
struct AdamOp {
  static constexpr bool LOAD_G = true, LOAD_W = true, LOAD_MV = true;
  static constexpr bool STORE_MV = true, STORE_W = true;
  // torch.optim.AdamW / Adam algebra (non-amsgrad), in torch's order
  static DEV_INLINE void elem(float g, float &w, float &m, float &v,
                              const OptHp &hp, float *) {
#pragma clang fp contract(off)
    g *= hp.clip;
    if (hp.adam_w_mode) w *= hp.decay;
    else g += hp.wd * w;
    m = hp.beta1 * m + hp.omb1 * g;
    v = hp.beta2 * v + hp.omb2 * g * g;
    float denom = sqrtf(v) / hp.sqrt_bc2 + hp.eps;
    w -= hp.step_size * (m / denom);
  }
};

DEV_INLINE float lamb_update(float w, float m, float v, const OptHp &hp) {
#pragma clang fp contract(off)
  float u = (m / hp.bc1) / (sqrtf(v / hp.bc2) + hp.eps);
  if (hp.adam_w_mode) u += hp.wd * w;
  return u;
}

struct LambStage1Op {
  static constexpr bool LOAD_G = true, LOAD_W = true, LOAD_MV = true;
  static constexpr bool STORE_MV = true, STORE_W = false;
  static DEV_INLINE void elem(float g, float &w, float &m, float &v,
                              const OptHp &hp, float *acc) {
#pragma clang fp contract(off)
    g *= hp.clip;
    if (!hp.adam_w_mode) g += hp.wd * w;
    m = hp.beta1 * m + hp.omb1 * g;
    v = hp.beta2 * v + hp.omb2 * g * g;
    float u = lamb_update(w, m, v, hp);
    acc[0] += w * w;
    acc[1] += u * u;
  }
};

struct LambStage2Op {
  static constexpr bool LOAD_G = false, LOAD_W = true, LOAD_MV = true;
  static constexpr bool STORE_MV = false, STORE_W = true;
  static DEV_INLINE void elem(float, float &w, float &m, float &v,
                              const OptHp &hp, float *) {
#pragma clang fp contract(off)
    w -= hp.lr_ratio * lamb_update(w, m, v, hp);
  }
};

struct L2NormOp {
  static constexpr bool LOAD_G = true, LOAD_W = false, LOAD_MV = false;
  static constexpr bool STORE_MV = false, STORE_W = false;
  static DEV_INLINE void elem(float g, float &, float &, float &,
                              const OptHp &, float *acc) {
#pragma clang fp contract(off)
    acc[0] += g * g;
  }
};

DEV_INLINE void load_f8(const float *p, float *x) {
  float4v a = *(const float4v *)p, b = *(const float4v *)(p + 4);
  x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
  x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
}

DEV_INLINE void store_f8(float *p, const float *x) {
  *(float4v *)p = float4v{x[0], x[1], x[2], x[3]};
  *(float4v *)(p + 4) = float4v{x[4], x[5], x[6], x[7]};
}

// n valid elements at i (n <= 8). VEC: n == 8 and every stream 16 B aligned
// — explicit 16 B loads/stores; otherwise per-element accesses of j < n only.
template <class OP, bool GRAD_BF16, bool VEC>
DEV_INLINE void opt_octet(const OptDesc &D, long i, int n, const OptHp &hp,
                          float *acc) {
  float g[8], w[8], m[8], v[8];
  if (VEC) {
    if (OP::LOAD_G) {
      if (GRAD_BF16) {
        ushort8 u = *(const ushort8 *)((const uint16_t *)D.grad + i);
        bf8_to_f8(u, g);
      } else
        load_f8((const float *)D.grad + i, g);
    }
    if (OP::LOAD_W) load_f8(D.master + i, w);
    if (OP::LOAD_MV) {
      load_f8(D.m + i, m);
      load_f8(D.v + i, v);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) OP::elem(g[j], w[j], m[j], v[j], hp, acc);
    if (OP::STORE_MV) {
      store_f8(D.m + i, m);
      store_f8(D.v + i, v);
    }
    if (OP::STORE_W) {
      store_f8(D.master + i, w);
      if (D.out) *(ushort8 *)(D.out + i) = f8_to_bf8(w);
    }
  } else {
    for (int j = 0; j < n; ++j) {
      float gj = 0.f, wj = 0.f, mj = 0.f, vj = 0.f;
      if (OP::LOAD_G)
        gj = GRAD_BF16 ? bf2f(((const uint16_t *)D.grad)[i + j])
                       : ((const float *)D.grad)[i + j];
      if (OP::LOAD_W) wj = D.master[i + j];
      if (OP::LOAD_MV) {
        mj = D.m[i + j];
        vj = D.v[i + j];
      }
      OP::elem(gj, wj, mj, vj, hp, acc);
      if (OP::STORE_MV) {
        D.m[i + j] = mj;
        D.v[i + j] = vj;
      }
      if (OP::STORE_W) {
        D.master[i + j] = wj;
        if (D.out) D.out[i + j] = f2bf(wj);
      }
    }
  }
}

template <class OP>
DEV_INLINE bool opt_aligned16(const OptDesc &D) {
  uintptr_t a = 0;
  if (OP::LOAD_G) a |= (uintptr_t)D.grad;
  if (OP::LOAD_W || OP::STORE_W) a |= (uintptr_t)D.master | (uintptr_t)D.out;
  if (OP::LOAD_MV || OP::STORE_MV) a |= (uintptr_t)D.m | (uintptr_t)D.v;
  return (a & 15) == 0;
}

// find this block's tensor (nt <= 40: linear scan, wave-uniform)
DEV_INLINE int opt_find_tensor(const OptArgs &args, int bid) {
  int t = 0;
  while (t + 1 <= args.nt - 1 && bid >= args.first_block[t + 1]) ++t;
  return t;
}

// one block's share of tensor t: OPT_EPB elements from `base`
template <class OP, bool GRAD_BF16>
DEV_INLINE void opt_block(const OptDesc &D, long base, const OptHp &hp,
                          float *acc) {
  const bool vec = opt_aligned16<OP>(D);
  if (vec && base + OPT_EPB <= D.numel) {
    // interior block: compile-time trip count, so the rounds fully unroll
    // and the loads are scheduled ahead (see sgd_step_k)
#pragma unroll
    for (int r = 0; r < OPT_EPB / OPT_ROUND; ++r)
      opt_octet<OP, GRAD_BF16, true>(
          D, base + r * (long)OPT_ROUND + threadIdx.x * 8L, 8, hp, acc);
    return;
  }
  const long end = min(base + OPT_EPB, D.numel);
  for (long i = base + threadIdx.x * 8L; i < end; i += OPT_ROUND) {
    int n = end - i < 8 ? (int)(end - i) : 8;
    if (vec && n == 8)
      opt_octet<OP, GRAD_BF16, true>(D, i, 8, hp, acc);
    else
      opt_octet<OP, GRAD_BF16, false>(D, i, n, hp, acc);
  }
}

// block sum of NA per-thread accumulators in a fixed order (lane butterfly,
// then the waves in index order); the result is valid in thread 0
template <int NA>
DEV_INLINE void opt_block_sum(float *acc) {
  __shared__ float red[NA][OPT_BLOCK / WAVE];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    float s = wave_sum(acc[a]);
    if (lane == 0) red[a][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      float s = red[a][0];
      for (int k = 1; k < OPT_BLOCK / WAVE; ++k) s += red[a][k];
      acc[a] = s;
    }
  }
}

// ---------------- step state ----------------
// One block; thread 0 owns the scalar block. With clipping on, all threads
// first fold the nblocks grad-norm partials (strided per-thread sums, then
// a fixed-order tree, in double).
__global__ void optim_tick_k(float *scalars, const float *__restrict__ partials,
                             int nblocks, double beta1, double beta2,
                             double max_grad_norm) {
  __shared__ double red[OPT_BLOCK];
  const bool clip = max_grad_norm > 0.0;
  if (clip) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += OPT_BLOCK) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = OPT_BLOCK / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
  }
  if (threadIdx.x != 0) return;
  int *step_p = reinterpret_cast<int *>(scalars) + OPT_STEP;
  const int step = *step_p + 1;
  *step_p = step;
  // double: fp32 1 - 0.999^t carries ~6e-5 relative error at small t
  scalars[OPT_BC1] = (float)(1.0 - pow(beta1, (double)step));
  scalars[OPT_BC2] = (float)(1.0 - pow(beta2, (double)step));
  float cs = 1.f;
  if (clip) {
    // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6) <= 1
    double coef = max_grad_norm / (sqrt(red[0]) + 1e-6);
    cs = coef < 1.0 ? (float)coef : 1.f;
  }
  scalars[OPT_CLIP] = cs;
}

// ---------------- grad-norm partials ----------------
template <bool GRAD_BF16>
__global__ void __launch_bounds__(OPT_BLOCK)
l2norm_partials_k(OptArgs args, float *__restrict__ partials) {
  const int bid = blockIdx.x;
  const int t = opt_find_tensor(args, bid);
  OptHp hp = {};
  float acc[1] = {0.f};
  opt_block<L2NormOp, GRAD_BF16>(
      args.d[t], (long)(bid - args.first_block[t]) * OPT_EPB, hp, acc);
  opt_block_sum<1>(acc);
  if (threadIdx.x == 0) partials[args.block_base + bid] = acc[0];
}

// ---------------- AdamW / Adam ----------------
template <bool GRAD_BF16>
__global__ void __launch_bounds__(OPT_BLOCK)
adam_step_k(OptArgs args, const float *__restrict__ scalars, OptHp hp) {
  const int bid = blockIdx.x;
  const int t = opt_find_tensor(args, bid);
  opt_read_scalars(scalars, hp);
  opt_block<AdamOp, GRAD_BF16>(
      args.d[t], (long)(bid - args.first_block[t]) * OPT_EPB, hp, nullptr);
}

// ---------------- LAMB ----------------
// stage 1: m, v updated and stored; u formed in registers only; per-block
// sum(w^2), sum(u^2) to the slab
template <bool GRAD_BF16>
__global__ void __launch_bounds__(OPT_BLOCK)
lamb_stage1_k(OptArgs args, const float *__restrict__ scalars,
              float *__restrict__ part_w, float *__restrict__ part_u,
              OptHp hp) {
  const int bid = blockIdx.x;
  const int t = opt_find_tensor(args, bid);
  opt_read_scalars(scalars, hp);
  float acc[2] = {0.f, 0.f};
  opt_block<LambStage1Op, GRAD_BF16>(
      args.d[t], (long)(bid - args.first_block[t]) * OPT_EPB, hp, acc);
  opt_block_sum<2>(acc);
  if (threadIdx.x == 0) {
    part_w[args.block_base + bid] = acc[0];
    part_u[args.block_base + bid] = acc[1];
  }
}

// one wave per tensor: its block partials summed in index order per lane,
// then the fixed lane butterfly
__global__ void __launch_bounds__(WAVE)
lamb_ratio_k(OptArgs args, const float *__restrict__ part_w,
             const float *__restrict__ part_u, float *__restrict__ ratio) {
  const int t = blockIdx.x;
  const int b0 = args.block_base + args.first_block[t];
  const int b1 = args.block_base + args.first_block[t + 1];
  float sw = 0.f, su = 0.f;
  for (int b = b0 + threadIdx.x; b < b1; b += WAVE) {
    sw += part_w[b];
    su += part_u[b];
  }
  sw = wave_sum(sw);
  su = wave_sum(su);
  if (threadIdx.x == 0) {
    float nw = sqrtf(sw), nu = sqrtf(su);
    ratio[args.tensor_base + t] = (nw > 0.f && nu > 0.f) ? nw / nu : 1.f;
  }
}

// stage 2: u recomputed from the just-written m, v and the old w
__global__ void __launch_bounds__(OPT_BLOCK)
lamb_stage2_k(OptArgs args, const float *__restrict__ scalars,
              const float *__restrict__ ratio, OptHp hp) {
  const int bid = blockIdx.x;
  const int t = opt_find_tensor(args, bid);
  opt_read_scalars(scalars, hp);
  hp.lr_ratio = hp.lr * ratio[args.tensor_base + t];
  opt_block<LambStage2Op, false>(
      args.d[t], (long)(bid - args.first_block[t]) * OPT_EPB, hp, nullptr);
}

// ---------------- launchers ----------------
extern "C" int optim_block_count(const OptDesc *descs, int nt) {
  long blocks = 0;
  for (int i = 0; i < nt; ++i) blocks += (descs[i].numel + OPT_EPB - 1) / OPT_EPB;
  return (int)blocks;
}

// Fill the next kernarg chunk starting at tensor `start`; returns its block
// count. block_base/tensor_base continue the slab / ratio[] numbering.
static int opt_fill_chunk(OptArgs &a, const OptDesc *descs, int nt, int start,
                          int block_base, int tensor_base) {
  a.nt = (nt - start < OPT_MAX_T) ? nt - start : OPT_MAX_T;
  int blocks = 0;
  for (int i = 0; i < a.nt; ++i) {
    a.d[i] = descs[start + i];
    a.first_block[i] = blocks;
    blocks += (int)((a.d[i].numel + OPT_EPB - 1) / OPT_EPB);
  }
  a.first_block[a.nt] = blocks;
  a.block_base = block_base;
  a.tensor_base = tensor_base;
  return blocks;
}

// the host-known half of OptHp; the kernels fill the rest from the scalars
static OptHp opt_host_hp(double beta1, double beta2, double eps, double wd,
                         int adam_w_mode) {
  OptHp hp = {};
  hp.beta1 = (float)beta1;
  hp.beta2 = (float)beta2;
  hp.omb1 = (float)(1.0 - beta1);
  hp.omb2 = (float)(1.0 - beta2);
  hp.eps = (float)eps;
  hp.wd = (float)wd;
  hp.adam_w_mode = adam_w_mode;
  return hp;
}

extern "C" hipError_t optim_tick_launch(float *scalars, const float *partials,
                                        int nblocks, double beta1, double beta2,
                                        double max_grad_norm, hipStream_t s) {
  optim_tick_k<<<1, OPT_BLOCK, 0, s>>>(scalars, partials, nblocks, beta1, beta2,
                                       max_grad_norm);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t l2norm_partials_launch(const OptDesc *descs, int nt,
                                             int grad_is_bf16, float *partials,
                                             int block_base, hipStream_t s) {
  for (int start = 0; start < nt; start += OPT_MAX_T) {
    OptArgs a;
    int blocks = opt_fill_chunk(a, descs, nt, start, block_base, 0);
    if (blocks > 0) {
      if (grad_is_bf16)
        l2norm_partials_k<true><<<blocks, OPT_BLOCK, 0, s>>>(a, partials);
      else
        l2norm_partials_k<false><<<blocks, OPT_BLOCK, 0, s>>>(a, partials);
      HIP_KERNEL_CHECK();
    }
    block_base += blocks;
  }
  return hipSuccess;
}

extern "C" hipError_t adam_step_launch(const OptDesc *descs, int nt,
                                       int grad_is_bf16, const float *scalars,
                                       double beta1, double beta2, double eps,
                                       double wd, int adam_w_mode,
                                       hipStream_t s) {
  const OptHp hp = opt_host_hp(beta1, beta2, eps, wd, adam_w_mode);
  for (int start = 0; start < nt; start += OPT_MAX_T) {
    OptArgs a;
    int blocks = opt_fill_chunk(a, descs, nt, start, 0, 0);
    if (blocks == 0) continue;
    if (grad_is_bf16)
      adam_step_k<true><<<blocks, OPT_BLOCK, 0, s>>>(a, scalars, hp);
    else
      adam_step_k<false><<<blocks, OPT_BLOCK, 0, s>>>(a, scalars, hp);
    HIP_KERNEL_CHECK();
  }
  return hipSuccess;
}

// stage 1 -> ratio -> stage 2 for one grad-dtype group. part_w / part_u are
// slabs with a slot for every block from block_base on; ratio has a slot for
// every tensor from tensor_base on.
extern "C" hipError_t lamb_step_launch(const OptDesc *descs, int nt,
                                       int grad_is_bf16, const float *scalars,
                                       float *part_w, float *part_u,
                                       int block_base, float *ratio,
                                       int tensor_base, double beta1,
                                       double beta2, double eps, double wd,
                                       int adam_w_mode, hipStream_t s) {
  const OptHp hp = opt_host_hp(beta1, beta2, eps, wd, adam_w_mode);
  for (int pass = 0; pass < 3; ++pass) {
    int bb = block_base;
    for (int start = 0; start < nt; start += OPT_MAX_T) {
      OptArgs a;
      int blocks = opt_fill_chunk(a, descs, nt, start, bb, tensor_base + start);
      bb += blocks;
      if (pass == 1) {
        lamb_ratio_k<<<a.nt, WAVE, 0, s>>>(a, part_w, part_u, ratio);
        HIP_KERNEL_CHECK();
        continue;
      }
      if (blocks == 0) continue;
      if (pass == 0) {
        if (grad_is_bf16)
          lamb_stage1_k<true><<<blocks, OPT_BLOCK, 0, s>>>(a, scalars, part_w,
                                                           part_u, hp);
        else
          lamb_stage1_k<false><<<blocks, OPT_BLOCK, 0, s>>>(a, scalars, part_w,
                                                            part_u, hp);
      } else {
        lamb_stage2_k<<<blocks, OPT_BLOCK, 0, s>>>(a, scalars, ratio, hp);
      }
      HIP_KERNEL_CHECK();
    }
  }
  return hipSuccess;
}
