// Element-wise dropout for contiguous bf16 tensors and the step counter of
// the device random-number state (philox.h holds the scheme). The forward
// draws the keep bits and saves them, one byte per octet (bit j = element j),
// 1/16 of the activation's bytes; the backward reads that mask and never
// regenerates it: the offset may have moved on by then (two forwards before
// one backward). The residual-join form fused into LayerNorm is in
// layernorm.hip.
#include "common.h"
#include "launchers.h"
#include "philox.h"

// offset += 1, once per training step, ahead of the step's dropout kernels
// on the same stream (the optim_tick_k pattern: the value lives on the
// device, so a captured step advances it on every replay)
__global__ void rng_tick_k(int64_t *state) { state[1] = state[1] + 1; }

// y = keep ? bf16(x * scale) : 0
__global__ void dropout_fwd_k(const ushort8 *__restrict__ x,
                              const int64_t *__restrict__ state, uint32_t site,
                              uint32_t thr, float scale,
                              ushort8 *__restrict__ y,
                              uint8_t *__restrict__ mask, long n8) {
  const DropState st = drop_state(state);
  long stride = (long)gridDim.x * blockDim.x;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < n8;
       o += stride) {
    ushort8 v = x[o];
    uint32_t keep = drop_keep8(st, site, thr, (uint32_t)o);
    ushort8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      r[j] = (keep >> j) & 1u ? f2bf(bf2f(v[j]) * scale) : (uint16_t)0;
    y[o] = r;
    mask[o] = (uint8_t)keep;
  }
}

// dx = keep ? bf16(dy * scale) : 0
__global__ void dropout_bwd_k(const ushort8 *__restrict__ dy,
                              const uint8_t *__restrict__ mask, float scale,
                              ushort8 *__restrict__ dx, long n8) {
  long stride = (long)gridDim.x * blockDim.x;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < n8;
       o += stride) {
    ushort8 v = dy[o];
    uint32_t keep = mask[o];
    ushort8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      r[j] = (keep >> j) & 1u ? f2bf(bf2f(v[j]) * scale) : (uint16_t)0;
    dx[o] = r;
  }
}

static int dropout_grid(long n8) {
  long g = (n8 + 255) / 256;
  if (g > 2048) g = 2048; // grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

extern "C" hipError_t rng_tick(int64_t *state, hipStream_t s) {
  rng_tick_k<<<1, 1, 0, s>>>(state);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t dropout_fwd(const void *x, const int64_t *state,
                                  uint32_t site, uint32_t thr, float scale,
                                  void *y, uint8_t *mask, long n,
                                  hipStream_t s) {
  if (!dropout_numel_ok(n) || thr > 65535u) return hipErrorInvalidValue;
  dropout_fwd_k<<<dropout_grid(n / 8), 256, 0, s>>>(
      (const ushort8 *)x, state, site, thr, scale, (ushort8 *)y, mask, n / 8);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t dropout_bwd(const void *dy, const uint8_t *mask,
                                  float scale, void *dx, long n,
                                  hipStream_t s) {
  if (!dropout_numel_ok(n)) return hipErrorInvalidValue;
  dropout_bwd_k<<<dropout_grid(n / 8), 256, 0, s>>>(
      (const ushort8 *)dy, mask, scale, (ushort8 *)dx, n / 8);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}
