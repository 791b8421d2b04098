// The MLM head on the labelled rows only: a fixed-capacity, device-side
// selection of the rows whose label is not ignore_index, the gather of those
// rows out of the trunk output, and the scatter of their gradient back.
//
// Every shape is fixed by (M, capacity, hidden); how many rows are labelled
// lives in the buffers' contents only, so a captured step replays on other
// labels. Nothing here reads on the host, no atomic decides an order, and
// every output element is written by a kernel (no memset nodes, see
// embedding.hip), so two calls agree bit for bit.
//
// Select (mlm_select_k): ONE workgroup of 1024 threads walks the labels in
// tiles of 2048, two consecutive labels per lane. Slots are handed out in
// ascending row order from three nested exclusive prefixes: the lanes below
// in the wave (two ballots and popcounts, no shuffles), the waves below in
// the tile (16 totals through LDS), the tiles before (a register). The next
// tile's labels are loaded ahead of the barrier. The same workgroup then
// pads the unused slots.
//
// Gather / scatter (gather_rows_k, scatter_rows_k): both are "row r of the
// output is row map[r] of the source, or zeros when map[r] is not a row of
// the source", so the backward is written per OUTPUT row and needs neither
// atomics nor a cleared buffer. One wave per output row, 16-byte octets
// strided over the 64 lanes (embedding.hip's ownership); the map entry is
// wave-uniform.
#include "common.h"
#include "launchers.h"

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / WAVE;
static_assert(SEL_THREADS * 2 == MLM_SELECT_TILE, "two labels per lane");

typedef __attribute__((ext_vector_type(2))) int64_t long2v;
typedef __attribute__((ext_vector_type(2))) int int2v;

// labels [i, i + 2) of the M; past the end reads as ignore_index. VEC: the
// pair is one 16-byte load (labels 16-byte aligned, i even).
template <bool VEC>
DEV_INLINE long2v sel_load(const int64_t *__restrict__ labels, long i, long M,
                           int64_t ignore_index) {
  long2v v = {ignore_index, ignore_index};
  if (VEC && i + 1 < M) return *(const long2v *)(labels + i);
  if (i < M) v[0] = labels[i];
  if (i + 1 < M) v[1] = labels[i + 1];
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(SEL_THREADS) void mlm_select_k(
    const int64_t *__restrict__ labels, int64_t ignore_index, int *__restrict__ pos,
    int *__restrict__ slot, int64_t *__restrict__ labels_c,
    int *__restrict__ counts, long M, int P) {
  // double-buffered: a wave that runs ahead writes the other half, and it
  // cannot be two tiles ahead of a wave that has not passed the barrier
  __shared__ int wave_total[2][SEL_WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  const long tiles = (M + MLM_SELECT_TILE - 1) / MLM_SELECT_TILE;
  long base = 0; // labelled rows in the tiles before; the same in every lane
  long2v cur = sel_load<VEC>(labels, 2L * tid, M, ignore_index);
  for (long t = 0; t < tiles; ++t) {
    const long i = t * MLM_SELECT_TILE + 2L * tid;
    long2v nxt = {ignore_index, ignore_index};
    if (t + 1 < tiles)
      nxt = sel_load<VEC>(labels, i + MLM_SELECT_TILE, M, ignore_index);
    // a row past M read ignore_index, so it is never "labelled"
    const bool f0 = cur[0] != ignore_index;
    const bool f1 = cur[1] != ignore_index;
    const uint64_t b0 = __ballot(f0), b1 = __ballot(f1);
    const int in_wave = __popcll(b0 & below) + __popcll(b1 & below);
    int *wt = wave_total[t & 1];
    if (lane == 0) wt[wave] = __popcll(b0) + __popcll(b1);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) {
      const int c = wt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const long k0 = base + before + in_wave;
    const long k1 = k0 + (f0 ? 1 : 0);
    // a labelled row past the capacity is dropped: it keeps slot -1
    const int s0 = f0 && k0 < P ? (int)k0 : -1;
    const int s1 = f1 && k1 < P ? (int)k1 : -1;
    if (s0 >= 0) {
      pos[s0] = (int)i;
      labels_c[s0] = cur[0];
    }
    if (s1 >= 0) {
      pos[s1] = (int)(i + 1);
      labels_c[s1] = cur[1];
    }
    if (i + 1 < M) {
      *(int2v *)(slot + i) = int2v{s0, s1}; // i is even, slot 8-byte aligned
    } else if (i < M) {
      slot[i] = s0;
    }
    base += total;
    cur = nxt;
  }
  const int selected = base < P ? (int)base : P;
  for (int k = selected + tid; k < P; k += SEL_THREADS) {
    pos[k] = -1;
    labels_c[k] = ignore_index;
  }
  if (tid == 0) {
    counts[0] = selected;
    counts[1] = (int)(base - selected);
  }
}

// out row `row` (C8 octets) = src row map[row], zeros unless 0 <= map[row]
// < src_rows. One wave per row; the branch is wave-uniform.
DEV_INLINE void rows_by_map(const ushort8 *__restrict__ src,
                            const int *__restrict__ map,
                            ushort8 *__restrict__ out, long rows, long src_rows,
                            int C8) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int m = __builtin_amdgcn_readfirstlane(map[row]);
  ushort8 *o = out + row * C8;
  if (m >= 0 && m < src_rows) {
    const ushort8 *s = src + (long)m * C8;
#pragma unroll 2
    for (int c = lane; c < C8; c += WAVE) o[c] = s[c];
  } else {
    const ushort8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
    for (int c = lane; c < C8; c += WAVE) o[c] = z;
  }
}

// out[k, :] = x[pos[k], :] for the P slots; an unused slot gets zeros
__global__ __launch_bounds__(256) void gather_rows_k(
    const ushort8 *__restrict__ x, const int *__restrict__ pos,
    ushort8 *__restrict__ out, long P, long M, int C8) {
  rows_by_map(x, pos, out, P, M, C8);
}

// dx[r, :] = dout[slot[r], :] for all M rows; a row without a slot gets zeros
__global__ __launch_bounds__(256) void scatter_rows_k(
    const ushort8 *__restrict__ dout, const int *__restrict__ slot,
    ushort8 *__restrict__ dx, long M, long P, int C8) {
  rows_by_map(dout, slot, dx, M, P, C8);
}

extern "C" hipError_t mlm_select_launch(const int64_t *labels,
                                        int64_t ignore_index, int *pos,
                                        int *slot, int64_t *labels_c,
                                        int *counts, long M, int P,
                                        hipStream_t s) {
  if (M < 1 || M > 0x7fffffffL || P < 1) return hipErrorInvalidValue;
  if (((uintptr_t)slot & 7) || ((uintptr_t)labels & 7))
    return hipErrorInvalidValue;
  if (((uintptr_t)labels & 15) == 0)
    mlm_select_k<true><<<1, SEL_THREADS, 0, s>>>(labels, ignore_index, pos,
                                                 slot, labels_c, counts, M, P);
  else // a view that starts on an odd label
    mlm_select_k<false><<<1, SEL_THREADS, 0, s>>>(labels, ignore_index, pos,
                                                  slot, labels_c, counts, M, P);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

static bool rows_args_ok(long rows, long src_rows, int N) {
  return N >= 8 && N % 8 == 0 && rows >= 1 && src_rows >= 1 &&
         (rows + 3) / 4 <= 0x7fffffffL && src_rows <= 0x7fffffffL;
}

extern "C" hipError_t gather_rows_launch(const void *x, const int *pos,
                                         void *out, long P, long M, int N,
                                         hipStream_t s) {
  if (!rows_args_ok(P, M, N)) return hipErrorInvalidValue;
  gather_rows_k<<<(int)((P + 3) / 4), 256, 0, s>>>(
      (const ushort8 *)x, pos, (ushort8 *)out, P, M, N / 8);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t scatter_rows_launch(const void *dout, const int *slot,
                                          void *dx, long M, long P, int N,
                                          hipStream_t s) {
  if (!rows_args_ok(M, P, N)) return hipErrorInvalidValue;
  scatter_rows_k<<<(int)((M + 3) / 4), 256, 0, s>>>(
      (const ushort8 *)dout, slot, (ushort8 *)dx, M, P, N / 8);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}
