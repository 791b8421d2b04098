// Embedding lookups for bf16 tables and their table gradients.
//
// Forward (embed_ln_fwd_k): one pass over the [T][N] output does what the
// BERT embedding block ran as three gathers, two adds, a LayerNorm and a
// dropout: x = tok[ids] + pos[position] (+ typ[type]) summed in fp32 and
// rounded once, y = dropout(LN(x)). It keeps the LayerNorm family's
// ownership (layernorm.hip): one WAVE per token row, ushort8 octets strided
// over the 64 lanes, wave_sum reductions, no LDS. NORM = false is the plain
// one-table gather.
//
// Backward (embed_bwd_chunk_k + embed_bwd_cross_k): dW[v] = sum of the
// dsum rows whose index is v, from the indices sorted by value (stable, so
// equal indices keep ascending row order). No atomics; every sum has one
// fixed order, so two calls agree bit for bit whatever the schedule.
#include "common.h"
#include "knobs.h"
#include "launchers.h"
#include "philox.h"

// ids / position_ids / type_ids arrive as int32 or int64 (one width per call)
DEV_INLINE long embed_idx(const void *__restrict__ p, long i, bool i64,
                          int rows) {
  long v = i64 ? (long)((const int64_t *)p)[i] : (long)((const int32_t *)p)[i];
  // preconditions are not checked on the device: a bad index reads a wrong
  // row, never outside the table
  return v < 0 ? 0 : (v >= rows ? rows - 1 : v);
}

struct EmbedTables {
  const ushort8 *tok, *pos, *typ; // typ == nullptr: two-table sum
  const void *ids, *pos_ids, *typ_ids; // pos_ids == nullptr: row % S
  int V, P, TY, S;                     // table rows, sequence length
  bool i64;
};

// C8T: compile-time octet count (0 = runtime), as in ln_fwd_k. With C8T the
// rounded sum row stays in registers (2 octets/lane at N <= 1024) between
// the statistics pass and the normalise pass; the runtime form reads it back
// from sum_out, where the same lane has just written it, and keeps its octet
// loops rolled (unrolled they spilled scalar registers).
template <bool NORM, bool DROP, int C8T>
__global__ void embed_ln_fwd_k(EmbedTables e, const float *__restrict__ gamma,
                               const float *__restrict__ beta,
                               const int64_t *__restrict__ state,
                               uint32_t site, uint32_t thr, float scale,
                               ushort8 *__restrict__ sum_out,
                               ushort8 *__restrict__ y,
                               float *__restrict__ mean,
                               float *__restrict__ rstd,
                               uint8_t *__restrict__ mask, long M, int C8rt,
                               float eps) {
  const int C8 = C8T ? C8T : C8rt;
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  int waves = blockDim.x >> 6;
  DropState st = {0, 0, 0, 0};
  if (DROP) st = drop_state(state);
  float inv_n = 1.f / (float)(C8 * 8);
  // one row per wave, no grid-stride loop: loop-carried scalars pushed the
  // dropout forms into scalar-register spills
  const long row = (long)blockIdx.x * waves + wave;
  if (row < M) {
    const ushort8 *tr = e.tok + embed_idx(e.ids, row, e.i64, e.V) * C8;
    ushort8 *yr = y + row * C8;
    if (!NORM) {
      for (int c = lane; c < C8; c += 64) yr[c] = tr[c];
      return;
    }
    long p = e.pos_ids ? embed_idx(e.pos_ids, row, e.i64, e.P)
                       : min((int)(row % e.S), e.P - 1);
    const ushort8 *pr = e.pos + p * C8;
    const ushort8 *qr =
        e.typ ? e.typ + embed_idx(e.typ_ids, row, e.i64, e.TY) * C8 : nullptr;
    ushort8 *sr = sum_out + row * C8;
    float s = 0.f, sq = 0.f;
    ushort8 cs[2];
#pragma unroll C8T ? 2 : 1
    for (int c = lane; c < C8; c += 64) {
      int ci = (c - lane) >> 6;
      float fa[8], fb[8], fc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      bf8_to_f8(tr[c], fa);
      bf8_to_f8(pr[c], fb);
      if (qr) bf8_to_f8(qr[c], fc);
      ushort8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // one rounding for the whole sum; the statistics are taken on the
        // rounded value, the x that ln_bwd recomputes xhat from
        v[j] = f2bf(fa[j] + fb[j] + fc[j]);
        float f = bf2f(v[j]);
        s += f;
        sq += f * f;
      }
      sr[c] = v;
      if (C8T && ci < 2) cs[ci] = v;
    }
    s = wave_sum(s);
    sq = wave_sum(sq);
    float mu = s * inv_n;
    float var = fmaxf(sq * inv_n - mu * mu, 0.f);
    float rs = rsqrtf(var + eps);
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
#pragma unroll C8T ? 2 : 1
    for (int c = lane; c < C8; c += 64) {
      int ci = (c - lane) >> 6;
      float f[8];
      bf8_to_f8(C8T && ci < 2 ? cs[ci] : sr[c], f);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        f[j] = (f[j] - mu) * rs * gamma[c * 8 + j] + beta[c * 8 + j];
      if (DROP) {
        // dropout.hip's element-wise scheme on the [M][N] output, so the
        // mask is the one a separate dropout kernel would draw; the scaled
        // value is rounded once. The launcher guarantees M * C8 < 2^32.
        uint32_t keep = drop_keep8(st, site, thr, (uint32_t)(row * C8 + c));
        ushort8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          r[j] = (keep >> j) & 1u ? f2bf(f[j] * scale) : (uint16_t)0;
        yr[c] = r;
        mask[row * C8 + c] = (uint8_t)keep;
      } else {
        yr[c] = f8_to_bf8(f);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Table gradient. Entry j of the sorted order names table row key(j) and
// dsum row src(j). Default BERT positions need no sort: with [B][S] tokens
// the order is position-major, batch ascending, so key(j) = j / B and
// src(j) = (j % B) * S + j / B.
//
// The sorted range is cut into chunks of EMBED_BWD_CHUNK entries. A wave
// owns one chunk and 64 octets of columns and walks its entries in order
// with fp32 accumulators in registers, so its work is bounded whatever the
// index histogram ([PAD], the two type rows and a position row each collect
// thousands of tokens). A run inside the chunk is rounded and stored to dW.
// A run that crosses a chunk edge leaves its fp32 partial in the slab
// [chunks][2][N]: slot 0 when it continues from the previous chunk ("head"),
// else slot 1 ("tail": it began here and continues into the next chunk).
// embed_bwd_cross_k then sums a crossing run's partials in chunk order from
// the chunk where it began. Only slots that were written are read.
struct EmbedSort {
  const int64_t *key, *perm; // nullptr: the closed form for default positions
  int B, S;
  long n;    // entries = rows of dsum
  long rows; // table rows
};

DEV_INLINE long embed_key(const EmbedSort &e, long j) {
  long k = e.key ? (long)e.key[j] : j / e.B;
  return k < 0 ? 0 : (k >= e.rows ? e.rows - 1 : k); // monotone: runs survive
}

DEV_INLINE long embed_src(const EmbedSort &e, long j) {
  long r = e.perm ? (long)e.perm[j] : (j % e.B) * e.S + j / e.B;
  return r < 0 ? 0 : (r >= e.n ? e.n - 1 : r);
}

constexpr int EMBED_BWD_LOADS = 8; // dsum rows in flight per lane

__global__ __launch_bounds__(64) void embed_bwd_chunk_k(
    EmbedSort e, const ushort8 *__restrict__ dsum, ushort8 *__restrict__ dW,
    float *__restrict__ slab, int C8) {
  constexpr int R = EMBED_BWD_CHUNK;
  const long chunk = blockIdx.x;
  const int c = blockIdx.y * 64 + threadIdx.x;
  if (c >= C8) return;
  const long j0 = chunk * R;
  const long j1 = j0 + R < e.n ? j0 + R : e.n;
  long cur = embed_key(e, j0);
  bool head = j0 > 0 && embed_key(e, j0 - 1) == cur;
  float *sl = slab + chunk * 2 * C8 * 8 + c * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long j = j0; j < j1; j += EMBED_BWD_LOADS) {
    long k[EMBED_BWD_LOADS];
    ushort8 v[EMBED_BWD_LOADS];
#pragma unroll
    for (int u = 0; u < EMBED_BWD_LOADS; ++u) {
      long jj = j + u < j1 ? j + u : j1 - 1;
      k[u] = embed_key(e, jj);
      v[u] = dsum[embed_src(e, jj) * C8 + c];
    }
#pragma unroll
    for (int u = 0; u < EMBED_BWD_LOADS; ++u) {
      if (j + u >= j1) break;
      if (k[u] != cur) { // the run of `cur` ended inside this chunk
        if (head) {
#pragma unroll
          for (int q = 0; q < 8; ++q) sl[q] = acc[q];
        } else {
          dW[cur * C8 + c] = f8_to_bf8(acc);
        }
        head = false;
        cur = k[u];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.f;
      }
      float f[8];
      bf8_to_f8(v[u], f);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += f[q];
    }
  }
  const bool tail = j1 < e.n && embed_key(e, j1) == cur;
  if (head || tail) {
    float *o = head ? sl : sl + C8 * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = acc[q];
  } else {
    dW[cur * C8 + c] = f8_to_bf8(acc);
  }
}

// One wave per (chunk, 64 octets): works only where a crossing run BEGINS
// in this chunk, and then owns that run's row of dW.
__global__ __launch_bounds__(64) void embed_bwd_cross_k(
    EmbedSort e, const float *__restrict__ slab, ushort8 *__restrict__ dW,
    int C8) {
  constexpr int R = EMBED_BWD_CHUNK;
  const long chunk = blockIdx.x;
  const int c = blockIdx.y * 64 + threadIdx.x;
  const long j1 = (chunk + 1) * R;
  if (c >= C8 || j1 >= e.n) return;
  const long key = embed_key(e, j1 - 1);
  if (embed_key(e, j1) != key) return; // nothing crosses this chunk's end
  if (chunk > 0 && embed_key(e, chunk * R - 1) == key) return; // began earlier
  const long chunks = (e.n + R - 1) / R;
  long last = chunk + 1; // the run's head partials: chunks (chunk, last]
  while (last + 1 < chunks && embed_key(e, (last + 1) * R) == key) ++last;
  const long pitch = 2L * C8 * 8;
  const float *sl = slab + c * 8;
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = sl[chunk * pitch + C8 * 8 + q];
#pragma unroll 4
  for (long d = chunk + 1; d <= last; ++d) {
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] += sl[d * pitch + q];
  }
  dW[key * C8 + c] = f8_to_bf8(acc);
}

// Rows no index names stay zero: cleared ahead of the scatter by a kernel,
// not hipMemsetAsync. Under capture that call becomes a memset node, and
// memset nodes have replayed unreliably in captured graphs on MI355X systems;
// new launchers keep to kernel nodes, which the graph tests replay against
// the eager result. The clear runs at the fill kernels' rate (62 MB in 12 us).
__global__ void embed_zero_k(ushort8 *__restrict__ p, long n8) {
  const ushort8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  long stride = (long)gridDim.x * blockDim.x;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < n8;
       o += stride)
    p[o] = z;
}

// 4 waves per block, one row each
static int embed_grid(long M) { return (int)((M + 3) / 4); }

extern "C" hipError_t embed_gather(const void *weight, const void *ids,
                                   int idx64, void *y, long M, int N,
                                   long rows, hipStream_t s) {
  if (N % 8 || N < 8 || M < 1 || M > 0x7fffffffL || rows < 1 ||
      rows > 0x7fffffffL)
    return hipErrorInvalidValue;
  EmbedTables e = {(const ushort8 *)weight, nullptr, nullptr, ids, nullptr,
                   nullptr, (int)rows, 0, 0, 1, idx64 != 0};
  embed_ln_fwd_k<false, false, 0><<<embed_grid(M), 256, 0, s>>>(
      e, nullptr, nullptr, nullptr, 0, 0, 1.f, nullptr, (ushort8 *)y, nullptr,
      nullptr, nullptr, M, N / 8, 0.f);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

template <bool DROP>
static void embed_ln_launch(const EmbedTables &e, const float *gamma,
                            const float *beta, const int64_t *state,
                            uint32_t site, uint32_t thr, float scale,
                            void *sum_out, void *y, float *mean, float *rstd,
                            uint8_t *mask, long M, int N, float eps,
                            hipStream_t s) {
  const int g = embed_grid(M);
  if (ln_spec() && N == 1024)
    embed_ln_fwd_k<true, DROP, 128><<<g, 256, 0, s>>>(
        e, gamma, beta, state, site, thr, scale, (ushort8 *)sum_out,
        (ushort8 *)y, mean, rstd, mask, M, N / 8, eps);
  else if (ln_spec() && N == 768)
    embed_ln_fwd_k<true, DROP, 96><<<g, 256, 0, s>>>(
        e, gamma, beta, state, site, thr, scale, (ushort8 *)sum_out,
        (ushort8 *)y, mean, rstd, mask, M, N / 8, eps);
  else
    embed_ln_fwd_k<true, DROP, 0><<<g, 256, 0, s>>>(
        e, gamma, beta, state, site, thr, scale, (ushort8 *)sum_out,
        (ushort8 *)y, mean, rstd, mask, M, N / 8, eps);
}

extern "C" hipError_t embed_ln_fwd(
    const void *tok, const void *pos, const void *typ, const void *ids,
    const void *pos_ids, const void *typ_ids, int idx64, const float *gamma,
    const float *beta, const int64_t *state, uint32_t site, uint32_t thr,
    float scale, void *sum_out, void *y, float *mean, float *rstd,
    uint8_t *mask, long M, int S, int N, long V, long P, long TY, float eps,
    hipStream_t s) {
  if (N % 8 || N < 8 || N > 2048 || M < 1 || M > 0x7fffffffL || S < 1 ||
      V < 1 || P < 1)
    return hipErrorInvalidValue;
  if ((typ != nullptr) != (typ_ids != nullptr) || (typ && TY < 1))
    return hipErrorInvalidValue;
  if (!pos_ids && S > P) return hipErrorInvalidValue;
  if (V > 0x7fffffffL || P > 0x7fffffffL || TY > 0x7fffffffL)
    return hipErrorInvalidValue;
  EmbedTables e = {(const ushort8 *)tok, (const ushort8 *)pos,
                   (const ushort8 *)typ, ids, pos_ids, typ_ids, (int)V, (int)P,
                   (int)TY, S,
                   idx64 != 0};
  if (mask) {
    if (!state || thr > 65535u || !dropout_numel_ok(M * N))
      return hipErrorInvalidValue;
    embed_ln_launch<true>(e, gamma, beta, state, site, thr, scale, sum_out, y,
                          mean, rstd, mask, M, N, eps, s);
  } else {
    embed_ln_launch<false>(e, gamma, beta, nullptr, 0, 0, 1.f, sum_out, y,
                           mean, rstd, nullptr, M, N, eps, s);
  }
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// dW [rows][N] bf16 from dsum [n][N] bf16. sorted_idx/perm: int64 [n], the
// stable sort of the indices and its permutation; both nullptr selects the
// default-position closed form of a [B][S] batch (n = B * S). slab holds
// [ceil(n / EMBED_BWD_CHUNK)][2][N] fp32.
extern "C" hipError_t embed_bwd(const int64_t *sorted_idx, const int64_t *perm,
                                int B, int S, const void *dsum, void *dW,
                                float *slab, long n, int N, long rows,
                                hipStream_t s) {
  if (N % 8 || N < 8 || n < 1 || rows < 1) return hipErrorInvalidValue;
  if ((sorted_idx == nullptr) != (perm == nullptr)) return hipErrorInvalidValue;
  if (!sorted_idx && (B < 1 || S < 1 || (long)B * S != n || S > rows))
    return hipErrorInvalidValue;
  const int C8 = N / 8;
  const long n8 = rows * C8;
  long zg = (n8 + 255) / 256;
  embed_zero_k<<<(int)(zg > 2048 ? 2048 : zg), 256, 0, s>>>((ushort8 *)dW, n8);
  HIP_KERNEL_CHECK();
  EmbedSort e = {sorted_idx, perm, B < 1 ? 1 : B, S, n, rows};
  const long chunks = (n + EMBED_BWD_CHUNK - 1) / EMBED_BWD_CHUNK;
  if (chunks > 0x7fffffffL) return hipErrorInvalidValue;
  dim3 grid((unsigned)chunks, (unsigned)((C8 + 63) / 64));
  embed_bwd_chunk_k<<<grid, 64, 0, s>>>(e, (const ushort8 *)dsum,
                                        (ushort8 *)dW, slab, C8);
  HIP_KERNEL_CHECK();
  if (chunks > 1) {
    embed_bwd_cross_k<<<grid, 64, 0, s>>>(e, slab, (ushort8 *)dW, C8);
    HIP_KERNEL_CHECK();
  }
  return hipSuccess;
}
