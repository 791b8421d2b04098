// Tiled ("flash") multi-head self-attention for BERT (bf16, head_dim 64):
// any sequence length, optional additive key mask, O(S) saved state.
//
//   ctx[b, s, h·64+d] = softmax(Q·Kᵀ·scale + mask[b, :]) · V
//   lse[b, h, s]      = log Σ_j exp(scale·q_s·k_j + mask[b, j])      (fp32)
//
// attention.hip keeps a whole score row in registers and a [4][32][S_MAX]
// P image in LDS (128 KiB at S_MAX=256) and saves probs [B,H,S,S] for the
// backward. Here the keys are walked in 128-wide tiles with an online
// softmax, so LDS is 64 KiB at any S, and the backward recomputes P from
// the per-row log-sum-exp instead of reading saved probs:
//   delta = rowsum(dO∘O)
//   P  = exp(scale·QKᵀ + mask − lse);  dP = dO·Vᵀ;  dS = (dP − delta)∘P·scale
//   dV = Pᵀ·dO;  dK = dSᵀ·Q;  dQ = dS·K
// dK/dV are accumulated per key chunk over q-chunks and dQ per q-chunk over
// key tiles, each in registers by ONE workgroup in a fixed order: no
// floating-point atomics, bit-reproducible.
//
// Row ownership, fragment maps and LDS images are those of attention.hip:
// 256 threads = 4 waves, wave w owns rows w·32..+31 of a 128-row chunk;
// NT operands ride the (row>>2)-XOR swizzled-octet image (b128 reads),
// transposed operands the [4 k][16 col] subtile image (ds_read_b64_tr_b16).
// The transpose read gathers across lanes and needs EXEC all ones, so no
// kernel here returns early or branches per lane around one: rows and
// columns past S are computed on zeros and selected away.
//
// Layouts: qkv / dqkv [B, S, 3, H, 64]; ctx / dctx [B, S, H·64];
// lse / delta [B, H, S] fp32; mask [B, S] fp32 additive (or nullptr).
//
// DROP (template parameter of the three MFMA kernels): dropout on P with the
// attention mask scheme of philox.h, keep drawn in the kernels and never
// stored — the backward regenerates it from (state, site, position):
//   O  = rs·(P∘keep)·V          rs = 1/(1 − p_eff), applied in fp32
//   dV = rs·(P∘keep)ᵀ·dO
//   dS = (rs·keep∘dP − delta)∘P·scale
// m, l and lse are those of the undropped softmax, and delta = rowsum(dO∘O)
// still equals rowsum(dP_eff∘P), so the delta kernel is shared.
//
// VARLEN (second template parameter of the three MFMA kernels): N sequences
// packed back to back in one token-major buffer, no padding and no key mask.
//   qkv / dqkv [T, 3, H, 64]; ctx / dctx [T, H·64]; lse / delta [H, T]
//   (the dense layouts at B = 1, S = T, so the delta kernel serves as is);
//   cu_seqlens int32 [N + 1] in DEVICE memory: sequence n owns rows
//   cu[n] .. cu[n+1] − 1.
// Block (n·H + h, y) reads its base row cu[n] and length L = cu[n+1] − cu[n]
// and is then the dense block (b, h, y) of a [1, L] batch at that base: L
// stands where S stands — bounds, key tiles, q-chunks — so tiles, their
// order and every rounding are the dense kernel's. The grid's y extent is
// sized by the host int max_seqlen; a workgroup whose chunk starts at or
// past L (every block of an empty slot) returns before its first barrier,
// the whole workgroup alike. Only the CONTENTS of cu_seqlens vary between
// launches, so a captured graph replays on another length mix.
// Preconditions, not checked on the device: cu[0] = 0, cu non-decreasing,
// cu[N] <= T, and no L > max_seqlen (rows past max_seqlen would be left
// zero). The base and end rows are clamped into [0, T], so cu_seqlens that
// break them give wrong numbers but no access outside the buffers.
// Rows at or past cu[N] belong to no block: the launchers zero ctx, lse
// and dqkv ahead of the kernels (memset nodes under capture).
// DROP keys the masks per sequence: see philox.h.
#include "common.h"
#include "launchers.h"
#include "philox.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8a;
typedef __attribute__((ext_vector_type(16))) float float16a;
typedef __attribute__((ext_vector_type(2))) unsigned int uint2a;

constexpr int FA_D = 64;    // head dim
constexpr int FA_T = 128;   // q-chunk rows and key-tile width
// running-max floor: finite, so exp(m_old − m_new) is never exp(−inf + inf),
// and above finfo(float).min, so a masked score (≈ finfo.min) minus the
// floor is still hugely negative and its exp is exactly 0
constexpr float FA_FLOOR = -3.4e38f;

// launch arguments of the VARLEN kernels (unused where VARLEN is false)
struct FaVarlen {
  const int *cu;  // [N + 1] device
  int total;      // T: rows of the packed buffers
  int max_seqlen; // the dropout masks' S (philox.h)
};

// where block row bh's sequence lives: first row in the token-major
// buffers, offset of its lse / delta row, and its length
struct FaSeq {
  long tok0, lse0;
  int S;
};

template <bool VARLEN>
DEV_INLINE FaSeq fa_seq(int bh, int H, int S, const FaVarlen &vl) {
  if constexpr (VARLEN) {
    int n = bh / H, h = bh % H;
    int c0 = min(max(vl.cu[n], 0), vl.total);
    int c1 = min(max(vl.cu[n + 1], c0), vl.total);
    return {(long)c0, (long)h * vl.total + c0, c1 - c0};
  } else {
    return {(long)(bh / H) * S, (long)bh * S, S};
  }
}

DEV_INLINE bf16x8a fa_bf8(ushort8 u) {
  union { ushort8 u; bf16x8a b; } v;
  v.u = u;
  return v.b;
}

DEV_INLINE int fa_swz(int q, int row) { return q ^ ((row >> 2) & 7); }

// row of C-layout register r (32x32 MFMA result) within the wave's 32 rows
DEV_INLINE int fa_crow(int r, int lane) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// u16 offset of element (row, col) in a [4 row][16 col] subtile image of a
// 128-row × 128-col tile (8 column blocks per row block)
DEV_INLINE int fa_sub128(int row, int col) {
  return ((row >> 2) * 8 + (col >> 4)) * 64 + (row & 3) * 16 + (col & 15);
}

// stage 128 rows × 64 d starting at row0 as swizzled NT octets; rows >= S
// are ZERO (un-staged LDS can hold Inf/NaN patterns and 0·Inf = NaN would
// leak through the excluded columns' MFMA products)
DEV_INLINE void fa_stage_nt(ushort8 *img, const uint16_t *src, long stride,
                            int row0, int S, int tid) {
  ushort8 z8{0, 0, 0, 0, 0, 0, 0, 0};
  for (int idx = tid; idx < FA_T * 8; idx += 256) {
    int row = idx >> 3, q = idx & 7;
    int g = row0 + row;
    img[row * 8 + fa_swz(q, row)] =
        g < S ? *(const ushort8 *)(src + (long)g * stride + q * 8) : z8;
  }
}

// stage 128 rows × 64 d starting at row0 as [4 k][16 d] subtiles (k = row)
DEV_INLINE void fa_stage_tr(ushort8 *img, const uint16_t *src, long stride,
                            int row0, int S, int tid) {
  ushort8 z8{0, 0, 0, 0, 0, 0, 0, 0};
  for (int idx = tid; idx < FA_T * 8; idx += 256) {
    int st = idx >> 3, kq = st >> 2, cq = st & 3;
    int kl = (idx & 7) >> 1, ch = idx & 1;
    int g = row0 + kq * 4 + kl, d0 = cq * 16 + ch * 8;
    img[idx] = g < S ? *(const ushort8 *)(src + (long)g * stride + d0) : z8;
  }
}

// MFMA operand (8 k deep) from a [4 k][16 col] subtile image with CQ column
// blocks per k block: two transpose reads at consecutive k blocks
template <int CQ>
DEV_INLINE bf16x8a fa_tr_frag(const ushort8 *img, int kq0, int cq, int lane) {
  unsigned ibase = (unsigned)(unsigned long)(
      __attribute__((address_space(3))) const void *)img;
  unsigned a0 = ibase + (unsigned)((kq0 * CQ + cq) * 128 + (lane & 15) * 8);
  uint2a lo, hi;
  if (CQ == 4)
    asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                 "ds_read_b64_tr_b16 %1, %2 offset:512\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(lo), "=&v"(hi) : "v"(a0) : "memory");
  else
    asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                 "ds_read_b64_tr_b16 %1, %2 offset:1024\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(lo), "=&v"(hi) : "v"(a0) : "memory");
  union { unsigned u[4]; bf16x8a v; } vv;
  vv.u[0] = lo.x; vv.u[1] = lo.y; vv.u[2] = hi.x; vv.u[3] = hi.y;
  return vv.v;
}

// A fragments (4 k-steps over d) of the wave's 32 rows straight from global;
// rows >= S read as zero
DEV_INLINE void fa_load_rows(bf16x8a f[4], const uint16_t *src, long stride,
                             int row0, int S, int lane) {
  int r = row0 + (lane & 31);
  bool rok = r < S;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    int q = ks * 2 + (lane >> 5);
    f[ks] = fa_bf8(rok ? *(const ushort8 *)(src + (long)r * stride + q * 8)
                       : ushort8{0, 0, 0, 0, 0, 0, 0, 0});
  }
}

// 32 rows × 32 cols of A·Bᵀ over d: A fragments × NT image rows ni·32..+31
DEV_INLINE float16a fa_nt_frag(const bf16x8a af[4], const ushort8 *img, int ni,
                               int lane) {
  float16a a = {};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    int kr = ni * 32 + (lane & 31);
    int q = ks * 2 + (lane >> 5);
    bf16x8a kf = fa_bf8(img[kr * 8 + fa_swz(q, kr)]);
    a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], kf, a, 0, 0, 0);
  }
  return a;
}

// ------------------------------ forward ------------------------------
// grid (B·H, ceil(S/128)); LDS K 16 KiB + V 16 KiB + P 32 KiB = 64 KiB
// (2 workgroups per CU).
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
template <bool DROP, bool VARLEN = false>
__global__ __launch_bounds__(256, 2) void flash_attn_fwd_k(
    const uint16_t *__restrict__ qkv, // [B, S, 3, H, 64]
    uint16_t *__restrict__ ctx,       // [B, S, H*64]
    float *__restrict__ lse,          // [B, H, S]
    const float *__restrict__ mask_,  // [B, S] additive (or nullptr)
    int B, int S_, int H, float scale, AttnDropArgs da, FaVarlen vl) {
  constexpr int D = FA_D, T = FA_T;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  const FaSeq sq = fa_seq<VARLEN>(bh, H, S_, vl);
  const int S = sq.S;
  // workgroup-uniform, ahead of the first barrier
  if (VARLEN && (int)blockIdx.y * T >= S) return;
  const float *mask = VARLEN ? nullptr : mask_;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  __shared__ __align__(128) ushort8 k_img[T * 8];
  __shared__ __align__(128) ushort8 v_img[T * 8];
  __shared__ __align__(128) uint16_t p_img[4][32][T];

  const long qkv_row = (long)3 * H * D;
  const uint16_t *base = qkv + sq.tok0 * qkv_row;
  const uint16_t *qp = base + h * D;
  const uint16_t *kp = base + (long)1 * H * D + h * D;
  const uint16_t *vp = base + (long)2 * H * D + h * D;

  // A wave whose 32 q-rows are all >= S stays in the loop (zero Q, nothing
  // written): every wave must reach both barriers of every tile.
  int qrow0 = blockIdx.y * T + wave * 32;
  bf16x8a qf[4];
  fa_load_rows(qf, qp, qkv_row, qrow0, S, lane);

  float m_run[16], l_run[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    m_run[r] = FA_FLOOR;
    l_run[r] = 0.f;
  }
  float16a oacc[2] = {};
  AttnDrop dr{};
  if (DROP) dr = attn_drop_init(da, bh, VARLEN ? vl.max_seqlen : S);

  const int nkt = (S + T - 1) / T;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * T;
    // first barrier: no wave is still reading the previous tile's K/V
    // images; second: the new images are complete
    __syncthreads();
    fa_stage_nt(k_img, kp, qkv_row, k0, S, tid);
    fa_stage_tr(v_img, vp, qkv_row, k0, S, tid);
    __syncthreads();

    // scores: compile-time fragment count (runtime-indexed accumulators
    // spill); key columns >= S compute zeros and are excluded below
    float16a acc[4];
    float mk[4];
    bool cok[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      acc[ni] = fa_nt_frag(qf, k_img, ni, lane);
      int col = k0 + ni * 32 + (lane & 31);
      cok[ni] = col < S;
      mk[ni] = (mask && cok[ni]) ? mask[(long)b * S + col] : 0.f;
    }

    // online softmax. Columns >= S are excluded EXACTLY: they enter the
    // max as the floor (which m already is at least) and get p = 0 by
    // selection, never by adding to a score computed from padding.
    // A tile whose keys are all masked has every v ≈ finfo.min < floor:
    // m stays put (alpha = 1) and every p = exp(v − m) = 0, so the tile
    // contributes nothing whether a real key came earlier or comes later.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float mt = FA_FLOOR;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        float v = cok[ni] ? acc[ni][r] * scale + mk[ni] : FA_FLOOR;
        acc[ni][r] = v;
        mt = fmaxf(mt, v);
      }
      // half-wave reduce (the 32 lanes holding this row)
#pragma unroll
      for (int off = 16; off > 0; off >>= 1)
        mt = fmaxf(mt, __shfl_xor(mt, off, 64));
      float m_new = fmaxf(m_run[r], mt);
      float alpha = __expf(m_run[r] - m_new);
      float s = 0.f;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        float e = cok[ni] ? __expf(acc[ni][r] - m_new) : 0.f;
        acc[ni][r] = e;
        s += e;
      }
#pragma unroll
      for (int off = 16; off > 0; off >>= 1)
        s += __shfl_xor(s, off, 64);
      m_run[r] = m_new;
      l_run[r] = l_run[r] * alpha + s;
      oacc[0][r] *= alpha;
      oacc[1][r] *= alpha;
    }

    // park the (unnormalized) P tile in this wave's LDS image; DROP parks
    // e·keep (m and l above are the undropped ones). The keep bits are
    // drawn one column fragment at a time, by every lane alike (columns
    // >= S hold e = 0 whatever they draw), and selected, never branched on.
    if constexpr (DROP) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        uint32_t kb = attn_drop_keep16(dr, (uint32_t)qrow0 >> 4, lane >> 5,
                                       k0 + ni * 32 + (lane & 31));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          uint16_t pv = f2bf(acc[ni][r]);
          p_img[wave][fa_crow(r, lane)][ni * 32 + (lane & 31)] =
              ((kb >> r) & 1u) ? pv : (uint16_t)0;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int prow = fa_crow(r, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          p_img[wave][prow][ni * 32 + (lane & 31)] = f2bf(acc[ni][r]);
      }
    }
    // per-wave private image: a wave-level LDS fence suffices
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // O += P·V
#pragma unroll
    for (int ks = 0; ks < T / 16; ++ks) {
      int r = lane & 31, kk = ks * 16 + (lane >> 5) * 8;
      bf16x8a pf = fa_bf8(*(const ushort8 *)&p_img[wave][r][kk]);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
        int cq = ni * 2 + ((lane >> 4) & 1);
        bf16x8a vf = fa_tr_frag<4>(v_img, kq0, cq, lane);
        oacc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, oacc[ni],
                                                           0, 0, 0);
      }
    }
  }

  // ctx = O / l, lse = m + log(l). A row with no valid key at all has
  // l = 0: write zeros and lse = floor (finite) instead of 0/0.
  long crow = (long)H * D;
  uint16_t *cp = ctx + sq.tok0 * crow + h * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = qrow0 + fa_crow(r, lane);
    if (row >= S) continue;
    float l = l_run[r];
    float inv = l > 0.f ? (DROP ? da.rs / l : 1.f / l) : 0.f;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
      cp[(long)row * crow + ni * 32 + (lane & 31)] = f2bf(oacc[ni][r] * inv);
    if ((lane & 31) == 0)
      lse[sq.lse0 + row] = l > 0.f ? m_run[r] + __logf(l) : m_run[r];
  }
}

extern "C" hipError_t flash_attn_fwd_launch(const void *qkv, void *ctx,
                                            float *lse, const float *mask,
                                            int B, int S, int H, float scale,
                                            hipStream_t strm) {
  if (S < 1) return hipErrorInvalidValue;
  flash_attn_fwd_k<false><<<dim3(B * H, (S + FA_T - 1) / FA_T), 256, 0, strm>>>(
      (const uint16_t *)qkv, (uint16_t *)ctx, lse, mask, B, S, H, scale,
      AttnDropArgs{}, FaVarlen{});
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t flash_attn_drop_fwd_launch(
    const void *qkv, void *ctx, float *lse, const float *mask,
    const int64_t *state, uint32_t site, uint32_t thr, float rs, int B, int S,
    int H, float scale, hipStream_t strm) {
  if (S < 1 || !state) return hipErrorInvalidValue;
  flash_attn_fwd_k<true><<<dim3(B * H, (S + FA_T - 1) / FA_T), 256, 0, strm>>>(
      (const uint16_t *)qkv, (uint16_t *)ctx, lse, mask, B, S, H, scale,
      AttnDropArgs{state, site, thr, rs}, FaVarlen{});
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// Packed forward: zero ctx and lse (the rows past cu[N] stay zero), then one
// block row per (sequence slot, head).
template <bool DROP>
static hipError_t fa_varlen_fwd(const void *qkv, void *ctx, float *lse,
                                const int *cu_seqlens, AttnDropArgs da, int N,
                                int T, int max_seqlen, int H, float scale,
                                hipStream_t strm) {
  if (N < 1 || T < 1 || max_seqlen < 1 || H < 1 || !cu_seqlens)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(ctx, 0, (size_t)T * H * FA_D * 2, strm);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(lse, 0, (size_t)T * H * sizeof(float), strm);
  if (e != hipSuccess) return e;
  dim3 grid(N * H, (max_seqlen + FA_T - 1) / FA_T);
  flash_attn_fwd_k<DROP, true><<<grid, 256, 0, strm>>>(
      (const uint16_t *)qkv, (uint16_t *)ctx, lse, nullptr, N, 0, H, scale, da,
      FaVarlen{cu_seqlens, T, max_seqlen});
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t flash_attn_varlen_fwd_launch(
    const void *qkv, void *ctx, float *lse, const int *cu_seqlens, int N, int T,
    int max_seqlen, int H, float scale, hipStream_t strm) {
  return fa_varlen_fwd<false>(qkv, ctx, lse, cu_seqlens, AttnDropArgs{}, N, T,
                              max_seqlen, H, scale, strm);
}

extern "C" hipError_t flash_attn_varlen_drop_fwd_launch(
    const void *qkv, void *ctx, float *lse, const int *cu_seqlens,
    const int64_t *state, uint32_t site, uint32_t thr, float rs, int N, int T,
    int max_seqlen, int H, float scale, hipStream_t strm) {
  if (!state) return hipErrorInvalidValue;
  return fa_varlen_fwd<true>(qkv, ctx, lse, cu_seqlens,
                             AttnDropArgs{state, site, thr, rs}, N, T,
                             max_seqlen, H, scale, strm);
}

// ------------------------------ backward ------------------------------
// delta[b, h, i] = Σ_d dctx[b, i, h·64+d]·ctx[b, i, h·64+d]: 8 lanes per
// (b, i, h) row, one 16-B load each, 3-step shuffle reduce.
__global__ __launch_bounds__(256) void flash_attn_delta_k(
    const uint16_t *__restrict__ ctx, const uint16_t *__restrict__ dctx,
    float *__restrict__ delta, int B, int S, int H) {
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  long rowid = t >> 3; // (b·S + i)·H + h
  int oct = (int)(t & 7);
  long nrows = (long)B * S * H;
  float acc = 0.f;
  if (rowid < nrows) {
    ushort8 c = *(const ushort8 *)(ctx + rowid * FA_D + oct * 8);
    ushort8 d = *(const ushort8 *)(dctx + rowid * FA_D + oct * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += bf2f(c[i]) * bf2f(d[i]);
  }
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (rowid < nrows && oct == 0) {
    int h = (int)(rowid % H);
    long bi = rowid / H;
    int i = (int)(bi % S);
    long b = bi / S;
    delta[(b * H + h) * S + i] = acc;
  }
}

// P and dS fragment (32 q-rows × 32 keys) recomputed from lse/delta and
// written as bf16 into [4 q][16 key] subtile images. `p16` may be nullptr
// (the dQ kernel needs dS only). Rows/keys >= S get exactly 0.
// DROP: the forward's keep bits are drawn again (band0 = global row of the
// wave's first q-row >> 4, gcol = this lane's global key column): the p16
// image takes p·keep and dS = (dp·keep·rs − delta)·p·scale.
// ROWINF: the caller passes lse_r = +inf for rows >= S instead, so that
// exp(0 − inf) = 0 gives those rows' exact zeros and `rok` is not read; the
// 16 row predicates then need not stay live in SGPR pairs across the call
// (the VARLEN dK/dV kernel spilled SGPRs without it). Valid rows are
// computed exactly as with ROWINF = false.
template <bool DROP, bool ROWINF = false>
DEV_INLINE void fa_pds_frag(const bf16x8a qf[4], const bf16x8a dof[4],
                            const ushort8 *k_nt, const ushort8 *v_nt, int ni,
                            int lane, int sqw, bool cok, float mk,
                            const float lse_r[16], const float delta_r[16],
                            const bool rok[16], float scale, uint16_t *p16,
                            uint16_t *ds16, const AttnDrop &dr, uint32_t band0,
                            uint32_t gcol) {
  float16a s = fa_nt_frag(qf, k_nt, ni, lane);
  float16a dp = fa_nt_frag(dof, v_nt, ni, lane);
  int col = ni * 32 + (lane & 31);
  uint32_t kb = 0;
  if (DROP) kb = attn_drop_keep16(dr, band0, lane >> 5, gcol);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = sqw + fa_crow(r, lane);
    float p = (cok && (ROWINF || rok[r]))
                  ? __expf(s[r] * scale + mk - lse_r[r]) : 0.f;
    float dpe = dp[r], pk = p;
    if (DROP) {
      bool keep = (kb >> r) & 1u;
      dpe = keep ? dp[r] * dr.rs : 0.f;
      pk = keep ? p : 0.f;
    }
    float ds = (dpe - delta_r[r]) * p * scale;
    int off = fa_sub128(row, col);
    if (p16) p16[off] = f2bf(pk);
    ds16[off] = f2bf(ds);
  }
}

// dK, dV: grid (B·H, ceil(S/128)) over key chunks, loop over q-chunks.
// LDS: K, V (NT, staged once) + Q, dO (subtile, per q-chunk) 4×16 KiB
// + P, dS 2×32 KiB = 128 KiB.
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
template <bool DROP, bool VARLEN = false>
__global__ __launch_bounds__(256) void flash_attn_bwd_dkv_k(
    const uint16_t *__restrict__ qkv,   // [B, S, 3, H, 64]
    const uint16_t *__restrict__ dctx,  // [B, S, H*64]
    const float *__restrict__ lse,      // [B, H, S]
    const float *__restrict__ delta,    // [B, H, S]
    const float *__restrict__ mask_,    // [B, S] or nullptr
    uint16_t *__restrict__ dqkv,        // [B, S, 3, H, 64]
    int B, int S_, int H, float scale, AttnDropArgs da, FaVarlen vl) {
  constexpr int D = FA_D, T = FA_T;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  const FaSeq sq = fa_seq<VARLEN>(bh, H, S_, vl);
  const int S = sq.S;
  const int kc0 = blockIdx.y * T;
  // workgroup-uniform, ahead of the first barrier
  if (VARLEN && kc0 >= S) return;
  const float *mask = VARLEN ? nullptr : mask_;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  __shared__ __align__(128) ushort8 k_nt[T * 8];
  __shared__ __align__(128) ushort8 v_nt[T * 8];
  __shared__ __align__(128) ushort8 q_tr[T * 8];
  __shared__ __align__(128) ushort8 do_tr[T * 8];
  __shared__ __align__(128) ushort8 p_tr[T * 16];
  __shared__ __align__(128) ushort8 ds_tr[T * 16];

  const long qrow = (long)3 * H * D, crow = (long)H * D;
  const uint16_t *base = qkv + sq.tok0 * qrow;
  const uint16_t *qp = base + h * D;
  const uint16_t *kp = base + (long)H * D + h * D;
  const uint16_t *vp = base + (long)2 * H * D + h * D;
  const uint16_t *dop = dctx + sq.tok0 * crow + h * D;
  const float *lsep = lse + sq.lse0;
  const float *delp = delta + sq.lse0;

  fa_stage_nt(k_nt, kp, qrow, kc0, S, tid);
  fa_stage_nt(v_nt, vp, qrow, kc0, S, tid);

  // this lane's 4 key columns (one per score fragment) are loop-invariant
  bool cok[4];
  float mk[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    int col = kc0 + ni * 32 + (lane & 31);
    cok[ni] = col < S;
    mk[ni] = (mask && cok[ni]) ? mask[(long)b * S + col] : 0.f;
  }

  const int sqw = wave * 32; // recompute: q-rows; accumulate: key rows
  float16a dk[2] = {}, dv[2] = {};
  AttnDrop dr{};
  if (DROP) dr = attn_drop_init(da, bh, VARLEN ? vl.max_seqlen : S);
  const int nqc = (S + T - 1) / T;
  for (int qc = 0; qc < nqc; ++qc) {
    const int q0 = qc * T;
    // first barrier: the previous chunk's dK/dV reads of all four per-chunk
    // images are done; second: Q/dO (and, first time, K/V) are staged
    __syncthreads();
    fa_stage_tr(q_tr, qp, qrow, q0, S, tid);
    fa_stage_tr(do_tr, dop, crow, q0, S, tid);
    __syncthreads();

    bf16x8a qf[4], dof[4];
    fa_load_rows(qf, qp, qrow, q0 + sqw, S, lane);
    fa_load_rows(dof, dop, crow, q0 + sqw, S, lane);
    float lse_r[16], delta_r[16];
    bool rok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int row = q0 + sqw + fa_crow(r, lane);
      rok[r] = row < S;
      // VARLEN: rows >= S get P = exp(0 − inf) = 0 (fa_pds_frag ROWINF)
      lse_r[r] = rok[r] ? lsep[row] : (VARLEN ? INFINITY : 0.f);
      delta_r[r] = rok[r] ? delp[row] : 0.f;
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      fa_pds_frag<DROP, VARLEN>(
          qf, dof, k_nt, v_nt, ni, lane, sqw, cok[ni], mk[ni], lse_r, delta_r,
          rok, scale, (uint16_t *)p_tr, (uint16_t *)ds_tr, dr,
          (uint32_t)(q0 + sqw) >> 4, kc0 + ni * 32 + (lane & 31));
    __syncthreads();

    // dK += dSᵀ·Q, dV += Pᵀ·dO: rows = this wave's 32 keys, k = the 128 q
    for (int ks = 0; ks < 8; ++ks) {
      int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
      int cqa = (sqw >> 4) + ((lane >> 4) & 1);
      bf16x8a a_ds = fa_tr_frag<8>(ds_tr, kq0, cqa, lane);
      bf16x8a a_p = fa_tr_frag<8>(p_tr, kq0, cqa, lane);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int cq = ni * 2 + ((lane >> 4) & 1);
        bf16x8a b_q = fa_tr_frag<4>(q_tr, kq0, cq, lane);
        bf16x8a b_do = fa_tr_frag<4>(do_tr, kq0, cq, lane);
        dk[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_ds, b_q, dk[ni], 0, 0, 0);
        dv[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_p, b_do, dv[ni], 0, 0, 0);
      }
    }
  }

  uint16_t *dk_out = dqkv + sq.tok0 * qrow + (long)H * D + h * D;
  uint16_t *dv_out = dk_out + (long)H * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = kc0 + sqw + fa_crow(r, lane);
    if (row >= S) continue;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int d = ni * 32 + (lane & 31);
      dk_out[(long)row * qrow + d] = f2bf(dk[ni][r]);
      dv_out[(long)row * qrow + d] = f2bf(DROP ? dv[ni][r] * da.rs : dv[ni][r]);
    }
  }
}

// dQ: grid (B·H, ceil(S/128)) over q-chunks, loop over key tiles.
// LDS: K, V (NT) + K (subtile) 3×16 KiB + dS 32 KiB = 80 KiB. The dS image
// is written and read by the same wave (its own 32 q-rows = 8 private row
// blocks), so it needs a wave-level fence only.
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
template <bool DROP, bool VARLEN = false>
__global__ __launch_bounds__(256) void flash_attn_bwd_dq_k(
    const uint16_t *__restrict__ qkv, const uint16_t *__restrict__ dctx,
    const float *__restrict__ lse, const float *__restrict__ delta,
    const float *__restrict__ mask_, uint16_t *__restrict__ dqkv, int B,
    int S_, int H, float scale, AttnDropArgs da, FaVarlen vl) {
  constexpr int D = FA_D, T = FA_T;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  const FaSeq sq = fa_seq<VARLEN>(bh, H, S_, vl);
  const int S = sq.S;
  const int q0 = blockIdx.y * T;
  // workgroup-uniform, ahead of the first barrier
  if (VARLEN && q0 >= S) return;
  const float *mask = VARLEN ? nullptr : mask_;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  __shared__ __align__(128) ushort8 k_nt[T * 8];
  __shared__ __align__(128) ushort8 v_nt[T * 8];
  __shared__ __align__(128) ushort8 k_tr[T * 8];
  __shared__ __align__(128) ushort8 ds_tr[T * 16];

  const long qrow = (long)3 * H * D, crow = (long)H * D;
  const uint16_t *base = qkv + sq.tok0 * qrow;
  const uint16_t *qp = base + h * D;
  const uint16_t *kp = base + (long)H * D + h * D;
  const uint16_t *vp = base + (long)2 * H * D + h * D;
  const uint16_t *dop = dctx + sq.tok0 * crow + h * D;
  const float *lsep = lse + sq.lse0;
  const float *delp = delta + sq.lse0;

  const int sqw = wave * 32;
  bf16x8a qf[4], dof[4];
  fa_load_rows(qf, qp, qrow, q0 + sqw, S, lane);
  fa_load_rows(dof, dop, crow, q0 + sqw, S, lane);
  float lse_r[16], delta_r[16];
  bool rok[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = q0 + sqw + fa_crow(r, lane);
    rok[r] = row < S;
    lse_r[r] = rok[r] ? lsep[row] : 0.f;
    delta_r[r] = rok[r] ? delp[row] : 0.f;
  }

  float16a dq[2] = {};
  AttnDrop dr{};
  if (DROP) dr = attn_drop_init(da, bh, VARLEN ? vl.max_seqlen : S);
  const int nkt = (S + T - 1) / T;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * T;
    __syncthreads(); // previous tile's K/V readers done
    fa_stage_nt(k_nt, kp, qrow, k0, S, tid);
    fa_stage_nt(v_nt, vp, qrow, k0, S, tid);
    fa_stage_tr(k_tr, kp, qrow, k0, S, tid);
    __syncthreads();

#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = k0 + ni * 32 + (lane & 31);
      bool cok = col < S;
      float mk = (mask && cok) ? mask[(long)b * S + col] : 0.f;
      fa_pds_frag<DROP>(qf, dof, k_nt, v_nt, ni, lane, sqw, cok, mk, lse_r,
                        delta_r, rok, scale, nullptr, (uint16_t *)ds_tr, dr,
                        (uint32_t)(q0 + sqw) >> 4, col);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // dQ += dS·K: A = dS (k-contiguous b128 at subtile-linear addresses)
    for (int ks = 0; ks < 8; ++ks) {
      int sq = sqw + (lane & 31);
      int kk = ks * 16 + (lane >> 5) * 8;
      bf16x8a af = fa_bf8(
          *(const ushort8 *)((const uint16_t *)ds_tr + fa_sub128(sq, kk)));
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
        int cq = ni * 2 + ((lane >> 4) & 1);
        bf16x8a bf = fa_tr_frag<4>(k_tr, kq0, cq, lane);
        dq[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, dq[ni], 0, 0, 0);
      }
    }
  }

  uint16_t *dq_out = dqkv + sq.tok0 * qrow + h * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = q0 + sqw + fa_crow(r, lane);
    if (row >= S) continue;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
      dq_out[(long)row * qrow + ni * 32 + (lane & 31)] = f2bf(dq[ni][r]);
  }
}

extern "C" hipError_t flash_attn_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const float *mask, void *dqkv, int B, int S, int H,
    float scale, hipStream_t strm) {
  if (S < 1) return hipErrorInvalidValue;
  long nthr = (long)B * S * H * 8;
  flash_attn_delta_k<<<cdiv_h(nthr, 256), 256, 0, strm>>>(
      (const uint16_t *)ctx, (const uint16_t *)dctx, delta, B, S, H);
  HIP_KERNEL_CHECK();
  dim3 grid(B * H, (S + FA_T - 1) / FA_T);
  flash_attn_bwd_dkv_k<false><<<grid, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, mask,
      (uint16_t *)dqkv, B, S, H, scale, AttnDropArgs{}, FaVarlen{});
  HIP_KERNEL_CHECK();
  flash_attn_bwd_dq_k<false><<<grid, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, mask,
      (uint16_t *)dqkv, B, S, H, scale, AttnDropArgs{}, FaVarlen{});
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// state, site, thr, rs: those of the forward; the masks are drawn again
extern "C" hipError_t flash_attn_drop_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const float *mask, const int64_t *state, uint32_t site,
    uint32_t thr, float rs, void *dqkv, int B, int S, int H, float scale,
    hipStream_t strm) {
  if (S < 1 || !state) return hipErrorInvalidValue;
  long nthr = (long)B * S * H * 8;
  flash_attn_delta_k<<<cdiv_h(nthr, 256), 256, 0, strm>>>(
      (const uint16_t *)ctx, (const uint16_t *)dctx, delta, B, S, H);
  HIP_KERNEL_CHECK();
  dim3 grid(B * H, (S + FA_T - 1) / FA_T);
  AttnDropArgs da{state, site, thr, rs};
  flash_attn_bwd_dkv_k<true><<<grid, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, mask,
      (uint16_t *)dqkv, B, S, H, scale, da, FaVarlen{});
  HIP_KERNEL_CHECK();
  flash_attn_bwd_dq_k<true><<<grid, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, mask,
      (uint16_t *)dqkv, B, S, H, scale, da, FaVarlen{});
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// Packed backward: delta over all T rows (the dense kernel at B = 1, S = T;
// ctx is zero past cu[N], so delta is too), dqkv zeroed for the rows past
// cu[N], then dK/dV and dQ with one block row per (sequence slot, head).
template <bool DROP>
static hipError_t fa_varlen_bwd(const void *qkv, const void *ctx,
                                const void *dctx, const float *lse,
                                float *delta, const int *cu_seqlens,
                                AttnDropArgs da, void *dqkv, int N, int T,
                                int max_seqlen, int H, float scale,
                                hipStream_t strm) {
  if (N < 1 || T < 1 || max_seqlen < 1 || H < 1 || !cu_seqlens)
    return hipErrorInvalidValue;
  long nthr = (long)T * H * 8;
  flash_attn_delta_k<<<cdiv_h(nthr, 256), 256, 0, strm>>>(
      (const uint16_t *)ctx, (const uint16_t *)dctx, delta, 1, T, H);
  HIP_KERNEL_CHECK();
  hipError_t e = hipMemsetAsync(dqkv, 0, (size_t)T * 3 * H * FA_D * 2, strm);
  if (e != hipSuccess) return e;
  dim3 grid(N * H, (max_seqlen + FA_T - 1) / FA_T);
  FaVarlen vl{cu_seqlens, T, max_seqlen};
  flash_attn_bwd_dkv_k<DROP, true><<<grid, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, nullptr,
      (uint16_t *)dqkv, N, 0, H, scale, da, vl);
  HIP_KERNEL_CHECK();
  flash_attn_bwd_dq_k<DROP, true><<<grid, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, nullptr,
      (uint16_t *)dqkv, N, 0, H, scale, da, vl);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t flash_attn_varlen_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const int *cu_seqlens, void *dqkv, int N, int T,
    int max_seqlen, int H, float scale, hipStream_t strm) {
  return fa_varlen_bwd<false>(qkv, ctx, dctx, lse, delta, cu_seqlens,
                              AttnDropArgs{}, dqkv, N, T, max_seqlen, H, scale,
                              strm);
}

// state, site, thr, rs: those of the forward; the masks are drawn again
extern "C" hipError_t flash_attn_varlen_drop_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const int *cu_seqlens, const int64_t *state, uint32_t site,
    uint32_t thr, float rs, void *dqkv, int N, int T, int max_seqlen, int H,
    float scale, hipStream_t strm) {
  if (!state) return hipErrorInvalidValue;
  return fa_varlen_bwd<true>(qkv, ctx, dctx, lse, delta, cu_seqlens,
                             AttnDropArgs{state, site, thr, rs}, dqkv, N, T,
                             max_seqlen, H, scale, strm);
}
