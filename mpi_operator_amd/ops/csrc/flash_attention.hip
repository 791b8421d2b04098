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
//
// CAUSAL (third template parameter of the three MFMA kernels): query row i
// of a sequence sees the keys j <= i of that sequence (positions counted from
// the sequence start under VARLEN); lse is that of the causal row. Q-chunks
// and key tiles are both 128 rows and aligned, so the work is a triangle of
// tiles and only its diagonal needs a per-element decision:
//   - forward and dQ block (.., c) walk the key tiles kt <= c, dK/dV block
//     (.., c) the q-chunks qc >= c. Tiles in the future are never staged,
//     multiplied or drawn for; the bounds depend on blockIdx and S only, so
//     every barrier stays workgroup-uniform.
//   - the past tiles run the dense tile body, unchanged and without any
//     causal test. The one diagonal tile (kt == c, qc == c) has a body of
//     its own (fa_fwd_diag, fa_dkv_diag, fa_dq_diag, instantiated by the
//     CAUSAL kernels only): a future column is excluded as a column >= S
//     is, by selection per (register row, column), floor into the max and
//     p = 0, which also zeroes dS. Nothing is added to a score. With the
//     key mask, excluded = future or masked.
//   - wave w owns rows w·32..+31 of the diagonal tile, so its column
//     fragments ni > w lie wholly in the future: the forward skips their
//     QKᵀ MFMAs, their keep draws and the k-steps >= 2(w+1) of P·V. The
//     decision is wave-uniform (scalar branches on the wave index, EXEC
//     stays all ones) and indexes registers at compile time. The backward
//     bodies do not trim: it measured slower there.
//   - forward and dQ block c does c + 1 tiles, so blockIdx.y is mapped to
//     chunks last-first (the heaviest blocks are dispatched first); dK/dV
//     block c does nqc − c and is heaviest-first as it is.
//   - DROP keep bits are keyed by (row, column), so a causal call draws the
//     dense call's bits of the lower triangle.
// A row always sees its own key, so causality alone leaves no empty row.
#include "common.h"
#include "flash_common.h"
#include "launchers.h"
#include "philox.h"

constexpr int FA_D = 64;    // head dim

// CAUSAL visibility inside the (aligned, 128×128) diagonal tile. Row r of
// the C layout sits at chunk offset sqw + fa_crow(r, lane) and column
// fragment ni holds column ni·32 + (lane & 31), so "column <= row" is
//   fa_cvis(lane, sqw) <= (r & 3) + 8·(r >> 2) − ni·32:
// one VGPR against a compile-time constant per (r, ni).
DEV_INLINE int fa_cvis(int lane, int sqw) {
  return (lane & 31) - 4 * (lane >> 5) - sqw;
}
DEV_INLINE bool fa_cvis_ok(int cv, int r, int ni) {
  return cv <= (r & 3) + 8 * (r >> 2) - ni * 32;
}

DEV_INLINE int fa_swz(int q, int row) { return q ^ ((row >> 2) & 7); }

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
// The diagonal tile of a CAUSAL forward block, K/V images staged by the
// caller: the dense tile body with the future columns selected away and
// this wave's all-future fragments (ni >= nfr) and k-steps skipped.
// p_w: this wave's P image; mrow: the batch row's key mask or nullptr.
// TWIN of the tile loop body in flash_attn_fwd_k (scores, online softmax,
// park, P·V), repeated here so the dense kernels never see the causal code:
// a fix to either must be made in both by hand.
template <bool DROP>
DEV_INLINE void fa_fwd_diag(const bf16x8a qf[4], const ushort8 *k_img,
                            const ushort8 *v_img, uint16_t (*p_w)[FA_T],
                            const float *mrow, int k0, int S, float scale,
                            int lane, int wave, int qrow0, const AttnDrop &dr,
                            float m_run[16], float l_run[16],
                            float16a oacc[2]) {
  const int nfr = __builtin_amdgcn_readfirstlane(wave) + 1;
  const int cv = fa_cvis(lane, wave * 32);
  float16a acc[4];
  float mk[4];
  bool cok[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    if (ni < nfr)
      acc[ni] = fa_nt_frag(qf, k_img, ni, lane);
    else
      acc[ni] = float16a{};
    int col = k0 + ni * 32 + (lane & 31);
    cok[ni] = col < S;
    mk[ni] = (mrow && cok[ni]) ? mrow[col] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float mt = FA_FLOOR;
    bool ok[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      ok[ni] = cok[ni] && fa_cvis_ok(cv, r, ni);
      float v = ok[ni] ? acc[ni][r] * scale + mk[ni] : FA_FLOOR;
      acc[ni][r] = v;
      mt = fmaxf(mt, v);
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
      mt = fmaxf(mt, __shfl_xor(mt, off, 64));
    float m_new = fmaxf(m_run[r], mt);
    float alpha = __expf(m_run[r] - m_new);
    float s = 0.f;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float e = ok[ni] ? __expf(acc[ni][r] - m_new) : 0.f;
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
  // park P (DROP: e·keep); the fragments ni >= nfr are never read below
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    if (ni >= nfr) continue;
    uint32_t kb = 0xffffu;
    if (DROP)
      kb = attn_drop_keep16(dr, (uint32_t)qrow0 >> 4, lane >> 5,
                            k0 + ni * 32 + (lane & 31));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      uint16_t pv = f2bf(acc[ni][r]);
      p_w[fa_crow(r, lane)][ni * 32 + (lane & 31)] =
          ((kb >> r) & 1u) ? pv : (uint16_t)0;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int ks = 0; ks < FA_T / 16; ++ks) {
    if (ks >= 2 * nfr) continue; // P is zero from here on
    int r = lane & 31, kk = ks * 16 + (lane >> 5) * 8;
    bf16x8a pf = fa_bf8(*(const ushort8 *)&p_w[r][kk]);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
      int cq = ni * 2 + ((lane >> 4) & 1);
      bf16x8a vf = fa_tr_frag<4>(v_img, kq0, cq, lane);
      oacc[ni] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, oacc[ni], 0, 0, 0);
    }
  }
}

// grid (B·H, ceil(S/128)); LDS K 16 KiB + V 16 KiB + P 32 KiB = 64 KiB
// (2 workgroups per CU).
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
// CAUSAL: block row y owns chunk yc = gridDim.y − 1 − y: key tiles 0..yc − 1
// in the dense body, then tile yc in fa_fwd_diag.
template <bool DROP, bool VARLEN = false, bool CAUSAL = false>
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
  const int yc = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  // workgroup-uniform, ahead of the first barrier
  if (VARLEN && yc * T >= S) return;
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
  int qrow0 = yc * T + wave * 32;
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

  // CAUSAL: chunk yc exists (yc·T < S), so the tiles 0..yc all do
  const int nkt = CAUSAL ? yc : (S + T - 1) / T;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * T;
    // first barrier: no wave is still reading the previous tile's K/V
    // images; second: the new images are complete
    __syncthreads();
    fa_stage_nt(k_img, kp, qkv_row, k0, S, tid);
    fa_stage_tr(v_img, vp, qkv_row, k0, S, tid);
    __syncthreads();

    // (this tile body has a TWIN for the diagonal tile, fa_fwd_diag: mirror
    // any fix there)
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
  if constexpr (CAUSAL) {
    const int k0 = yc * T;
    __syncthreads();
    fa_stage_nt(k_img, kp, qkv_row, k0, S, tid);
    fa_stage_tr(v_img, vp, qkv_row, k0, S, tid);
    __syncthreads();
    fa_fwd_diag<DROP>(qf, k_img, v_img, p_img[wave],
                      mask ? mask + (long)b * S : nullptr, k0, S, scale, lane,
                      wave, qrow0, dr, m_run, l_run, oacc);
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

// the forward instantiation for (DROP, VARLEN) and the runtime causal flag
template <bool DROP, bool VARLEN>
static hipError_t fa_fwd(const void *qkv, void *ctx, float *lse,
                         const float *mask, int B, int S, int H, float scale,
                         AttnDropArgs da, FaVarlen vl, int causal,
                         hipStream_t strm) {
  int rows = VARLEN ? vl.max_seqlen : S;
  dim3 grid(B * H, (rows + FA_T - 1) / FA_T);
  auto k = causal ? flash_attn_fwd_k<DROP, VARLEN, true>
                  : flash_attn_fwd_k<DROP, VARLEN, false>;
  k<<<grid, 256, 0, strm>>>((const uint16_t *)qkv, (uint16_t *)ctx, lse, mask,
                            B, S, H, scale, da, vl);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t flash_attn_fwd_launch(const void *qkv, void *ctx,
                                            float *lse, const float *mask,
                                            int B, int S, int H, float scale,
                                            int causal, hipStream_t strm) {
  if (S < 1) return hipErrorInvalidValue;
  return fa_fwd<false, false>(qkv, ctx, lse, mask, B, S, H, scale,
                              AttnDropArgs{}, FaVarlen{}, causal, strm);
}

extern "C" hipError_t flash_attn_drop_fwd_launch(
    const void *qkv, void *ctx, float *lse, const float *mask,
    const int64_t *state, uint32_t site, uint32_t thr, float rs, int B, int S,
    int H, float scale, int causal, hipStream_t strm) {
  if (S < 1 || !state) return hipErrorInvalidValue;
  return fa_fwd<true, false>(qkv, ctx, lse, mask, B, S, H, scale,
                             AttnDropArgs{state, site, thr, rs}, FaVarlen{},
                             causal, strm);
}

// Packed forward: zero ctx and lse (the rows past cu[N] stay zero), then one
// block row per (sequence slot, head).
template <bool DROP>
static hipError_t fa_varlen_fwd(const void *qkv, void *ctx, float *lse,
                                const int *cu_seqlens, AttnDropArgs da, int N,
                                int T, int max_seqlen, int H, float scale,
                                int causal, hipStream_t strm) {
  if (N < 1 || T < 1 || max_seqlen < 1 || H < 1 || !cu_seqlens)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(ctx, 0, (size_t)T * H * FA_D * 2, strm);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(lse, 0, (size_t)T * H * sizeof(float), strm);
  if (e != hipSuccess) return e;
  return fa_fwd<DROP, true>(qkv, ctx, lse, nullptr, N, 0, H, scale, da,
                            FaVarlen{cu_seqlens, T, max_seqlen}, causal, strm);
}

extern "C" hipError_t flash_attn_varlen_fwd_launch(
    const void *qkv, void *ctx, float *lse, const int *cu_seqlens, int N, int T,
    int max_seqlen, int H, float scale, int causal, hipStream_t strm) {
  return fa_varlen_fwd<false>(qkv, ctx, lse, cu_seqlens, AttnDropArgs{}, N, T,
                              max_seqlen, H, scale, causal, strm);
}

extern "C" hipError_t flash_attn_varlen_drop_fwd_launch(
    const void *qkv, void *ctx, float *lse, const int *cu_seqlens,
    const int64_t *state, uint32_t site, uint32_t thr, float rs, int N, int T,
    int max_seqlen, int H, float scale, int causal, hipStream_t strm) {
  if (!state) return hipErrorInvalidValue;
  return fa_varlen_fwd<true>(qkv, ctx, lse, cu_seqlens,
                             AttnDropArgs{state, site, thr, rs}, N, T,
                             max_seqlen, H, scale, causal, strm);
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
// DIAG (the diagonal tile of a CAUSAL kernel): the keys in the future of a
// q-row get p = 0, hence dS = 0, too; cv = fa_cvis(lane, sqw).
template <bool DROP, bool ROWINF = false, bool DIAG = false>
DEV_INLINE void fa_pds_frag(const bf16x8a qf[4], const bf16x8a dof[4],
                            const ushort8 *k_nt, const ushort8 *v_nt, int ni,
                            int lane, int sqw, bool cok, float mk,
                            const float lse_r[16], const float delta_r[16],
                            const bool rok[16], float scale, uint16_t *p16,
                            uint16_t *ds16, const AttnDrop &dr, uint32_t band0,
                            uint32_t gcol, int cv = 0) {
  float16a s = fa_nt_frag(qf, k_nt, ni, lane);
  float16a dp = fa_nt_frag(dof, v_nt, ni, lane);
  int col = ni * 32 + (lane & 31);
  uint32_t kb = 0;
  if (DROP) kb = attn_drop_keep16(dr, band0, lane >> 5, gcol);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = sqw + fa_crow(r, lane);
    float p = (cok && (ROWINF || rok[r]) && (!DIAG || fa_cvis_ok(cv, r, ni)))
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

// The diagonal q-chunk (qc == key chunk) of a CAUSAL dK/dV block, Q/dO
// images staged by the caller: the dense chunk body with the future keys
// of each q-row selected away. No wave-uniform trim here or in fa_dq_diag:
// skipping the all-future fragments and their k-steps measured 2 % slower
// on the whole backward (profiles/BENCH_HISTORY.md).
// TWIN of the recompute + accumulate part of the q-chunk loop body in
// flash_attn_bwd_dkv_k; that kernel's CAUSAL prologue also repeats the
// loop's staging and lse/delta row loads. Mirror a fix to one in the other.
template <bool DROP, bool ROWINF>
DEV_INLINE void fa_dkv_diag(const bf16x8a qf[4], const bf16x8a dof[4],
                            const ushort8 *k_nt, const ushort8 *v_nt,
                            const ushort8 *q_tr, const ushort8 *do_tr,
                            ushort8 *p_tr, ushort8 *ds_tr, int lane, int wave,
                            const bool cok[4], const float mk[4],
                            const float lse_r[16], const float delta_r[16],
                            const bool rok[16], float scale,
                            const AttnDrop &dr, int kc0, float16a dk[2],
                            float16a dv[2]) {
  const int sqw = wave * 32, cv = fa_cvis(lane, sqw);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    fa_pds_frag<DROP, ROWINF, true>(
        qf, dof, k_nt, v_nt, ni, lane, sqw, cok[ni], mk[ni], lse_r, delta_r,
        rok, scale, (uint16_t *)p_tr, (uint16_t *)ds_tr, dr,
        (uint32_t)(kc0 + sqw) >> 4, kc0 + ni * 32 + (lane & 31), cv);
  }
  __syncthreads();
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

// dK, dV: grid (B·H, ceil(S/128)) over key chunks, loop over q-chunks.
// LDS: K, V (NT, staged once) + Q, dO (subtile, per q-chunk) 4×16 KiB
// + P, dS 2×32 KiB = 128 KiB.
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
// CAUSAL: q-chunk blockIdx.y in fa_dkv_diag, then the later ones as dense.
template <bool DROP, bool VARLEN = false, bool CAUSAL = false>
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
  // fa_pds_frag's ROWINF: the CAUSAL kernels take it too (their DROP forms
  // spilled SGPRs on the 16 row predicates)
  constexpr bool RI = VARLEN || CAUSAL;
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
  if constexpr (CAUSAL) {
    // the diagonal chunk: the head of the loop body below, repeated (TWIN)
    __syncthreads();
    fa_stage_tr(q_tr, qp, qrow, kc0, S, tid);
    fa_stage_tr(do_tr, dop, crow, kc0, S, tid);
    __syncthreads();
    bf16x8a qf[4], dof[4];
    fa_load_rows(qf, qp, qrow, kc0 + sqw, S, lane);
    fa_load_rows(dof, dop, crow, kc0 + sqw, S, lane);
    float lse_r[16], delta_r[16];
    bool rok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int row = kc0 + sqw + fa_crow(r, lane);
      rok[r] = row < S;
      lse_r[r] = rok[r] ? lsep[row] : (RI ? INFINITY : 0.f);
      delta_r[r] = rok[r] ? delp[row] : 0.f;
    }
    fa_dkv_diag<DROP, RI>(qf, dof, k_nt, v_nt, q_tr, do_tr, p_tr, ds_tr,
                              lane, wave, cok, mk, lse_r, delta_r, rok, scale,
                              dr, kc0, dk, dv);
  }
  for (int qc = CAUSAL ? (int)blockIdx.y + 1 : 0; qc < nqc; ++qc) {
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
      lse_r[r] = rok[r] ? lsep[row] : (RI ? INFINITY : 0.f);
      delta_r[r] = rok[r] ? delp[row] : 0.f;
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      fa_pds_frag<DROP, RI>(
          qf, dof, k_nt, v_nt, ni, lane, sqw, cok[ni], mk[ni], lse_r, delta_r,
          rok, scale, (uint16_t *)p_tr, (uint16_t *)ds_tr, dr,
          (uint32_t)(q0 + sqw) >> 4, kc0 + ni * 32 + (lane & 31));
    __syncthreads();

    // dK += dSᵀ·Q, dV += Pᵀ·dO: rows = this wave's 32 keys, k = the 128 q
    // (this chunk body has a TWIN, fa_dkv_diag and the CAUSAL prologue
    // above: mirror any fix there)
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

// The diagonal key tile of a CAUSAL dQ block, K/V images staged by the
// caller. TWIN of the key-tile loop body in flash_attn_bwd_dq_k (recompute
// dS, dQ += dS·K): a fix to either must be made in both by hand.
template <bool DROP, bool ROWINF>
DEV_INLINE void fa_dq_diag(const bf16x8a qf[4], const bf16x8a dof[4],
                           const ushort8 *k_nt, const ushort8 *v_nt,
                           const ushort8 *k_tr, ushort8 *ds_tr,
                           const float *mrow, int k0, int S, int lane,
                           int wave, const float lse_r[16],
                           const float delta_r[16], const bool rok[16],
                           float scale, const AttnDrop &dr, float16a dq[2]) {
  const int sqw = wave * 32, cv = fa_cvis(lane, sqw);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    int col = k0 + ni * 32 + (lane & 31);
    bool cok = col < S;
    float mk = (mrow && cok) ? mrow[col] : 0.f;
    fa_pds_frag<DROP, ROWINF, true>(qf, dof, k_nt, v_nt, ni, lane, sqw, cok, mk,
                                   lse_r, delta_r, rok, scale, nullptr,
                                   (uint16_t *)ds_tr, dr,
                                   (uint32_t)(k0 + sqw) >> 4, col, cv);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
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

// dQ: grid (B·H, ceil(S/128)) over q-chunks, loop over key tiles.
// LDS: K, V (NT) + K (subtile) 3×16 KiB + dS 32 KiB = 80 KiB. The dS image
// is written and read by the same wave (its own 32 q-rows = 8 private row
// blocks), so it needs a wave-level fence only.
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
// CAUSAL: chunk yc as in the forward; key tiles 0..yc − 1 as dense, then
// tile yc in fa_dq_diag.
template <bool DROP, bool VARLEN = false, bool CAUSAL = false>
__global__ __launch_bounds__(256, CAUSAL ? 2 : 1) void flash_attn_bwd_dq_k(
    const uint16_t *__restrict__ qkv, const uint16_t *__restrict__ dctx,
    const float *__restrict__ lse, const float *__restrict__ delta,
    const float *__restrict__ mask_, uint16_t *__restrict__ dqkv, int B,
    int S_, int H, float scale, AttnDropArgs da, FaVarlen vl) {
  constexpr int D = FA_D, T = FA_T;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  const FaSeq sq = fa_seq<VARLEN>(bh, H, S_, vl);
  const int S = sq.S;
  const int yc = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const int q0 = yc * T;
  // fa_pds_frag's ROWINF for the CAUSAL DROP forms, which spilled SGPRs on
  // the row predicates (the others spilled a VGPR with it)
  constexpr bool RI = CAUSAL && DROP;
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
    lse_r[r] = rok[r] ? lsep[row] : (RI ? INFINITY : 0.f);
    delta_r[r] = rok[r] ? delp[row] : 0.f;
  }

  float16a dq[2] = {};
  AttnDrop dr{};
  if (DROP) dr = attn_drop_init(da, bh, VARLEN ? vl.max_seqlen : S);
  const int nkt = CAUSAL ? yc : (S + T - 1) / T;
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
      fa_pds_frag<DROP, RI>(qf, dof, k_nt, v_nt, ni, lane, sqw, cok, mk, lse_r,
                        delta_r, rok, scale, nullptr, (uint16_t *)ds_tr, dr,
                        (uint32_t)(q0 + sqw) >> 4, col);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // dQ += dS·K: A = dS (k-contiguous b128 at subtile-linear addresses)
    // (this tile body has a TWIN for the diagonal tile, fa_dq_diag)
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
  if constexpr (CAUSAL) {
    __syncthreads();
    fa_stage_nt(k_nt, kp, qrow, q0, S, tid);
    fa_stage_nt(v_nt, vp, qrow, q0, S, tid);
    fa_stage_tr(k_tr, kp, qrow, q0, S, tid);
    __syncthreads();
    fa_dq_diag<DROP, RI>(qf, dof, k_nt, v_nt, k_tr, ds_tr,
                     mask ? mask + (long)b * S : nullptr, q0, S, lane, wave,
                     lse_r, delta_r, rok, scale, dr, dq);
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

// the dK/dV and dQ instantiations for (DROP, VARLEN) and the
// runtime causal flag.
template <bool DROP, bool VARLEN>
static hipError_t fa_bwd(const void *qkv, const void *dctx, const float *lse,
                         float *delta, const float *mask,
                         void *dqkv, int B, int S, int H, float scale,
                         AttnDropArgs da, FaVarlen vl, int causal,
                         hipStream_t strm) {
  int rows = VARLEN ? vl.max_seqlen : S;
  dim3 grid(B * H, (rows + FA_T - 1) / FA_T);
  auto dkv = causal ? flash_attn_bwd_dkv_k<DROP, VARLEN, true>
                    : flash_attn_bwd_dkv_k<DROP, VARLEN, false>;
  dkv<<<grid, 256, 0, strm>>>((const uint16_t *)qkv, (const uint16_t *)dctx,
                              lse, delta, mask, (uint16_t *)dqkv, B, S, H,
                              scale, da, vl);
  HIP_KERNEL_CHECK();
  auto dq = causal ? flash_attn_bwd_dq_k<DROP, VARLEN, true>
                   : flash_attn_bwd_dq_k<DROP, VARLEN, false>;
  dq<<<grid, 256, 0, strm>>>((const uint16_t *)qkv, (const uint16_t *)dctx,
                             lse, delta, mask, (uint16_t *)dqkv, B, S, H,
                             scale, da, vl);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

static hipError_t fa_delta(const void *ctx, const void *dctx, float *delta,
                           int B, int S, int H, hipStream_t strm) {
  long nthr = (long)B * S * H * 8;
  flash_attn_delta_k<<<cdiv_h(nthr, 256), 256, 0, strm>>>(
      (const uint16_t *)ctx, (const uint16_t *)dctx, delta, B, S, H);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t flash_attn_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const float *mask, void *dqkv, int B, int S, int H,
    float scale, int causal, hipStream_t strm) {
  if (S < 1) return hipErrorInvalidValue;
  hipError_t e = fa_delta(ctx, dctx, delta, B, S, H, strm);
  if (e != hipSuccess) return e;
  return fa_bwd<false, false>(qkv, dctx, lse, delta, mask, dqkv, B, S, H,
                              scale, AttnDropArgs{}, FaVarlen{}, causal, strm);
}

// state, site, thr, rs: those of the forward; the masks are drawn again
extern "C" hipError_t flash_attn_drop_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const float *mask, const int64_t *state, uint32_t site,
    uint32_t thr, float rs, void *dqkv, int B, int S, int H, float scale,
    int causal, hipStream_t strm) {
  if (S < 1 || !state) return hipErrorInvalidValue;
  hipError_t e = fa_delta(ctx, dctx, delta, B, S, H, strm);
  if (e != hipSuccess) return e;
  return fa_bwd<true, false>(qkv, dctx, lse, delta, mask, dqkv, B, S, H,
                             scale, AttnDropArgs{state, site, thr, rs},
                             FaVarlen{}, causal, strm);
}

// Packed backward: delta over all T rows (the dense kernel at B = 1, S = T;
// ctx is zero past cu[N], so delta is too), dqkv zeroed for the rows past
// cu[N], then dK/dV and dQ with one block row per (sequence slot, head).
template <bool DROP>
static hipError_t fa_varlen_bwd(const void *qkv, const void *ctx,
                                const void *dctx, const float *lse,
                                float *delta, const int *cu_seqlens,
                                AttnDropArgs da, void *dqkv, int N, int T,
                                int max_seqlen, int H, float scale, int causal,
                                hipStream_t strm) {
  if (N < 1 || T < 1 || max_seqlen < 1 || H < 1 || !cu_seqlens)
    return hipErrorInvalidValue;
  hipError_t e = fa_delta(ctx, dctx, delta, 1, T, H, strm);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(dqkv, 0, (size_t)T * 3 * H * FA_D * 2, strm);
  if (e != hipSuccess) return e;
  return fa_bwd<DROP, true>(qkv, dctx, lse, delta, nullptr, dqkv, N, 0, H,
                            scale, da, FaVarlen{cu_seqlens, T, max_seqlen},
                            causal, strm);
}

extern "C" hipError_t flash_attn_varlen_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const int *cu_seqlens, void *dqkv, int N, int T,
    int max_seqlen, int H, float scale, int causal, hipStream_t strm) {
  return fa_varlen_bwd<false>(qkv, ctx, dctx, lse, delta, cu_seqlens,
                              AttnDropArgs{}, dqkv, N, T, max_seqlen, H, scale,
                              causal, strm);
}

// state, site, thr, rs: those of the forward; the masks are drawn again
extern "C" hipError_t flash_attn_varlen_drop_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const int *cu_seqlens, const int64_t *state, uint32_t site,
    uint32_t thr, float rs, void *dqkv, int N, int T, int max_seqlen, int H,
    float scale, int causal, hipStream_t strm) {
  if (!state) return hipErrorInvalidValue;
  return fa_varlen_bwd<true>(qkv, ctx, dctx, lse, delta, cu_seqlens,
                             AttnDropArgs{state, site, thr, rs}, dqkv, N, T,
                             max_seqlen, H, scale, causal, strm);
}
