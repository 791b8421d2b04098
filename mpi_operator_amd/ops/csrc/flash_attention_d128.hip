// Tiled ("flash") multi-head self-attention at head_dim 128 (bf16 in, fp32
// accumulation on v_mfma_f32_32x32x16_bf16): the maths, the layouts (128 in
// place of 64), the VARLEN and CAUSAL template parameters and every
// convention of flash_attention.hip — wave w owns rows w·32..+31 of a
// 128-row chunk, NT operands from an XOR-swizzled octet image (b128 reads),
// transposed operands from [4 k][16 col] subtile images (ds_read_b64_tr_b16,
// EXEC all ones: no lane returns early or branches around one), rows and
// columns past S computed on zeros and selected away, the finite FA_FLOOR
// running max, no float atomics (one workgroup per output element, fixed
// order: the backward is bit-reproducible). There is no dropout form.
//
// What differs is the LDS plan, since the D = 64 images do not scale: that
// file's dK/dV kernel already fills 128 KiB and would need 192 KiB here.
//
//   kernel   workgroup owns      loops over        LDS images
//   fwd      128 q-rows          128-key tiles     K NT 32 + V sub 32 + P 32
//                                                  = 96 KiB
//   dK/dV    64 key rows         128-row q-chunks  K NT 16 + V NT 16 + Q sub
//                                                  32 + dO sub 32 + P 16 + dS
//                                                  16 = 128 KiB
//   dQ       128 q-rows          128-key tiles     K NT 32 + V NT 32 + K sub
//                                                  32 + dS 32 = 128 KiB
//
// One workgroup (4 waves, up to 512 VGPRs a lane) per CU in all three. Q and
// dO of the wave's own rows live in registers as 8 A fragments each.
//
// dK/dV splits its two phases differently. Recompute: wave w owns q-rows
// w·32..+31 and both 32-key fragments, and writes P and dS (bf16) into
// [4 q][16 key] subtile images of 128 q × 64 keys. Accumulate: wave w owns
// key half w & 1 and d half w >> 1 and holds dK and dV as two 32×32
// fragments each (the D = 64 kernel's accumulator count), reading dSᵀ and Pᵀ
// with transpose reads as the A operand and Q / dO as B.
//
// CAUSAL: forward and dQ as in flash_attention.hip (tiles kt < c dense, the
// aligned diagonal tile kt == c with the future selected away; the forward
// also skips each wave's all-future fragments wave-uniformly; chunks are
// dispatched heaviest-first). A 64-key dK/dV chunk at kc0 starts at q-chunk
// kc0 / 128, to which it is not aligned, so that one chunk tests
// "key <= row" per element; the later chunks run the dense body. Block y
// does the most chunks at y = 0, so dK/dV is heaviest-first as it is.
#include "common.h"
#include "flash_common.h"
#include "launchers.h"

constexpr int FB_D = 128; // head dim: 16 octets (256 bytes) a row
constexpr int FB_KC = 64; // key rows of a dK/dV workgroup

// Octet slot of octet q in row `row` of an NT image with 256-byte rows. A
// b128 read is served 16 lanes at a time, and those 16 lanes read one octet
// q of 16 consecutive rows (row0 a multiple of 16). A row is exactly the 64
// banks, so unswizzled they would all hit the same 4 banks; q ^ (row & 15)
// sends them to 16 different slots = all 64 banks once. The staging writes
// (16 lanes = the 16 octets of one row) are a permutation of one row: also
// conflict-free. (The D = 64 image XORs row >> 2 because two of its 128-byte
// rows share a bank line.)
DEV_INLINE int fb_swz(int q, int row) { return q ^ (row & 15); }

// stage ROWS rows × 128 d starting at row0 as swizzled NT octets; rows >= S
// are ZERO (0·Inf = NaN from un-staged LDS would leak through the MFMAs)
template <int ROWS>
DEV_INLINE void fb_stage_nt(ushort8 *img, const uint16_t *src, long stride,
                            int row0, int S, int tid) {
  ushort8 z8{0, 0, 0, 0, 0, 0, 0, 0};
  for (int idx = tid; idx < ROWS * 16; idx += 256) {
    int row = idx >> 4, q = idx & 15;
    int g = row0 + row;
    img[row * 16 + fb_swz(q, row)] =
        g < S ? *(const ushort8 *)(src + (long)g * stride + q * 8) : z8;
  }
}

// stage 128 rows × 128 d starting at row0 as [4 k][16 d] subtiles (k = row,
// 8 column blocks: fa_sub128)
DEV_INLINE void fb_stage_tr(ushort8 *img, const uint16_t *src, long stride,
                            int row0, int S, int tid) {
  ushort8 z8{0, 0, 0, 0, 0, 0, 0, 0};
  for (int idx = tid; idx < FA_T * 16; idx += 256) {
    int st = idx >> 3, kq = st >> 3, cq = st & 7;
    int kl = (idx & 7) >> 1, ch = idx & 1;
    int g = row0 + kq * 4 + kl, d0 = cq * 16 + ch * 8;
    img[idx] = g < S ? *(const ushort8 *)(src + (long)g * stride + d0) : z8;
  }
}

// A fragments (8 k-steps over d) of the wave's 32 rows straight from global;
// rows >= S read as zero
DEV_INLINE void fb_load_rows(bf16x8a f[8], const uint16_t *src, long stride,
                             int row0, int S, int lane) {
  int r = row0 + (lane & 31);
  bool rok = r < S;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    int q = ks * 2 + (lane >> 5);
    f[ks] = fa_bf8(rok ? *(const ushort8 *)(src + (long)r * stride + q * 8)
                       : ushort8{0, 0, 0, 0, 0, 0, 0, 0});
  }
}

// 32 rows × 32 cols of A·Bᵀ over d: A fragments × NT image rows ni·32..+31
DEV_INLINE float16a fb_nt_frag(const bf16x8a af[8], const ushort8 *img, int ni,
                               int lane) {
  float16a a = {};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    int kr = ni * 32 + (lane & 31);
    int q = ks * 2 + (lane >> 5);
    bf16x8a kf = fa_bf8(img[kr * 16 + fb_swz(q, kr)]);
    a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], kf, a, 0, 0, 0);
  }
  return a;
}

// Causal visibility. C-layout register r of a lane sits at row
// row0 + (r & 3) + 8·(r >> 2) + 4·(lane >> 5), so with
//   cv = column − row0 − 4·(lane >> 5)      (global indices, one VGPR)
// "column <= row" is cv <= (r & 3) + 8·(r >> 2): a compile-time constant.
DEV_INLINE bool fb_vis(int cv, int r) { return cv <= (r & 3) + 8 * (r >> 2); }

// u16 offset of (row, col) in this wave's P image [32][128]: the octet of a
// row is XORed with row & 15, so the P·V A-operand read (32 lanes, 32 rows,
// one octet) spreads over the banks as fb_swz's does
DEV_INLINE int fb_poff(int row, int col) {
  return row * FA_T + (((col >> 3) ^ (row & 15)) << 3) + (col & 7);
}

// ------------------------------ forward ------------------------------
// One key tile of a forward block, K/V images staged by the caller: scores
// (4 fragments × 8 k-steps), online softmax, park P, O += P·V (4 fragments).
// DIAG: the diagonal tile of a CAUSAL block (k0 = the chunk's first row):
// future columns are excluded as columns >= S are, by selection, and this
// wave's all-future fragments (ni >= nfr) and their P·V k-steps are skipped
// wave-uniformly (scalar branch on the wave index, EXEC stays all ones).
template <bool DIAG>
DEV_INLINE void fb_fwd_tile(const bf16x8a qf[8], const ushort8 *k_img,
                            const ushort8 *v_img, uint16_t *p_w,
                            const float *mrow, int k0, int S, float scale,
                            int lane, int wave, float m_run[16],
                            float l_run[16], float16a oacc[4]) {
  const int nfr = DIAG ? __builtin_amdgcn_readfirstlane(wave) + 1 : 4;
  float16a acc[4];
  float mk[4];
  bool cok[4];
  int cv[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    if (!DIAG || ni < nfr)
      acc[ni] = fb_nt_frag(qf, k_img, ni, lane);
    else
      acc[ni] = float16a{};
    int col = k0 + ni * 32 + (lane & 31);
    cok[ni] = col < S;
    mk[ni] = (mrow && cok[ni]) ? mrow[col] : 0.f;
    cv[ni] = ni * 32 + (lane & 31) - wave * 32 - 4 * (lane >> 5);
  }
  // Columns >= S (and the future) are excluded EXACTLY: the floor into the
  // max and p = 0 by selection, never by adding to a score. A tile whose
  // keys are all masked leaves m where it was and adds nothing.
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float mt = FA_FLOOR;
    bool ok[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      ok[ni] = cok[ni] && (!DIAG || fb_vis(cv[ni], r));
      float v = ok[ni] ? acc[ni][r] * scale + mk[ni] : FA_FLOOR;
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
      float e = ok[ni] ? __expf(acc[ni][r] - m_new) : 0.f;
      acc[ni][r] = e;
      s += e;
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
      s += __shfl_xor(s, off, 64);
    m_run[r] = m_new;
    l_run[r] = l_run[r] * alpha + s;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) oacc[ni][r] *= alpha;
  }
  // park the (unnormalized) P tile; DIAG: fragments ni >= nfr are never read
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    if (DIAG && ni >= nfr) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      p_w[fb_poff(fa_crow(r, lane), ni * 32 + (lane & 31))] = f2bf(acc[ni][r]);
  }
  // per-wave private image: a wave-level LDS fence suffices
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int ks = 0; ks < FA_T / 16; ++ks) {
    if (DIAG && ks >= 2 * nfr) continue; // P is zero from here on
    int kk = ks * 16 + (lane >> 5) * 8;
    bf16x8a pf = fa_bf8(*(const ushort8 *)&p_w[fb_poff(lane & 31, kk)]);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
      int cq = ni * 2 + ((lane >> 4) & 1);
      bf16x8a vf = fa_tr_frag<8>(v_img, kq0, cq, lane);
      oacc[ni] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, oacc[ni], 0, 0, 0);
    }
  }
}

// grid (B·H, ceil(S/128)); LDS K 32 KiB + V 32 KiB + P 32 KiB = 96 KiB.
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
// CAUSAL: block row y owns chunk yc = gridDim.y − 1 − y: key tiles 0..yc − 1
// dense, then tile yc as the diagonal.
template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash128_fwd_k(
    const uint16_t *__restrict__ qkv, // [B, S, 3, H, 128]
    uint16_t *__restrict__ ctx,       // [B, S, H*128]
    float *__restrict__ lse,          // [B, H, S]
    const float *__restrict__ mask_,  // [B, S] additive (or nullptr)
    int B, int S_, int H, float scale, FaVarlen vl) {
  constexpr int D = FB_D, T = FA_T;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  const FaSeq sq = fa_seq<VARLEN>(bh, H, S_, vl);
  const int S = sq.S;
  const int yc = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  // workgroup-uniform, ahead of the first barrier
  if (VARLEN && yc * T >= S) return;
  const float *mrow = (VARLEN || !mask_) ? nullptr : mask_ + (long)b * S;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  __shared__ __align__(128) ushort8 k_img[T * 16];
  __shared__ __align__(128) ushort8 v_img[T * 16];
  __shared__ __align__(128) uint16_t p_img[4][32 * T];

  const long qkv_row = (long)3 * H * D;
  const uint16_t *base = qkv + sq.tok0 * qkv_row;
  const uint16_t *qp = base + h * D;
  const uint16_t *kp = base + (long)1 * H * D + h * D;
  const uint16_t *vp = base + (long)2 * H * D + h * D;

  // A wave whose 32 q-rows are all >= S stays in the loop (zero Q, nothing
  // written): every wave must reach both barriers of every tile.
  int qrow0 = yc * T + wave * 32;
  bf16x8a qf[8];
  fb_load_rows(qf, qp, qkv_row, qrow0, S, lane);

  float m_run[16], l_run[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    m_run[r] = FA_FLOOR;
    l_run[r] = 0.f;
  }
  float16a oacc[4] = {};

  // CAUSAL: chunk yc exists (yc·T < S), so the tiles 0..yc all do
  const int nkt = CAUSAL ? yc : (S + T - 1) / T;
  for (int kt = 0; kt < nkt; ++kt) {
    // first barrier: no wave is still reading the previous tile's K/V
    // images; second: the new images are complete
    __syncthreads();
    fb_stage_nt<T>(k_img, kp, qkv_row, kt * T, S, tid);
    fb_stage_tr(v_img, vp, qkv_row, kt * T, S, tid);
    __syncthreads();
    fb_fwd_tile<false>(qf, k_img, v_img, p_img[wave], mrow, kt * T, S, scale,
                       lane, wave, m_run, l_run, oacc);
  }
  if constexpr (CAUSAL) {
    __syncthreads();
    fb_stage_nt<T>(k_img, kp, qkv_row, yc * T, S, tid);
    fb_stage_tr(v_img, vp, qkv_row, yc * T, S, tid);
    __syncthreads();
    fb_fwd_tile<true>(qf, k_img, v_img, p_img[wave], mrow, yc * T, S, scale,
                      lane, wave, m_run, l_run, oacc);
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
    float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      cp[(long)row * crow + ni * 32 + (lane & 31)] = f2bf(oacc[ni][r] * inv);
    if ((lane & 31) == 0)
      lse[sq.lse0 + row] = l > 0.f ? m_run[r] + __logf(l) : m_run[r];
  }
}

// ------------------------------ backward ------------------------------
// delta[b, h, i] = Σ_d dctx[b, i, h·128+d]·ctx[b, i, h·128+d]: 16 lanes per
// (b, i, h) row, one 16-B load each, 4-step shuffle reduce.
__global__ __launch_bounds__(256) void flash128_delta_k(
    const uint16_t *__restrict__ ctx, const uint16_t *__restrict__ dctx,
    float *__restrict__ delta, int B, int S, int H) {
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  long rowid = t >> 4; // (b·S + i)·H + h
  int oct = (int)(t & 15);
  long nrows = (long)B * S * H;
  float acc = 0.f;
  if (rowid < nrows) {
    ushort8 c = *(const ushort8 *)(ctx + rowid * FB_D + oct * 8);
    ushort8 d = *(const ushort8 *)(dctx + rowid * FB_D + oct * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += bf2f(c[i]) * bf2f(d[i]);
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (rowid < nrows && oct == 0) {
    int h = (int)(rowid % H);
    long bi = rowid / H;
    int i = (int)(bi % S);
    long b = bi / S;
    delta[(b * H + h) * S + i] = acc;
  }
}

// P and dS fragment (32 q-rows × 32 keys) recomputed from lse/delta and
// written as bf16 at image row rw + fa_crow, column ni·32 + (lane & 31) of
// [4 q][16 key] subtile images with CQ column blocks (`p16` may be nullptr:
// dQ needs dS only). The caller passes lse_r = +inf for q-rows >= S, so
// that exp(. − inf) = 0 gives those rows' exact zeros without 16 live row
// predicates; keys >= S (cok false) get exactly 0 by selection.
// DIAG: the keys in the future of a q-row get p = 0, hence dS = 0 (cv as
// for fb_vis, from global indices).
template <bool DIAG, int CQ>
DEV_INLINE void fb_pds_frag(const bf16x8a qf[8], const bf16x8a dof[8],
                            const ushort8 *k_nt, const ushort8 *v_nt, int ni,
                            int lane, int rw, bool cok, float mk,
                            const float lse_r[16], const float delta_r[16],
                            float scale, uint16_t *p16, uint16_t *ds16,
                            int cv) {
  float16a s = fb_nt_frag(qf, k_nt, ni, lane);
  float16a dp = fb_nt_frag(dof, v_nt, ni, lane);
  int col = ni * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = rw + fa_crow(r, lane);
    float p = (cok && (!DIAG || fb_vis(cv, r)))
                  ? __expf(s[r] * scale + mk - lse_r[r]) : 0.f;
    float ds = (dp[r] - delta_r[r]) * p * scale;
    int off = ((row >> 2) * CQ + (col >> 4)) * 64 + (row & 3) * 16 + (col & 15);
    if (p16) p16[off] = f2bf(p);
    ds16[off] = f2bf(ds);
  }
}

// lse and delta of the wave's 16 C-layout rows from row0 on; rows >= S get
// lse = +inf (fb_pds_frag) and delta = 0
DEV_INLINE void fb_row_stats(float lse_r[16], float delta_r[16],
                             const float *lsep, const float *delp, int row0,
                             int S, int lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = row0 + fa_crow(r, lane);
    bool rok = row < S;
    lse_r[r] = rok ? lsep[row] : INFINITY;
    delta_r[r] = rok ? delp[row] : 0.f;
  }
}

// pointers of one (sequence, head) for the backward kernels
struct FbBwdPtrs {
  const uint16_t *qp, *kp, *vp, *dop;
  const float *lsep, *delp;
  long qrow, crow;
};

// One q-chunk (rows q0..q0+127) of a dK/dV block: stage Q and dO, recompute
// P and dS for this workgroup's 64 keys, then dK += dSᵀ·Q and dV += Pᵀ·dO.
// DIAG: the first chunk of a CAUSAL block, with the per-element future test.
template <bool DIAG>
DEV_INLINE void fb_dkv_chunk(const FbBwdPtrs &pt, const ushort8 *k_nt,
                             const ushort8 *v_nt, ushort8 *q_tr,
                             ushort8 *do_tr, ushort8 *p_tr, ushort8 *ds_tr,
                             int q0, int kc0, int S, float scale,
                             const bool cok[2], const float mk[2], int tid,
                             float16a dk[2], float16a dv[2]) {
  const int lane = tid & 63, wave = tid >> 6, sqw = wave * 32;
  // first barrier: the previous chunk's dK/dV reads of all four per-chunk
  // images are done; second: Q/dO (and, first time, K/V) are staged
  __syncthreads();
  fb_stage_tr(q_tr, pt.qp, pt.qrow, q0, S, tid);
  fb_stage_tr(do_tr, pt.dop, pt.crow, q0, S, tid);
  __syncthreads();

  // recompute: this wave's 32 q-rows × the 64 keys
  {
    bf16x8a qf[8], dof[8];
    fb_load_rows(qf, pt.qp, pt.qrow, q0 + sqw, S, lane);
    fb_load_rows(dof, pt.dop, pt.crow, q0 + sqw, S, lane);
    float lse_r[16], delta_r[16];
    fb_row_stats(lse_r, delta_r, pt.lsep, pt.delp, q0 + sqw, S, lane);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int cv = kc0 + ni * 32 + (lane & 31) - (q0 + sqw) - 4 * (lane >> 5);
      fb_pds_frag<DIAG, 4>(qf, dof, k_nt, v_nt, ni, lane, sqw, cok[ni], mk[ni],
                           lse_r, delta_r, scale, (uint16_t *)p_tr,
                           (uint16_t *)ds_tr, cv);
    }
  }
  __syncthreads();

  // accumulate: rows = key half kh (32 keys), cols = d half dh (2 × 32),
  // k = the 128 q-rows
  const int kh = wave & 1, dh = wave >> 1;
  for (int ks = 0; ks < 8; ++ks) {
    int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
    int cqa = kh * 2 + ((lane >> 4) & 1);
    bf16x8a a_ds = fa_tr_frag<4>(ds_tr, kq0, cqa, lane);
    bf16x8a a_p = fa_tr_frag<4>(p_tr, kq0, cqa, lane);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int cq = dh * 4 + ni * 2 + ((lane >> 4) & 1);
      bf16x8a b_q = fa_tr_frag<8>(q_tr, kq0, cq, lane);
      bf16x8a b_do = fa_tr_frag<8>(do_tr, kq0, cq, lane);
      dk[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_ds, b_q, dk[ni], 0, 0, 0);
      dv[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_p, b_do, dv[ni], 0, 0, 0);
    }
  }
}

template <bool VARLEN>
DEV_INLINE FbBwdPtrs fb_bwd_ptrs(const uint16_t *qkv, const uint16_t *dctx,
                                 const float *lse, const float *delta,
                                 const FaSeq &sq, int h, int H) {
  const long qrow = (long)3 * H * FB_D, crow = (long)H * FB_D;
  const uint16_t *base = qkv + sq.tok0 * qrow + h * FB_D;
  return {base, base + (long)H * FB_D, base + (long)2 * H * FB_D,
          dctx + sq.tok0 * crow + h * FB_D, lse + sq.lse0, delta + sq.lse0,
          qrow, crow};
}

// dK, dV: grid (B·H, ceil(S/64)) over 64-row key chunks, loop over q-chunks.
// LDS: K, V (NT, 64 rows, staged once) 2×16 KiB + Q, dO (subtile, per
// q-chunk) 2×32 KiB + P, dS (128 q × 64 keys) 2×16 KiB = 128 KiB.
// VARLEN: grid (N·H, ceil(max_seqlen/64)), B = N, S_ unused, no mask.
// CAUSAL: q-chunk kc0/128 with the future test, then the later ones dense.
template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash128_bwd_dkv_k(
    const uint16_t *__restrict__ qkv,   // [B, S, 3, H, 128]
    const uint16_t *__restrict__ dctx,  // [B, S, H*128]
    const float *__restrict__ lse,      // [B, H, S]
    const float *__restrict__ delta,    // [B, H, S]
    const float *__restrict__ mask_,    // [B, S] or nullptr
    uint16_t *__restrict__ dqkv,        // [B, S, 3, H, 128]
    int B, int S_, int H, float scale, FaVarlen vl) {
  constexpr int D = FB_D, T = FA_T, KC = FB_KC;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  const FaSeq sq = fa_seq<VARLEN>(bh, H, S_, vl);
  const int S = sq.S;
  const int kc0 = blockIdx.y * KC;
  // workgroup-uniform, ahead of the first barrier
  if (VARLEN && kc0 >= S) return;
  const float *mrow = (VARLEN || !mask_) ? nullptr : mask_ + (long)b * S;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  __shared__ __align__(128) ushort8 k_nt[KC * 16];
  __shared__ __align__(128) ushort8 v_nt[KC * 16];
  __shared__ __align__(128) ushort8 q_tr[T * 16];
  __shared__ __align__(128) ushort8 do_tr[T * 16];
  __shared__ __align__(128) ushort8 p_tr[T * 8];
  __shared__ __align__(128) ushort8 ds_tr[T * 8];

  const FbBwdPtrs pt = fb_bwd_ptrs<VARLEN>(qkv, dctx, lse, delta, sq, h, H);
  fb_stage_nt<KC>(k_nt, pt.kp, pt.qrow, kc0, S, tid);
  fb_stage_nt<KC>(v_nt, pt.vp, pt.qrow, kc0, S, tid);

  // this lane's 2 key columns (one per score fragment) are loop-invariant
  bool cok[2];
  float mk[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    int col = kc0 + ni * 32 + (lane & 31);
    cok[ni] = col < S;
    mk[ni] = (mrow && cok[ni]) ? mrow[col] : 0.f;
  }

  float16a dk[2] = {}, dv[2] = {};
  const int nqc = (S + T - 1) / T;
  // kc0 < S, so q-chunk kc0/128 exists
  const int qc0 = CAUSAL ? kc0 / T : 0;
  if constexpr (CAUSAL)
    fb_dkv_chunk<true>(pt, k_nt, v_nt, q_tr, do_tr, p_tr, ds_tr, qc0 * T, kc0,
                       S, scale, cok, mk, tid, dk, dv);
  for (int qc = CAUSAL ? qc0 + 1 : 0; qc < nqc; ++qc)
    fb_dkv_chunk<false>(pt, k_nt, v_nt, q_tr, do_tr, p_tr, ds_tr, qc * T, kc0,
                        S, scale, cok, mk, tid, dk, dv);

  const int kh = wave & 1, dh = wave >> 1;
  uint16_t *dk_out = dqkv + sq.tok0 * pt.qrow + (long)H * D + h * D;
  uint16_t *dv_out = dk_out + (long)H * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = kc0 + kh * 32 + fa_crow(r, lane);
    if (row >= S) continue;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int d = dh * 64 + ni * 32 + (lane & 31);
      dk_out[(long)row * pt.qrow + d] = f2bf(dk[ni][r]);
      dv_out[(long)row * pt.qrow + d] = f2bf(dv[ni][r]);
    }
  }
}

// One key tile (rows k0..k0+127) of a dQ block, K/V images staged by the
// caller: recompute dS, then dQ += dS·K. The dS image is written and read
// by the same wave (its own 32 q-rows = 8 private row blocks), so it needs
// a wave-level fence only. DIAG: the diagonal tile of a CAUSAL block.
template <bool DIAG>
DEV_INLINE void fb_dq_tile(const bf16x8a qf[8], const bf16x8a dof[8],
                           const ushort8 *k_nt, const ushort8 *v_nt,
                           const ushort8 *k_tr, ushort8 *ds_tr,
                           const float *mrow, int k0, int q0, int S, int lane,
                           int wave, const float lse_r[16],
                           const float delta_r[16], float scale,
                           float16a dq[4]) {
  const int sqw = wave * 32;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    int col = k0 + ni * 32 + (lane & 31);
    bool cok = col < S;
    float mk = (mrow && cok) ? mrow[col] : 0.f;
    int cv = col - (q0 + sqw) - 4 * (lane >> 5);
    fb_pds_frag<DIAG, 8>(qf, dof, k_nt, v_nt, ni, lane, sqw, cok, mk, lse_r,
                         delta_r, scale, nullptr, (uint16_t *)ds_tr, cv);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // A = dS (k-contiguous b128 at subtile-linear addresses)
  for (int ks = 0; ks < 8; ++ks) {
    int kk = ks * 16 + (lane >> 5) * 8;
    bf16x8a af = fa_bf8(*(const ushort8 *)((const uint16_t *)ds_tr +
                                           fa_sub128(sqw + (lane & 31), kk)));
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
      int cq = ni * 2 + ((lane >> 4) & 1);
      bf16x8a bf = fa_tr_frag<8>(k_tr, kq0, cq, lane);
      dq[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, dq[ni], 0, 0, 0);
    }
  }
}

// dQ: grid (B·H, ceil(S/128)) over q-chunks, loop over key tiles.
// LDS: K, V (NT) + K (subtile) 3×32 KiB + dS 32 KiB = 128 KiB.
// VARLEN: grid (N·H, ceil(max_seqlen/128)), B = N, S_ unused, no mask.
// CAUSAL: chunk yc as in the forward; key tiles 0..yc − 1 dense, then tile
// yc as the diagonal.
template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash128_bwd_dq_k(
    const uint16_t *__restrict__ qkv, const uint16_t *__restrict__ dctx,
    const float *__restrict__ lse, const float *__restrict__ delta,
    const float *__restrict__ mask_, uint16_t *__restrict__ dqkv, int B,
    int S_, int H, float scale, FaVarlen vl) {
  constexpr int D = FB_D, T = FA_T;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  const FaSeq sq = fa_seq<VARLEN>(bh, H, S_, vl);
  const int S = sq.S;
  const int yc = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const int q0 = yc * T;
  // workgroup-uniform, ahead of the first barrier
  if (VARLEN && q0 >= S) return;
  const float *mrow = (VARLEN || !mask_) ? nullptr : mask_ + (long)b * S;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  __shared__ __align__(128) ushort8 k_nt[T * 16];
  __shared__ __align__(128) ushort8 v_nt[T * 16];
  __shared__ __align__(128) ushort8 k_tr[T * 16];
  __shared__ __align__(128) ushort8 ds_tr[T * 16];

  const FbBwdPtrs pt = fb_bwd_ptrs<VARLEN>(qkv, dctx, lse, delta, sq, h, H);
  const int sqw = wave * 32;
  bf16x8a qf[8], dof[8];
  fb_load_rows(qf, pt.qp, pt.qrow, q0 + sqw, S, lane);
  fb_load_rows(dof, pt.dop, pt.crow, q0 + sqw, S, lane);
  float lse_r[16], delta_r[16];
  fb_row_stats(lse_r, delta_r, pt.lsep, pt.delp, q0 + sqw, S, lane);

  float16a dq[4] = {};
  const int nkt = CAUSAL ? yc : (S + T - 1) / T;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads(); // previous tile's K/V readers done
    fb_stage_nt<T>(k_nt, pt.kp, pt.qrow, kt * T, S, tid);
    fb_stage_nt<T>(v_nt, pt.vp, pt.qrow, kt * T, S, tid);
    fb_stage_tr(k_tr, pt.kp, pt.qrow, kt * T, S, tid);
    __syncthreads();
    fb_dq_tile<false>(qf, dof, k_nt, v_nt, k_tr, ds_tr, mrow, kt * T, q0, S,
                      lane, wave, lse_r, delta_r, scale, dq);
  }
  if constexpr (CAUSAL) {
    __syncthreads();
    fb_stage_nt<T>(k_nt, pt.kp, pt.qrow, q0, S, tid);
    fb_stage_nt<T>(v_nt, pt.vp, pt.qrow, q0, S, tid);
    fb_stage_tr(k_tr, pt.kp, pt.qrow, q0, S, tid);
    __syncthreads();
    fb_dq_tile<true>(qf, dof, k_nt, v_nt, k_tr, ds_tr, mrow, q0, q0, S, lane,
                     wave, lse_r, delta_r, scale, dq);
  }

  uint16_t *dq_out = dqkv + sq.tok0 * pt.qrow + h * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = q0 + sqw + fa_crow(r, lane);
    if (row >= S) continue;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      dq_out[(long)row * pt.qrow + ni * 32 + (lane & 31)] = f2bf(dq[ni][r]);
  }
}

// ------------------------------ launchers ------------------------------
template <bool VARLEN>
static hipError_t fb_fwd(const void *qkv, void *ctx, float *lse,
                         const float *mask, int B, int S, int H, float scale,
                         FaVarlen vl, int causal, hipStream_t strm) {
  int rows = VARLEN ? vl.max_seqlen : S;
  dim3 grid(B * H, (rows + FA_T - 1) / FA_T);
  auto k = causal ? flash128_fwd_k<VARLEN, true> : flash128_fwd_k<VARLEN, false>;
  k<<<grid, 256, 0, strm>>>((const uint16_t *)qkv, (uint16_t *)ctx, lse, mask,
                            B, S, H, scale, vl);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// delta, then dK/dV (64-key chunks) and dQ (128-row chunks)
template <bool VARLEN>
static hipError_t fb_bwd(const void *qkv, const void *ctx, const void *dctx,
                         const float *lse, float *delta, const float *mask,
                         void *dqkv, int B, int S, int H, float scale,
                         FaVarlen vl, int causal, hipStream_t strm) {
  // the packed layouts are the dense ones at B = 1, S = T
  long drows = VARLEN ? (long)vl.total * H : (long)B * S * H;
  flash128_delta_k<<<cdiv_h(drows * 16, 256), 256, 0, strm>>>(
      (const uint16_t *)ctx, (const uint16_t *)dctx, delta, VARLEN ? 1 : B,
      VARLEN ? vl.total : S, H);
  HIP_KERNEL_CHECK();
  int rows = VARLEN ? vl.max_seqlen : S;
  auto dkv = causal ? flash128_bwd_dkv_k<VARLEN, true>
                    : flash128_bwd_dkv_k<VARLEN, false>;
  dkv<<<dim3(B * H, (rows + FB_KC - 1) / FB_KC), 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, mask,
      (uint16_t *)dqkv, B, S, H, scale, vl);
  HIP_KERNEL_CHECK();
  auto dq = causal ? flash128_bwd_dq_k<VARLEN, true>
                   : flash128_bwd_dq_k<VARLEN, false>;
  dq<<<dim3(B * H, (rows + FA_T - 1) / FA_T), 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, lse, delta, mask,
      (uint16_t *)dqkv, B, S, H, scale, vl);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t flash128_fwd_launch(const void *qkv, void *ctx,
                                          float *lse, const float *mask, int B,
                                          int S, int H, float scale,
                                          int causal, hipStream_t strm) {
  if (B < 1 || S < 1 || H < 1) return hipErrorInvalidValue;
  return fb_fwd<false>(qkv, ctx, lse, mask, B, S, H, scale, FaVarlen{}, causal,
                       strm);
}

extern "C" hipError_t flash128_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const float *mask, void *dqkv, int B, int S, int H,
    float scale, int causal, hipStream_t strm) {
  if (B < 1 || S < 1 || H < 1) return hipErrorInvalidValue;
  return fb_bwd<false>(qkv, ctx, dctx, lse, delta, mask, dqkv, B, S, H, scale,
                       FaVarlen{}, causal, strm);
}

// Packed forward: zero ctx and lse (the rows past cu[N] stay zero), then one
// block row per (sequence slot, head).
extern "C" hipError_t flash128_varlen_fwd_launch(
    const void *qkv, void *ctx, float *lse, const int *cu_seqlens, int N, int T,
    int max_seqlen, int H, float scale, int causal, hipStream_t strm) {
  if (N < 1 || T < 1 || max_seqlen < 1 || H < 1 || !cu_seqlens)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(ctx, 0, (size_t)T * H * FB_D * 2, strm);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(lse, 0, (size_t)T * H * sizeof(float), strm);
  if (e != hipSuccess) return e;
  return fb_fwd<true>(qkv, ctx, lse, nullptr, N, 0, H, scale,
                      FaVarlen{cu_seqlens, T, max_seqlen}, causal, strm);
}

// Packed backward: delta over all T rows (ctx is zero past cu[N], so delta
// is too), dqkv zeroed for the rows past cu[N], then dK/dV and dQ.
extern "C" hipError_t flash128_varlen_bwd_launch(
    const void *qkv, const void *ctx, const void *dctx, const float *lse,
    float *delta, const int *cu_seqlens, void *dqkv, int N, int T,
    int max_seqlen, int H, float scale, int causal, hipStream_t strm) {
  if (N < 1 || T < 1 || max_seqlen < 1 || H < 1 || !cu_seqlens)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(dqkv, 0, (size_t)T * 3 * H * FB_D * 2, strm);
  if (e != hipSuccess) return e;
  return fb_bwd<true>(qkv, ctx, dctx, lse, delta, nullptr, dqkv, N, 0, H,
                      scale, FaVarlen{cu_seqlens, T, max_seqlen}, causal, strm);
}
