// Fused multi-head self-attention forward for BERT (bf16, head_dim 64):
//   ctx[b, s, h·64+d] = softmax(Q·Kᵀ / √64 + mask) · V
//
// Replaces the hipBLASLt batched-GEMM + torch-softmax chain (reference
// role: the fused attention of the out-of-tree BERT images, SURVEY §2.3
// N7). MI355X-first structure:
//   - one workgroup per (batch, head): B·H blocks (BERT-Large bs32: 512 —
//     2 blocks/CU), 256 threads = 4 waves; wave w owns Q rows w·32..+31
//   - K staged in LDS [S][64] with the (row>>2)-XOR octet swizzle and read
//     as b128 MFMA B-fragments (k = head_dim, NT)
//   - V staged in LDS as [4 s_k][16 d] subtiles and consumed with
//     ds_read_b64_tr_b16 — the hardware transpose read (probed semantics:
//     lane receives column (l&15) of its 128-B block), so the PV operand
//     needs no repacking
//   - scores never leave registers: full-row softmax (fp32 max/exp/sum via
//     4-wide frag reduce + half-wave shfl) — S ≤ 512 keeps the whole row
//     resident, no online-softmax rescaling needed
//   - P crosses to the PV MFMA via one per-wave LDS image (the C-layout →
//     A-fragment transpose)
//   - probs optionally written out (bf16) for the torch-side backward
//
// Layouts: qkv is the fused projection output [B, S, 3, H, 64] (the model's
// qkv view before any transpose — the kernel does the head split itself);
// ctx is [B, S, H·64] so the consumer (attn.out linear) needs no reshape.
#include "common.h"
#include "launchers.h"
#include "philox.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8a;
typedef __attribute__((ext_vector_type(4))) float float4a;
typedef __attribute__((ext_vector_type(16))) float float16a;
typedef __attribute__((ext_vector_type(2))) unsigned int uint2a;

DEV_INLINE bf16x8a us8_to_bf8a(ushort8 u) {
  union { ushort8 u; bf16x8a b; } v;
  v.u = u;
  return v.b;
}

DEV_INLINE int att_swz(int q, int row) { return q ^ ((row >> 2) & 7); }

// S_MAX: compile-time sequence capacity (LDS sizing); launched per actual S.
// DROP: dropout on P with the attention mask scheme of philox.h. The P image
// takes keep ? bf16(P) : 0, the fp32 accumulator of P·V is scaled by
// 1/(1 - p_eff) before the ctx store, and the saved probs keep bf16(P) with
// the SIGN BIT set where dropped (P >= 0, so the bit is free): the backward
// needs both P and the mask and gets them from the one tensor.
template <int S_MAX, bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_k(
    const uint16_t *__restrict__ qkv, // [B, S, 3, H, 64]
    uint16_t *__restrict__ ctx,       // [B, S, H*64]
    uint16_t *__restrict__ probs,     // [B, H, S, S] or nullptr
    const float *__restrict__ mask,   // [B, S] additive (or nullptr)
    int B, int S, int H, float scale, AttnDropArgs da) {
  constexpr int D = 64;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // LDS: K [S_MAX][8 slots] (swizzled octets), V subtiles [S_MAX/4][4][16],
  // P per-wave [32][S_MAX]
  __shared__ __align__(128) ushort8 k_img[S_MAX * 8];
  __shared__ __align__(128) ushort8 v_img[S_MAX * 8];
  __shared__ __align__(128) uint16_t p_img[4][32][S_MAX];

  const long qkv_row = (long)3 * H * D; // elements per (b, s)
  const uint16_t *base = qkv + (long)b * S * qkv_row;
  const uint16_t *kp = base + (long)1 * H * D + h * D;
  const uint16_t *vp = base + (long)2 * H * D + h * D;

  // stage K/V padded to a 32-row multiple with ZEROS — un-staged LDS
  // garbage can be Inf/NaN bf16 patterns, and 0·Inf = NaN would leak
  // through the padded score columns
  // staged to the full S_MAX capacity so every compile-time-unrolled
  // fragment read sees defined (zero) data
  ushort8 z8{0, 0, 0, 0, 0, 0, 0, 0};
  // K: thread t covers octet slices; row = s_k, 8 octets per row
  for (int idx = tid; idx < S_MAX * 8; idx += 256) {
    int row = idx >> 3, q = idx & 7;
    // store octet q of row at slot q^swz(row): read side XORs the same
    k_img[row * 8 + att_swz(q, row)] =
        row < S ? *(const ushort8 *)(kp + (long)row * qkv_row + q * 8) : z8;
  }
  // V: subtile st = (kq, cq): rows kq*4..+3 (s_k), cols cq*16..+15 (d)
  // slot layout: [st][kl*2 + ch] with ch = 8-col half (TnPipe image)
  for (int idx = tid; idx < S_MAX * 8; idx += 256) {
    int st = idx >> 3, kq = st >> 2, cq = st & 3;
    int kl = (idx & 7) >> 1, ch = idx & 1;
    int sk = kq * 4 + kl, d0 = cq * 16 + ch * 8;
    v_img[idx] =
        sk < S ? *(const ushort8 *)(vp + (long)sk * qkv_row + d0) : z8;
  }
  __syncthreads();

  // Q fragments straight from global: lane holds row (l&31), k-octet (l>>5).
  // blockIdx.y selects the 128-row q-chunk: a block's 4 waves cover 128
  // q-rows, so S in (128, 256] launches TWO chunks per (b, h) — the first
  // S_MAX=256 cut covered only rows 0..127 and left ctx rows 128+ as
  // uninitialized memory (NaN loss at seq 256; caught by the edge sweep).
  int qrow0 = blockIdx.y * 128 + wave * 32;
  if (qrow0 >= S) return; // short sequences: idle waves (after the barrier)
  const uint16_t *qp = base + h * D;
  bf16x8a qf[4]; // 4 k-steps of 16 over D=64
  {
    int r = qrow0 + (lane & 31);
    bool rok = r < S;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      int q = ks * 2 + (lane >> 5);
      qf[ks] = us8_to_bf8a(rok ? *(const ushort8 *)(qp + (long)r * qkv_row + q * 8)
                               : ushort8{0, 0, 0, 0, 0, 0, 0, 0});
    }
  }

  // scores: per wave 32 rows × S_MAX cols as compile-time col-frags.
  // COMPILE-TIME bounds are load-bearing: a runtime `nf` bound makes
  // acc[] runtime-indexed → every accumulator spills to scratch (the
  // first cut of this kernel ran 168 µs; padded frags compute zeros
  // instead and the -inf mask drops them)
  constexpr int NF = S_MAX / 32;
  float16a acc[NF];
#pragma unroll
  for (int ni = 0; ni < NF; ++ni) {
    float16a a = {};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      int kr = ni * 32 + (lane & 31); // key row for the B fragment
      int q = ks * 2 + (lane >> 5);
      bf16x8a kf = us8_to_bf8a(k_img[kr * 8 + att_swz(q, kr)]);
      a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kf, a, 0, 0, 0);
    }
    acc[ni] = a;
  }

  // row softmax in fp32. value (row, col): reg r of frag ni belongs to
  // row = qrow0 + (r&3) + 8*(r>>2) + 4*(lane>>5), col = ni*32 + (lane&31):
  // a row's values live in one half-wave at fixed r across frags.
  float srow[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float m = -3.4e38f;
#pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      float v = acc[ni][r] * scale;
      int col = ni * 32 + (lane & 31);
      if (col >= S)
        v = -3.4e38f; // padded key columns (SET, not add: acc was garbage)
      else if (mask)
        v += mask[(long)b * S + col];
      acc[ni][r] = v;
      m = fmaxf(m, v);
    }
    // half-wave reduce (the 32 lanes holding this row)
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
      m = fmaxf(m, __shfl_xor(m, off, 64));
    float s = 0.f;
#pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      float e = __expf(acc[ni][r] - m);
      acc[ni][r] = e;
      s += e;
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
      s += __shfl_xor(s, off, 64);
    srow[r] = 1.f / s;
  }

  // keep bits of this lane's 16 registers per column fragment (two Philox
  // calls each); columns >= S hold P = 0 whatever they draw
  uint32_t kb[NF];
  if (DROP) {
    AttnDrop dr = attn_drop_init(da, bh, S);
#pragma unroll
    for (int ni = 0; ni < NF; ++ni)
      kb[ni] = attn_drop_keep16(dr, (uint32_t)qrow0 >> 4, lane >> 5,
                                ni * 32 + (lane & 31));
  }

  // normalize + park P in this wave's LDS image (and optionally to global)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int prow = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      int col = ni * 32 + (lane & 31);
      uint16_t pv = f2bf(acc[ni][r] * srow[r]);
      uint16_t sv = pv; // as saved
      if (DROP) {
        bool keep = (kb[ni] >> r) & 1u;
        sv = keep ? pv : (uint16_t)(pv | 0x8000u);
        pv = keep ? pv : (uint16_t)0;
      }
      p_img[wave][prow][col] = pv;
      if (probs && col < S && qrow0 + prow < S)
        probs[((long)bh * S + qrow0 + prow) * S + col] = sv;
    }
  }
  // P image is per-wave private; the producing lanes and consuming lanes
  // are in the SAME wave, so a wave-level LDS fence suffices (no barrier:
  // waves run decoupled from here on)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // O = P·V: A-frags from p_img (row-major b128), B-frags via tr_b16
  float16a oacc[2] = {};
  unsigned vbase = (unsigned)(unsigned long)(
      __attribute__((address_space(3))) const void *)v_img;
  constexpr int NKS = S_MAX / 16; // padded P cols / V rows are zero
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    bf16x8a pf;
    {
      int r = lane & 31, k0 = ks * 16 + (lane >> 5) * 8;
      pf = us8_to_bf8a(*(const ushort8 *)&p_img[wave][r][k0]);
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      // V fragment: lane holds d-col (ni*32 + l&31), k 8 deep at
      // ks*16 + (l>>5)*8: two tr reads at consecutive k-subtiles
      int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
      int cq = ni * 2 + ((lane >> 4) & 1);
      unsigned a0 = vbase + (unsigned)((kq0 * 4 + cq) * 128 + (lane & 15) * 8);
      uint2a lo, hi;
      asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                   "ds_read_b64_tr_b16 %1, %2 offset:512\n\t"
                   "s_waitcnt lgkmcnt(0)"
                   : "=&v"(lo), "=&v"(hi)
                   : "v"(a0)
                   : "memory");
      union { unsigned u[4]; bf16x8a v; } vv;
      vv.u[0] = lo.x; vv.u[1] = lo.y; vv.u[2] = hi.x; vv.u[3] = hi.y;
      oacc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vv.v, oacc[ni],
                                                         0, 0, 0);
    }
  }

  // write ctx [b][s][h*64 + d]
  long crow = (long)H * D;
  uint16_t *cp = ctx + (long)b * S * crow + h * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = qrow0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row >= S) continue;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int d = ni * 32 + (lane & 31);
      cp[(long)row * crow + d] =
          f2bf(DROP ? oacc[ni][r] * da.rs : oacc[ni][r]);
    }
  }
}

template <bool DROP>
static hipError_t attn_fwd_dispatch(const void *qkv, void *ctx, void *probs,
                                    const float *mask, int B, int S, int H,
                                    float scale, AttnDropArgs da,
                                    hipStream_t strm) {
  // LDS: S_MAX=128 → 64 KiB (2 blocks/CU); S_MAX=256 → 128 KiB (1/CU).
  // S > 256 needs a tiled/online-softmax variant (flash_attention.hip).
  if (S <= 128)
    attn_fwd_k<128, DROP><<<dim3(B * H, 1), 256, 0, strm>>>(
        (const uint16_t *)qkv, (uint16_t *)ctx, (uint16_t *)probs, mask, B, S,
        H, scale, da);
  else if (S <= 256) // two 128-row q-chunks per (b, h)
    attn_fwd_k<256, DROP><<<dim3(B * H, 2), 256, 0, strm>>>(
        (const uint16_t *)qkv, (uint16_t *)ctx, (uint16_t *)probs, mask, B, S,
        H, scale, da);
  else
    return hipErrorInvalidValue;
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

extern "C" hipError_t attn_fwd_launch(const void *qkv, void *ctx, void *probs,
                                      const float *mask, int B, int S, int H,
                                      float scale, hipStream_t strm) {
  return attn_fwd_dispatch<false>(qkv, ctx, probs, mask, B, S, H, scale,
                                  AttnDropArgs{}, strm);
}

// probs is required: it carries the mask to the backward
extern "C" hipError_t attn_drop_fwd_launch(const void *qkv, void *ctx,
                                           void *probs, const float *mask,
                                           const int64_t *state, uint32_t site,
                                           uint32_t thr, float rs, int B,
                                           int S, int H, float scale,
                                           hipStream_t strm) {
  if (!probs || !state) return hipErrorInvalidValue;
  return attn_fwd_dispatch<true>(qkv, ctx, probs, mask, B, S, H, scale,
                                 AttnDropArgs{state, site, thr, rs}, strm);
}

// ---- fused attention backward (S == 128, D == 64) ---------------------
// Per (b, h) block, 256 threads / 4 waves — replaces the torch chain
// (4 hipBLASLt batched GEMMs + fp32 probs materialization + softmax-grad
// elementwise + the dqkv stack copy, ~12% of a BERT-Large step):
//   dP = dO·Vᵀ;  dS = (dP − rowsum(dP∘P))∘P·scale
//   dQ = dS·K;   dK = dSᵀ·Q;   dV = Pᵀ·dO     (all written straight into
//   the [B,S,3,H,64] dqkv gradient layout — no stack, no transposes)
// Transposed operands ride tr-subtile LDS images ([4 k][16 col] blocks,
// ds_read_b64_tr_b16); dS lives in ONE such image that serves both the
// k-contiguous dQ reads (b128 at subtile-linear addresses) and the
// k-strided dK reads (tr pairs).
// DROP: probs is the forward's sign-coded tensor (sign bit = dropped). The
// dS pass decodes |P| and keep where it consumes p_tr, takes
// dP = rs·keep∘(dO·Vᵀ), and writes keep ? P : 0 back into the element it just
// read (each element has one owner lane), so the dV reads after the barrier
// see P∘keep; dV is scaled by rs at the store.
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_k(
    const uint16_t *__restrict__ qkv,   // [B, S, 3, H, 64]
    const uint16_t *__restrict__ dctx,  // [B, S, H*64]
    const uint16_t *__restrict__ probs, // [B, H, S, S]
    uint16_t *__restrict__ dqkv,        // [B, S, 3, H, 64]
    int B, int H, float scale, float rs) {
  constexpr int S = 128, D = 64;
  int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // tr-subtile images: [4 k][16 col] blocks, cq-fastest.
  // S×S images (P, dS) hold S*S/8 = S*16 slots; S×D images S*D/8 = S*8.
  __shared__ __align__(128) ushort8 p_tr[S * 16];  // k=sq, col=sk  (32 KB)
  __shared__ __align__(128) ushort8 ds_tr[S * 16]; // k=sq, col=sk  (32 KB)
  __shared__ __align__(128) ushort8 do_tr[S * 8];  // k=sq, col=d   (16 KB)
  __shared__ __align__(128) ushort8 k_tr[S * 8];   // k=sk, col=d
  __shared__ __align__(128) ushort8 q_tr[S * 8];   // k=sq, col=d
  __shared__ __align__(128) ushort8 v_nt[S * 8];   // [sk][8 d-octets], swizzled

  const long qrow = (long)3 * H * D;
  const uint16_t *base = qkv + (long)b * S * qrow;
  const uint16_t *qp = base + h * D;
  const uint16_t *kp = base + (long)H * D + h * D;
  const uint16_t *vp = base + (long)2 * H * D + h * D;
  const long crow = (long)H * D;
  const uint16_t *dop = dctx + (long)b * S * crow + h * D;
  const uint16_t *pp = probs + (long)bh * S * S;

  // stage: v as swizzled NT rows; q/k/do as [4][16-d] subtiles (cq=4);
  // p as [4][16-sk] subtiles (cq=8)
  for (int idx = tid; idx < S * 8; idx += 256) {
    int row = idx >> 3, q = idx & 7;
    v_nt[row * 8 + att_swz(q, row)] =
        *(const ushort8 *)(vp + (long)row * qrow + q * 8);
  }
  for (int idx = tid; idx < S * 8; idx += 256) {
    int st = idx >> 3, kq = st >> 2, cq = st & 3;
    int kl = (idx & 7) >> 1, ch = idx & 1;
    int r = kq * 4 + kl, d0 = cq * 16 + ch * 8;
    q_tr[idx] = *(const ushort8 *)(qp + (long)r * qrow + d0);
    k_tr[idx] = *(const ushort8 *)(kp + (long)r * qrow + d0);
    do_tr[idx] = *(const ushort8 *)(dop + (long)r * crow + d0);
  }
  for (int idx = tid; idx < S * 16; idx += 256) {
    int st = idx >> 3, kq = st >> 3, cq = st & 7;
    int kl = (idx & 7) >> 1, ch = idx & 1;
    int sq = kq * 4 + kl, sk0 = cq * 16 + ch * 8;
    p_tr[idx] = *(const ushort8 *)(pp + (long)sq * S + sk0);
  }
  __syncthreads();

  // dP = dO·Vᵀ (per wave: sq rows wave*32..+31, all 128 sk)
  int sq0 = wave * 32;
  float16a acc[4];
  {
    bf16x8a dof[4];
    int r = sq0 + (lane & 31);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      int q = ks * 2 + (lane >> 5);
      dof[ks] = us8_to_bf8a(*(const ushort8 *)(dop + (long)r * crow + q * 8));
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float16a a = {};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        int kr = ni * 32 + (lane & 31);
        int q = ks * 2 + (lane >> 5);
        bf16x8a vf = us8_to_bf8a(v_nt[kr * 8 + att_swz(q, kr)]);
        a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof[ks], vf, a, 0, 0, 0);
      }
      acc[ni] = a;
    }
  }

  // dS = (dP − rowsum(dP∘P))∘P·scale, written into ds_tr's subtile slots
  unsigned pbase = (unsigned)(unsigned long)(
      __attribute__((address_space(3))) const void *)p_tr;
  uint16_t *ds16 = (uint16_t *)ds_tr;
  uint16_t *p16 = (uint16_t *)p_tr;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int sq = sq0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    float pv[4], t = 0.f;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int sk = ni * 32 + (lane & 31);
      // element (sq, sk) in the [4 sq][16 sk] subtile image
      int off = ((sq >> 2) * 8 + (sk >> 4)) * 64 + (sq & 3) * 16 + (sk & 15);
      if (DROP) {
        uint16_t u = p16[off];
        bool keep = !(u & 0x8000u); // the bit itself: a dropped +0 is -0
        pv[ni] = bf2f((uint16_t)(u & 0x7fffu));
        acc[ni][r] = keep ? acc[ni][r] * rs : 0.f;
        p16[off] = keep ? u : (uint16_t)0;
      } else {
        pv[ni] = bf2f(p16[off]);
      }
      t += acc[ni][r] * pv[ni];
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
      t += __shfl_xor(t, off, 64);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int sk = ni * 32 + (lane & 31);
      int off = ((sq >> 2) * 8 + (sk >> 4)) * 64 + (sq & 3) * 16 + (sk & 15);
      ds16[off] = f2bf((acc[ni][r] - t) * pv[ni] * scale);
    }
  }
  __syncthreads();

  // helper: tr-fragment read from a [4 k][16 col] subtile image
  auto tr_frag = [&](const ushort8 *img, int CQ, int kq0, int cq) -> bf16x8a {
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
  };

  long drow = (long)3 * H * D;
  uint16_t *dq_out = dqkv + (long)b * S * drow + h * D;
  uint16_t *dk_out = dq_out + (long)H * D;
  uint16_t *dv_out = dq_out + (long)2 * H * D;

  // dQ = dS·K: A = ds (k-contig over sk via subtile-linear b128), B = k_tr
  {
    float16a dq[2] = {};
    for (int ks = 0; ks < 8; ++ks) {
      int sq = sq0 + (lane & 31);
      int k0 = ks * 16 + (lane >> 5) * 8;
      const ushort8 *ap = (const ushort8 *)(
          (const uint16_t *)ds_tr +
          (((sq >> 2) * 8 + (k0 >> 4)) * 64 + (sq & 3) * 16 + (k0 & 15)));
      bf16x8a af = us8_to_bf8a(*ap);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
        int cq = ni * 2 + ((lane >> 4) & 1);
        bf16x8a bf = tr_frag(k_tr, 4, kq0, cq);
        dq[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, dq[ni], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int row = sq0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        dq_out[(long)row * drow + ni * 32 + (lane & 31)] = f2bf(dq[ni][r]);
    }
  }

  // dK = dSᵀ·Q and dV = Pᵀ·dO: rows are sk (wave's 32), k = sq (tr reads)
  {
    float16a dk[2] = {}, dv[2] = {};
    for (int ks = 0; ks < 8; ++ks) {
      int kq0 = ks * 4 + ((lane >> 5) & 1) * 2;
      // A fragments: lane&31 = sk row within the wave's 32-slice
      int cqa = (sq0 >> 4) + ((lane >> 4) & 1); // sk block of this wave
      bf16x8a a_ds = tr_frag(ds_tr, 8, kq0, cqa);
      bf16x8a a_p = tr_frag(p_tr, 8, kq0, cqa);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int cq = ni * 2 + ((lane >> 4) & 1);
        bf16x8a b_q = tr_frag(q_tr, 4, kq0, cq);
        bf16x8a b_do = tr_frag(do_tr, 4, kq0, cq);
        dk[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_ds, b_q, dk[ni], 0, 0, 0);
        dv[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_p, b_do, dv[ni], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int row = sq0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); // sk row
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int d = ni * 32 + (lane & 31);
        dk_out[(long)row * drow + d] = f2bf(dk[ni][r]);
        dv_out[(long)row * drow + d] = f2bf(DROP ? dv[ni][r] * rs : dv[ni][r]);
      }
    }
  }
}

extern "C" hipError_t attn_bwd_launch(const void *qkv, const void *dctx,
                                      const void *probs, void *dqkv, int B,
                                      int S, int H, float scale,
                                      hipStream_t strm) {
  if (S != 128) return hipErrorInvalidValue; // torch fallback upstream
  attn_bwd_k<false><<<B * H, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, (const uint16_t *)probs,
      (uint16_t *)dqkv, B, H, scale, 1.f);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}

// probs: the sign-coded tensor of attn_drop_fwd_launch; rs = 1/(1 - p_eff)
extern "C" hipError_t attn_drop_bwd_launch(const void *qkv, const void *dctx,
                                           const void *probs, void *dqkv,
                                           float rs, int B, int S, int H,
                                           float scale, hipStream_t strm) {
  if (S != 128) return hipErrorInvalidValue; // torch fallback upstream
  attn_bwd_k<true><<<B * H, 256, 0, strm>>>(
      (const uint16_t *)qkv, (const uint16_t *)dctx, (const uint16_t *)probs,
      (uint16_t *)dqkv, B, H, scale, rs);
  HIP_KERNEL_CHECK();
  return hipSuccess;
}
