// Mixed-staging MFMA GEMM for gfx950: C[M][N] = sum_k A(m,k)·B(n,k) where
// EITHER operand may be stored k-contiguous (NT: rows along the output dim,
// 16 B loads along k) or k-strided (TN: memory rows ARE k, 16 B loads along
// the output dim, transposed during the LDS write pass).
//
// This removes every materialized transpose / im2col in the framework:
//   conv wgrad   : dw[q][rsc] = Σ_m dy[m][q]·xcol[m][rsc]   (TN × TN-gather)
//   conv dgrad   : dx[m][c]   = Σ_k dy-gather · w[q][rs·C+c] (NT-gather × TN)
//   linear dx    : dx[m][k]   = Σ_n dy[m][n]·w[n][k]         (NT × TN)
//   linear dw    : dw[n][k]   = Σ_m dy[m][n]·x[m][k]         (TN × TN)
// (profiled before: im2col_t_k 15% + transpose2d_k 7.4% of step time —
//  both are pure data movement this file deletes.)
//
// LDS image: [128 rows][9 slots of 16 B] (pitch 144 B). The 9-slot pitch
// makes ds_read_b128 conflict-free WITHOUT an XOR swizzle: a 16-lane read
// group covers rows r..r+15 at one slot, and banks (36·row + 4·slot) mod 64
// are distinct because 36·row mod 64 has period 16. The TN write pass packs
// two k's per lane into one ds_write_b32 (its ≤2-way write conflicts are
// free: LDS-array cycles stay under the instruction's own 4).
//
// Schedule: register staging, issue-early / write-late (load tile t+1's
// global data during tile t's MFMAs, write it to LDS after them) — the
// measured-best register-staging form for this 2-barrier structure.
#pragma once
#include <atomic>
#include <cstdint>
#include <type_traits>

#include "knobs.h"
#include "launchers.h"
#include "mfma_tile.h"

constexpr int MXP = 9; // slots per LDS image row (pitch 144 B)

// ---- staging policies ----
// NT: loader.load(row, k0) -> 8 bf16 along k (row-major k-contiguous).
// TN: loader.load(k, col0) -> 8 bf16 along the output dim (k-strided).

template <class L> struct NtStage {
  static constexpr int PITCH = MXP;
  static constexpr bool GLDS = false;
  static DEV_INLINE int rslot(int slot, int) { return slot; }
  L l;
  ushort8 r[4];
  DEV_INLINE void init(int, int) {}
  DEV_INLINE void load(int tid, int base, int kb, ushort8 *) {
    int s_row = tid >> 3, s_slot = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      r[i] = l.load(base + s_row + 32 * i, kb + s_slot * 8);
  }
  DEV_INLINE void write(int tid, ushort8 *img) const {
    int s_row = tid >> 3, s_slot = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) img[(s_row + 32 * i) * MXP + s_slot] = r[i];
  }
};

// TN pair assignment: 16 consecutive lanes cover 16 consecutive column
// octets of ONE k-pair, so each wave instruction reads 4 CONTIGUOUS 256 B
// spans instead of 64 scattered 16 B lines (ablation: staging loads were
// 62% of the TN kernel). The transposed LDS write then lands 16 lanes on
// one slot column — the (row>>3)&7 slot-XOR spreads them across banks
// (matching XOR on the read side via rslot()).
template <class L> struct TnStage {
  static constexpr int PITCH = MXP;
  static constexpr bool GLDS = false;
  static DEV_INLINE int rslot(int slot, int row) {
    return slot ^ ((row >> 3) & 7);
  }
  L l;
  ushort8 r[4]; // [it][k-parity]: 2 pair-loads of 2 adjacent k each
  DEV_INLINE void init(int, int) {}
  DEV_INLINE void load(int tid, int base, int kb, ushort8 *) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      int p = tid + it * 256;  // pair index in [0,512)
      int k0 = (p >> 4) * 2;   // even k within the 64-deep tile
      int col0 = (p & 15) * 8; // 8 output-dim columns, contiguous per wave
      r[it * 2] = l.load(kb + k0, base + col0);
      r[it * 2 + 1] = l.load(kb + k0 + 1, base + col0);
    }
  }
  DEV_INLINE void write(int tid, ushort8 *img) const {
    uint32_t *img32 = (uint32_t *)img;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      int p = tid + it * 256;
      int k0 = (p >> 4) * 2;
      int col0 = (p & 15) * 8;
      int slot = k0 >> 3, within = (k0 & 7) >> 1;
      const ushort8 &va = r[it * 2], &vb = r[it * 2 + 1];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int row = col0 + j;
        img32[row * (MXP * 4) + rslot(slot, row) * 4 + within] =
            (uint32_t)va[j] | ((uint32_t)vb[j] << 16);
      }
    }
  }
};

// Plain k-contiguous operand staged by global_load_lds (direct HBM→LDS DMA,
// no staging registers, no ds_write pass — the measured +69% rung of the
// guide's ladder at this tile). glds writes wave-uniform-base + lane*16, so
// the LDS image is lane-linear (pitch 8, no pad); bank conflicts are dodged
// by pre-swizzling the SOURCE k-octet with (row&7) and XOR-ing the same on
// the read side.
struct GldsNt {
  static constexpr int PITCH = 8;
  static constexpr bool GLDS = true;
  static DEV_INLINE int rslot(int slot, int row) { return slot ^ (row & 7); }
  const uint16_t *p;
  int rows;
  long ld;
  int kdim;
  DEV_INLINE void init(int, int) {}
  DEV_INLINE void load(int tid, int base, int kb, ushort8 *img) {
    int s_row = tid >> 3, s_slot = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = base + s_row + 32 * i;
      int k = kb + (s_slot ^ (row & 7)) * 8; // pre-swizzled source octet
      if (row < rows && k < kdim) {
        auto *dst = (__attribute__((address_space(3))) ushort8 *)(img + i * 256 + tid);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void *)(p + (long)row * ld + k),
            (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
      } else {
        img[i * 256 + tid] = ushort8{0, 0, 0, 0, 0, 0, 0, 0}; // edge zero-fill
      }
    }
  }
  DEV_INLINE void write(int, ushort8 *) const {} // loads land in LDS directly
};

typedef __attribute__((ext_vector_type(16))) float float16v;

// Epilogue address map: row/col → element offset in the output. The
// default is a plain row-major matrix; Stride2Writer scatters a parity
// sub-image back into an NHWC tensor (stride-2 dgrad decomposition).
// Writer concept: RowCtx row_ctx(row) hoists the per-row address work out
// of the column loop; store_*(ptr, ctx, col, v) places one value.
//
// Vector path (optional, flagged by VEC): store_bf16x8 / store_f32x4 place 8
// already-rounded bf16 or 4 fp32 values of ONE row at a column that is a
// multiple of 8 / 4 with a single 16-byte store. The row-major epilogues of
// pipe_mix8_k and pipe256x16_gemm_k use it when the launcher finds the
// launch eligible (vec_ok() + epilogue_vec_eligible() below); writers without
// it (VEC = false) keep the one-element-per-lane epilogue.
struct LinearWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = true;
  long ldc;
  typedef long RowCtx;
  // host: every row base lands on a 16-byte boundary for group width g
  bool vec_ok(int g) const { return ldc % g == 0; }
  DEV_INLINE RowCtx row_ctx(int row) const { return (long)row * ldc; }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    p[b + col] = v;
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    p[b + col] = f2bf(v);
  }
  DEV_INLINE void store_f32x4(float *p, RowCtx b, int col, float4v v) const {
    *(float4v *)(p + b + col) = v;
  }
  DEV_INLINE void store_bf16x8(uint16_t *p, RowCtx b, int col, ushort8 v) const {
    *(ushort8 *)(p + b + col) = v;
  }
};

// linear forward with the bias folded into the epilogue (fp32 bias, the
// separate bias_add pass was a full activation read+write — 2.4% of a
// BERT-Large step).
struct BiasWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = false;
  long ldc;
  const float *bias;
  typedef long RowCtx;
  DEV_INLINE RowCtx row_ctx(int row) const { return (long)row * ldc; }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    p[b + col] = v + bias[col];
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    p[b + col] = f2bf(v + bias[col]);
  }
};

// tanh-approx GELU (BERT's activation) and its derivative, fp32.
// tanh via one hardware exp (v_exp_f32): libm tanhf costs ~10× as many
// VALU ops and dominated the fused-GELU GEMM epilogues (113 vs 58 µs on
// the fc2-dx kernel). |rel err| ~1e-7 — far below bf16 output rounding.
DEV_INLINE float tanh_fast(float u) {
  float a = __expf(-2.f * fabsf(u));
  float t = (1.f - a) / (1.f + a);
  return u < 0.f ? -t : t;
}
DEV_INLINE float gelu_f(float x) {
  float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  return 0.5f * x * (1.f + tanh_fast(u));
}
DEV_INLINE float dgelu_f(float x) {
  float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  float t = tanh_fast(u);
  return 0.5f * (1.f + t) +
         0.5f * x * (1.f - t * t) * 0.7978845608028654f *
             (1.f + 3.f * 0.044715f * x * x);
}
// gelu and its derivative off ONE tanh evaluation (forward epilogue saves
// the derivative so the backward epilogue is exp-free — recomputing
// gelu'(h) there cost ~27 us of v_exp per fc2-dx GEMM, 16.7M elements at
// the transcendental issue rate, serialized after the MFMA work)
DEV_INLINE float gelu_pair_f(float x, float &dg) {
  float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  float t = tanh_fast(u);
  dg = 0.5f * (1.f + t) +
       0.5f * x * (1.f - t * t) * 0.7978845608028654f *
           (1.f + 3.f * 0.044715f * x * x);
  return 0.5f * x * (1.f + t);
}

// FFN fc1 epilogue: writes BOTH the pre-activation h = xW₁ᵀ+b (saved for
// backward) and g = gelu(h) — the separate torch GELU pass re-read the
// whole intermediate activation (BERT-Large: 32 MB/layer at 8 TB/s).
struct GeluBiasWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = false;
  long ldc;
  const float *bias;
  uint16_t *deriv; // gelu'(h), bf16, same layout as C (saved for backward)
  typedef long RowCtx;
  DEV_INLINE RowCtx row_ctx(int row) const { return (long)row * ldc; }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    float h = v + bias[col], dg;
    p[b + col] = gelu_pair_f(h, dg);
    deriv[b + col] = f2bf(dg);
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    float h = v + bias[col], dg;
    p[b + col] = f2bf(gelu_pair_f(h, dg));
    deriv[b + col] = f2bf(dg);
  }
};

// FFN backward epilogue: the fc2-dx GEMM produces dg; multiplying by
// gelu'(h) here yields dh directly — kills the separate dgelu pass
// (2 reads + 1 write over the intermediate activation per layer).
struct GeluBwdWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = false;
  long ldc;
  const uint16_t *deriv; // gelu'(h) saved by GeluBiasWriter — exp-free
  typedef long RowCtx;
  DEV_INLINE RowCtx row_ctx(int row) const { return (long)row * ldc; }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    p[b + col] = v * bf2f(deriv[b + col]);
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    p[b + col] = f2bf(v * bf2f(deriv[b + col]));
  }
};

// legacy pair (MPIAMD_GELU_DERIV=0): forward saves the PRE-ACTIVATION and
// backward recomputes gelu' (one tanh per element in the bwd epilogue)
struct GeluBiasPreWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = false;
  long ldc;
  const float *bias;
  uint16_t *pre; // h (pre-activation), bf16
  typedef long RowCtx;
  DEV_INLINE RowCtx row_ctx(int row) const { return (long)row * ldc; }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    float h = v + bias[col];
    pre[b + col] = f2bf(h);
    p[b + col] = gelu_f(h);
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    float h = v + bias[col];
    pre[b + col] = f2bf(h);
    p[b + col] = f2bf(gelu_f(h));
  }
};

struct GeluBwdPreWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = false;
  long ldc;
  const uint16_t *pre;
  typedef long RowCtx;
  DEV_INLINE RowCtx row_ctx(int row) const { return (long)row * ldc; }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    p[b + col] = v * dgelu_f(bf2f(pre[b + col]));
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    p[b + col] = f2bf(v * dgelu_f(bf2f(pre[b + col])));
  }
};

// Conv-forward epilogue that ALSO produces the BatchNorm per-channel
// partial statistics (Σy, Σy²) — removes bn_partials' full re-read of the
// activation it just wrote (~9% of a ResNet step at 8 TB/s).
//
// Deterministic, atomic-free: the slab has one entry per 64 OUTPUT ROWS
// ([ceil(M/64)][2][C], allocated UNINITIALIZED by the host: every band has
// at least one valid row and its first row belongs to a lane < 32, so each
// (band, channel < C) entry the finalize reads is written — ragged last
// band and ragged last column tile included). In every tile kernel here
// (mix/pipe_mix 2×2 waves, pipe_mix8 2×4 waves, pipe256) a lane's epilogue
// rows all fall in ONE 64-row band per m-frag half, and a (band, channel)
// pair is written by exactly one lane pair (l, l^32) — combined with one
// shfl, stored plain. Stats use the ROUNDED bf16 value (what bn_partials
// would read).
//
// Accumulators are addressed by a SLOT the kernel names with its unrolled
// loop indices — slot(band, colslot), both compile-time constants after
// unrolling — never by values derived from row/col: runtime-indexed
// accumulator arrays went to scratch memory (80 B/lane, one scratch
// read-modify-write per stored element; the 256² kernel ran 48 vs 18 us).
// band: which of the lane's (at most two) 64-row bands the m-frag is in;
// colslot: which of the lane's (at most two) columns.
struct BnStatsWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = true;
  static constexpr bool VEC = false;
  long ldc;
  float *slab; // [ceil(M/64)][2][C]
  int C;
  // mutable per-lane accumulators: [band slot][col slot]
  mutable float s0[2][2], s1[2][2];
  mutable int tm[2], colc[2];
  mutable int h_, c_, band_;
  typedef long RowCtx;
  DEV_INLINE void reset() const {
    s0[0][0] = s0[0][1] = s0[1][0] = s0[1][1] = 0.f;
    s1[0][0] = s1[0][1] = s1[1][0] = s1[1][1] = 0.f;
    tm[0] = tm[1] = -1;
    colc[0] = colc[1] = -1;
    h_ = c_ = 0;
    band_ = -1;
  }
  DEV_INLINE void slot(int band, int colslot) const {
    h_ = band;
    c_ = colslot;
  }
  DEV_INLINE RowCtx row_ctx(int row) const {
    band_ = row >> 6;
    return (long)row * ldc;
  }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    p[b + col] = v; // split-K callers never attach stats (caller contract)
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    uint16_t r = f2bf(v);
    p[b + col] = r;
    float vr = bf2f(r);
    tm[h_] = band_;
    colc[c_] = col;
    s0[h_][c_] += vr;
    s1[h_][c_] += vr * vr;
  }
  DEV_INLINE void flush(int lane) const {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // bands are per-(lane-half) identical; tm/col agree across l, l^32
      // wherever both lanes stored (the lane < 32 owns the band's first row)
#pragma unroll
      for (int ci = 0; ci < 2; ++ci) {
        float a = s0[h][ci] + __shfl_xor(s0[h][ci], 32, 64);
        float b = s1[h][ci] + __shfl_xor(s1[h][ci], 32, 64);
        if (lane < 32 && tm[h] >= 0 && colc[ci] >= 0) {
          float *e = slab + (long)tm[h] * 2 * C;
          e[colc[ci]] = a;
          e[C + colc[ci]] = b;
        }
      }
    }
  }
};

// += into an existing bf16 tensor (bottleneck backward: conv1's dgrad
// accumulates onto the skip-connection gradient — no separate add pass).
struct LinearAccWriter {
  static constexpr bool ACC = true;
  static constexpr bool STATS = false;
  static constexpr bool VEC = true; // acc_bf16x8 takes fp32, not rounded bf16
  long ldc;
  typedef long RowCtx;
  bool vec_ok(int g) const { return ldc % g == 0; }
  DEV_INLINE void store_f32x4(float *p, RowCtx b, int col, float4v v) const {
    float4v o = *(const float4v *)(p + b + col);
    *(float4v *)(p + b + col) = o + v;
  }
  // 16-byte read-modify-write: the sum is formed in fp32 from the UNROUNDED
  // accumulator and rounded once, exactly as store_bf16 does per element
  DEV_INLINE void acc_bf16x8(uint16_t *p, RowCtx b, int col, float4v lo,
                             float4v hi) const {
    ushort8 o = *(const ushort8 *)(p + b + col), r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[j] = f2bf(lo[j] + bf2f(o[j]));
      r[4 + j] = f2bf(hi[j] + bf2f(o[4 + j]));
    }
    *(ushort8 *)(p + b + col) = r;
  }
  DEV_INLINE RowCtx row_ctx(int row) const { return (long)row * ldc; }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    p[b + col] += v;
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    p[b + col] = f2bf(v + bf2f(p[b + col]));
  }
};

struct Stride2Writer {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = true;
  int W2, H2, ph, pw, W, H, C;
  typedef long RowCtx;
  bool vec_ok(int g) const { return C % g == 0; } // pixel bases are k*C
  DEV_INLINE RowCtx row_ctx(int row) const {
    int w_ = row % W2;
    long t = row / W2;
    int h_ = (int)(t % H2);
    int n = (int)(t / H2);
    return (((long)n * H + 2 * h_ + ph) * W + 2 * w_ + pw) * (long)C;
  }
  DEV_INLINE void store_f32(float *p, RowCtx b, int col, float v) const {
    p[b + col] = v;
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx b, int col, float v) const {
    p[b + col] = f2bf(v);
  }
  DEV_INLINE void store_f32x4(float *p, RowCtx b, int col, float4v v) const {
    *(float4v *)(p + b + col) = v;
  }
  DEV_INLINE void store_bf16x8(uint16_t *p, RowCtx b, int col, ushort8 v) const {
    *(ushort8 *)(p + b + col) = v;
  }
};

// 1x1 stride-2 dgrad: parity (pad%2, pad%2) is the ONLY contributor, so the
// epilogue zeroes the three sibling pixels itself — no 100 MB memset pass.
struct Stride2ZeroWriter {
  static constexpr bool ACC = false;
  static constexpr bool STATS = false;
  static constexpr bool VEC = true;
  int W2, H2, ph, pw, W, H, C;
  bool vec_ok(int g) const { return C % g == 0; }
  struct RowCtx {
    long base;
    int sib; // bit0: w+1 valid, bit1: h+1 valid
  };
  DEV_INLINE RowCtx row_ctx(int row) const {
    int w_ = row % W2;
    long t = row / W2;
    int h_ = (int)(t % H2);
    int n = (int)(t / H2);
    int hh = 2 * h_ + ph, ww = 2 * w_ + pw;
    RowCtx c;
    c.base = (((long)n * H + hh) * W + ww) * (long)C;
    c.sib = (ww + 1 < W ? 1 : 0) | (hh + 1 < H ? 2 : 0);
    return c;
  }
  DEV_INLINE void store_f32(float *p, RowCtx c, int col, float v) const {
    p[c.base + col] = v; // (f32 split-K path never uses ZSIB)
  }
  DEV_INLINE void store_bf16(uint16_t *p, RowCtx c, int col, float v) const {
    p[c.base + col] = f2bf(v);
    if (c.sib & 1) p[c.base + C + col] = 0;
    if (c.sib & 2) {
      p[c.base + (long)W * C + col] = 0;
      if (c.sib & 1) p[c.base + (long)W * C + C + col] = 0;
    }
  }
  DEV_INLINE void store_f32x4(float *p, RowCtx c, int col, float4v v) const {
    *(float4v *)(p + c.base + col) = v;
  }
  DEV_INLINE void store_bf16x8(uint16_t *p, RowCtx c, int col, ushort8 v) const {
    const ushort8 z{0, 0, 0, 0, 0, 0, 0, 0};
    *(ushort8 *)(p + c.base + col) = v;
    if (c.sib & 1) *(ushort8 *)(p + c.base + C + col) = z;
    if (c.sib & 2) {
      *(ushort8 *)(p + c.base + (long)W * C + col) = z;
      if (c.sib & 1) *(ushort8 *)(p + c.base + (long)W * C + C + col) = z;
    }
  }
};

// ---- row-major (16-byte store) epilogue --------------------------------
// Process-wide switch, set through the extension's set_epilogue_vec(); the
// launchers read it per launch. One object for every translation unit of
// the library (C++17 inline variable).
inline std::atomic<bool> g_epilogue_vec{true};

// Per-launch eligibility of the 16-byte store path: whole column groups
// (N % g), 16-byte aligned output pointer, row bases (the writer's vec_ok)
// and split-K slab stride. g = 4 for fp32, 8 for bf16.
template <class WR>
static inline bool epilogue_vec_eligible(const WR &wrt, const void *c, int N,
                                         bool c_f32, int splits,
                                         long split_stride) {
  if constexpr (!WR::VEC) {
    return false;
  } else {
    const int g = c_f32 ? 4 : 8;
    return g_epilogue_vec.load(std::memory_order_relaxed) && N % g == 0 &&
           ((uintptr_t)c & 15) == 0 && wrt.vec_ok(g) &&
           (splits <= 1 || split_stride % g == 0);
  }
}

typedef float __attribute__((may_alias)) f32_alias;
typedef uint16_t __attribute__((may_alias)) u16_alias;
typedef float4v __attribute__((may_alias)) float4v_alias;
typedef ushort8 __attribute__((may_alias)) ushort8_alias;

// One 32-row band of a wave's accumulators, NF 32x32 fragments side by
// side (32·NF columns), through a WAVE-PRIVATE LDS region of 4·NF KiB:
// the MFMA C/D map (lane = column, 16 regs = rows) is written row-major
// (unpadded pitch: the b32/b16 writes of 32 consecutive columns and the
// b128 reads below are bank-conflict-free for the ds_read_b128 lane
// groups), read back as 16-byte row segments and stored through the
// writer's vector path. bf16 rounds per element BEFORE staging (same f2bf
// as the scalar path). Only wave-local ordering is needed — LDS operations
// of one wave execute in order — so no s_barrier in here; the caller
// barriers ONCE before the first band, when other waves may still be
// reading the operand images this region overlays.
template <int NF, bool C_F32, class WR>
DEV_INLINE void vec_epilogue_band(const WR &wrt, void *cptr, void *wave_lds,
                                  const float16v *a, int lane, int row_base,
                                  int col_base, int M, int N) {
  constexpr int PITCH = NF * 32; // elements per staged row
  const int lc = lane & 31, lr = 4 * (lane >> 5);
  if constexpr (WR::ACC && !C_F32) {
    // accumulating writer: stage fp32 (the old value joins before rounding)
    f32_alias *w = (f32_alias *)wave_lds;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        w[((r & 3) + 8 * (r >> 2) + lr) * PITCH + f * 32 + lc] = a[f][r];
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    constexpr int LPR = NF * 4, RPP = 64 / LPR;
    const int rl0 = lane / LPR, cg = (lane % LPR) * 8;
#pragma unroll
    for (int p = 0; p < 32 / RPP; ++p) {
      int rl = p * RPP + rl0;
      float4v lo = *(const float4v_alias *)(w + rl * PITCH + cg);
      float4v hi = *(const float4v_alias *)(w + rl * PITCH + cg + 4);
      int row = row_base + rl, col = col_base + cg;
      if (row < M && col < N)
        wrt.acc_bf16x8((uint16_t *)cptr, wrt.row_ctx(row), col, lo, hi);
    }
  } else if constexpr (C_F32) {
    f32_alias *w = (f32_alias *)wave_lds;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        w[((r & 3) + 8 * (r >> 2) + lr) * PITCH + f * 32 + lc] = a[f][r];
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    constexpr int LPR = NF * 8, RPP = 64 / LPR; // lanes per row, rows per pass
    const int rl0 = lane / LPR, cg = (lane % LPR) * 4;
#pragma unroll
    for (int p = 0; p < 32 / RPP; ++p) {
      int rl = p * RPP + rl0;
      float4v v = *(const float4v_alias *)(w + rl * PITCH + cg);
      int row = row_base + rl, col = col_base + cg;
      if (row < M && col < N)
        wrt.store_f32x4((float *)cptr, wrt.row_ctx(row), col, v);
    }
  } else {
    u16_alias *w = (u16_alias *)wave_lds;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        w[((r & 3) + 8 * (r >> 2) + lr) * PITCH + f * 32 + lc] = f2bf(a[f][r]);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    constexpr int LPR = NF * 4, RPP = 64 / LPR;
    const int rl0 = lane / LPR, cg = (lane % LPR) * 8;
#pragma unroll
    for (int p = 0; p < 32 / RPP; ++p) {
      int rl = p * RPP + rl0;
      ushort8 v = *(const ushort8_alias *)(w + rl * PITCH + cg);
      int row = row_base + rl, col = col_base + cg;
      if (row < M && col < N)
        wrt.store_bf16x8((uint16_t *)cptr, wrt.row_ctx(row), col, v);
    }
  }
  // the next band overwrites this region: keep its writes behind the reads
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// ONEBUF: single LDS buffer (36 KB vs 72 KB) with a second barrier per
// k-step — 4 workgroups/CU instead of 2 (16 waves/CU): trades one barrier
// for 2x the latency-hiding wave pool. A/B via MPIAMD_GEMM_ONEBUF=0/1.
template <class SA, class SB, bool C_F32, class WR = LinearWriter,
          bool ONEBUF = false>
__global__ __launch_bounds__(NT_THREADS) void mix_gemm_k(
    SA sa, SB sb, void *__restrict__ cptr, int M, int N, int K, WR wrt,
    int tiles_n, int kt_per_split, long split_stride, int xcd_cpx, int swap) {
  // SPLIT-MAJOR grid (x = split, y = tile) when swap: the N-tiles sharing
  // an A panel are y-adjacent, which lands them on ONE XCD's L2 when
  // gridDim.x%8==0. Tile-major dispatch spread a panel's sharers over 4+
  // XCDs and the panel re-reads all went to HBM (ablation: staging at full
  // HBM BW; +16-28% on split-K wgrad shapes in the standalone A/B).
  int tile = swap ? blockIdx.y : blockIdx.x;
  int split = swap ? blockIdx.x : blockIdx.y;
  if (xcd_cpx) // T1: contiguous tile chunk per XCD (L2 reuse of panels)
    tile = (tile & 7) * xcd_cpx + (tile >> 3);
  int tm = tile / tiles_n, tn = tile % tiles_n;
  int row0 = tm * BM, col0 = tn * BN;
  int tid = threadIdx.x;
  int lane = tid & 63, wave = tid >> 6;
  int wr = wave >> 1, wc = wave & 1;

  // ONE shared object (a second __shared__ array makes hipcc drain vmcnt(0)
  // before every ds_read while a glds is in flight — guide §5 trap 4a)
  constexpr int ASZ = BM * SA::PITCH, BSZ = BM * SB::PITCH;
  constexpr int NBUF = ONEBUF ? 1 : 2;
  __shared__ ushort8 lds[NBUF * (ASZ + BSZ)];
  // NOTE: compute image bases arithmetically at each use — a runtime-indexed
  // private array of LDS pointers de-optimizes every ds_read (measured -15%
  // across ALL kernels when these were ushort8* imgA[2] arrays)
#define MXG_A(b) (lds + ((b) % NBUF) * (ASZ + BSZ))
#define MXG_B(b) (lds + ((b) % NBUF) * (ASZ + BSZ) + ASZ)

  // 32x32x16 MFMA (higher ceiling than 16x16x32): each wave computes a
  // 64x64 quadrant as 2x2 fragments of 32x32, 16 fp32 accumulators each.
  float16v acc[2][2] = {};

  int nk_total = (K + BK - 1) / BK;
  int t0 = split * kt_per_split;
  int nk = min(kt_per_split, nk_total - t0);
  if (nk < 0) nk = 0;

  // Register staging, issue-early / write-late (distance-1). A distance-2
  // two-register-set variant was measured SLOWER on the gather stagers
  // (address-compute duplication outweighed the extra latency cover) and
  // neutral on plain ones — don't re-add it.
  sa.init(tid, row0);
  sb.init(tid, col0);
  if (nk > 0) {
    sa.load(tid, row0, t0 * BK, MXG_A(0));
    sb.load(tid, col0, t0 * BK, MXG_B(0));
    sa.write(tid, MXG_A(0));
    sb.write(tid, MXG_B(0));
  }
  __syncthreads();

  for (int t = 0; t < nk; ++t) {
    int buf = ONEBUF ? 0 : (t & 1);
    if (t + 1 < nk) { // issue-early: loads (or glds DMA) land under MFMAs
      sa.load(tid, row0, (t0 + t + 1) * BK, MXG_A(buf ^ 1));
      sb.load(tid, col0, (t0 + t + 1) * BK, MXG_B(buf ^ 1));
    }
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) { // 4 k-steps of 16
      bf16x8 af[2], bf_[2];
      // lane l: row = l&31, k = kk*16 + (l>>5)*8 .. +7 → slot kk*2+(l>>5)
      int slot = kk * 2 + (lane >> 5);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        int arow = wr * 64 + mi * 32 + (lane & 31);
        af[mi] = us8_to_bf8v(MXG_A(buf)[arow * SA::PITCH + SA::rslot(slot, arow)]);
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int brow = wc * 64 + ni * 32 + (lane & 31);
        bf_[ni] = us8_to_bf8v(MXG_B(buf)[brow * SB::PITCH + SB::rslot(slot, brow)]);
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              af[mi], bf_[ni], acc[mi][ni], 0, 0, 0);
    }
    if (ONEBUF) {
      if (t + 1 < nk) { // reuse the single buffer: drain-readers barrier,
        __syncthreads(); // then overwrite with tile t+1
        sa.write(tid, MXG_A(0));
        sb.write(tid, MXG_B(0));
      }
    } else if (t + 1 < nk) { // write-late into the other buffer
      sa.write(tid, MXG_A(buf ^ 1));
      sb.write(tid, MXG_B(buf ^ 1));
    }
    __syncthreads();
  }

  // 32x32 C/D map: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  // Row-major loop order so each row's address context is computed once.
  if constexpr (WR::STATS) wrt.reset();
  cptr = (void *)((char *)cptr + split * split_stride * (C_F32 ? 4 : 2));
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int row = row0 + wr * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= M) continue;
      typename WR::RowCtx rc = wrt.row_ctx(row);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int col = col0 + wc * 64 + ni * 32 + (lane & 31);
        if (col >= N) continue;
        if constexpr (WR::STATS) wrt.slot(0, ni); // both m-frags: one band
        if (C_F32)
          wrt.store_f32((float *)cptr, rc, col, acc[mi][ni][r]);
        else
          wrt.store_bf16((uint16_t *)cptr, rc, col, acc[mi][ni][r]);
      }
    }
  }
  if constexpr (WR::STATS) wrt.flush(lane);
}

#undef MXG_A
#undef MXG_B

// ---- launch geometry shared by every split-K tile launcher ----------------

// Split count a launch really runs: at most one split per `bk`-deep k-tile.
// A caller that reduces the slabs afterwards clamps with the same function,
// so it sums exactly the slabs the GEMM wrote.
static inline int clamp_splits(int splits, long K, int bk) {
  long nk = (K + bk - 1) / bk;
  return splits > nk ? (nk > 0 ? (int)nk : 1) : splits;
}

// Grid of a `tile`²-tile, `bk`-deep GEMM run in `splits` split-K slices
// (mix_gemm_k, pipe_mix_k, pipe_mix8_k).
struct TileGeom {
  int tiles_n, splits, kts, nwg;
  long split_stride; // elements between the fp32 slabs of two splits
  TileGeom(int M, int N, int K, long ldc, int splits_in, int tile, int bk)
      : tiles_n((N + tile - 1) / tile), splits(clamp_splits(splits_in, K, bk)),
        kts(((K + bk - 1) / bk + splits - 1) / splits),
        nwg(((M + tile - 1) / tile) * tiles_n), split_stride((long)M * ldc) {}
  // T1 XCD swizzle: give each XCD a contiguous chunk of tiles so neighbor
  // tiles (sharing operand panels) hit the same per-XCD L2. Needs nwg%8==0
  // and enough tiles to matter; under split-K only where the launcher says
  // so (`fold_sk`).
  int cpx(bool fold_sk) const {
    return (nwg % 8 == 0 && nwg >= 32 && (splits == 1 || fold_sk)) ? nwg / 8
                                                                    : 0;
  }
};

// f(std::true_type{}) or f(std::false_type{}): turns a runtime flag into a
// kernel template argument with ONE launch statement in f instead of one
// per value.
template <class F> static inline void with_bool(bool b, F &&f) {
  if (b)
    f(std::true_type{});
  else
    f(std::false_type{});
}

template <class SA, class SB, class WR>
static hipError_t launch_mix_gemm_wr(const SA &sa, const SB &sb, void *c,
                                     int M, int N, int K, const WR &wrt,
                                     long ldc, bool c_f32, hipStream_t s,
                                     int splits = 1) {
  const TileGeom g(M, N, K, ldc, splits, BM, BK);
  int swap = (g.splits > 1 && g.splits % 8 == 0 && use_splitmajor()) ? 1 : 0;
  int cpx = g.cpx(swap);
  dim3 grid = swap ? dim3(g.splits, g.nwg) : dim3(g.nwg, g.splits);
  // glds targets the next buffer while the current one is being read — a
  // single buffer would race
  const bool onebuf = use_onebuf() && !SA::GLDS && !SB::GLDS;
  with_bool(c_f32, [&](auto f32) {
    with_bool(onebuf, [&](auto ob) {
      mix_gemm_k<SA, SB, decltype(f32)::value, WR, decltype(ob)::value>
          <<<grid, NT_THREADS, 0, s>>>(sa, sb, c, M, N, K, wrt, g.tiles_n,
                                       g.kts, g.split_stride, cpx, swap);
    });
  });
  return hipGetLastError();
}

template <class SA, class SB>
static hipError_t launch_mix_gemm(const SA &sa, const SB &sb, void *c, int M,
                                  int N, int K, long ldc, bool c_f32,
                                  hipStream_t s, int splits = 1) {
  return launch_mix_gemm_wr(sa, sb, c, M, N, K, LinearWriter{ldc}, ldc, c_f32,
                            s, splits);
}

#include "gemm256.h"
#include "pipe256.h"
#include "pipe_mix.h"

// Plain NT×NT entry (both operands k-contiguous row-major). glds staging
// vs register staging selectable for same-box A/B (MPIAMD_GLDS=0 reverts).
// Full-tile shapes take the 256²-tile counted-vmcnt pipeline (gemm256.h);
// MPIAMD_GEMM256=0 reverts those to the mix_gemm path.
// Route choice of the plain NT×NT entry, factored out so the BN-stats conv
// forward (conv.hip conv_fwd_bn) runs exactly the kernel the unfused conv
// runs for the same shape and environment.
enum NtRoute { NT_PIPE256, NT_256, NT_PIPEMIX, NT_GLDS, NT_REG };

static inline NtRoute nt_gemm_route(int M, int N, int K, long ldc, int kdim_a,
                                    int kdim_b, int splits) {
  // occupancy floor: 256² tiles run 1 block/CU (96 KB LDS), so a grid
  // under ~half the 256 CUs loses more to idle CUs than the pipeline wins
  // (measured: M=12544,N=512 → 98 wgs: 338 vs 506 TF on the 128² path;
  // M=50176,N=256 → 196 wgs: 505 vs 417 — the crossover is between)
  if (use_gemm256() && splits <= 1 && M % 256 == 0 && N % 256 == 0 &&
      K % 32 == 0 && K > 0 && kdim_a == K && kdim_b == K && ldc == N &&
      (long)(M / 256) * (N / 256) >= 128)
    return (use_pipe() && K % 64 == 0) ? NT_PIPE256 : NT_256;
  // non-full-tile / small-grid shapes: the 128²-tile deep pipeline
  // (pipe_mix.h) — ragged edges handled by its zeros-page staging.
  if (use_pipemix() && use_pipent()) return NT_PIPEMIX;
  return use_glds() ? NT_GLDS : NT_REG;
}

template <class LA, class LB>
static hipError_t launch_nt_gemm(const LA &la, const LB &lb, void *c, int M,
                                 int N, int K, long ldc, bool c_f32,
                                 hipStream_t s, int splits = 1,
                                 const float *bias = nullptr) {
  switch (nt_gemm_route(M, N, K, ldc, la.kdim, lb.kdim, splits)) {
  case NT_PIPE256:
    return launch_pipe256(la, lb, c, M, N, K, ldc, c_f32, s, bias);
  case NT_256:
    return launch_nt256(la, lb, c, M, N, K, ldc, c_f32, s, bias);
  case NT_PIPEMIX: {
    NtPipe<PlainNtSrc> ga{{la.p, la.ld, la.rows, la.kdim}};
    NtPipe<PlainNtSrc> gb{{lb.p, lb.ld, lb.rows, lb.kdim}};
    if (bias)
      return launch_pipe_mix_wr(ga, gb, c, M, N, K, BiasWriter{ldc, bias},
                                ldc, c_f32, s, splits);
    return launch_pipe_mix_wr(ga, gb, c, M, N, K, LinearWriter{ldc}, ldc,
                              c_f32, s, splits);
  }
  case NT_GLDS: {
    GldsNt ga{la.p, la.rows, la.ld, la.kdim};
    GldsNt gb{lb.p, lb.rows, lb.ld, lb.kdim};
    if (bias)
      return launch_mix_gemm_wr(ga, gb, c, M, N, K, BiasWriter{ldc, bias},
                                ldc, c_f32, s, splits);
    return launch_mix_gemm(ga, gb, c, M, N, K, ldc, c_f32, s, splits);
  }
  default:
    break;
  }
  if (bias)
    return launch_mix_gemm_wr(NtStage<LA>{la}, NtStage<LB>{lb}, c, M, N, K,
                              BiasWriter{ldc, bias}, ldc, c_f32, s, splits);
  return launch_mix_gemm(NtStage<LA>{la}, NtStage<LB>{lb}, c, M, N, K, ldc,
                         c_f32, s, splits);
}

// ---- TN loaders ----

// k-strided view of a row-major [K][cols] matrix (dy, x, w as TN operand).
struct TnRowMajor {
  const uint16_t *p;
  long ld;  // elements per k-row
  int kdim; // rows (= reduce extent)
  int cols;
  DEV_INLINE ushort8 load(int k, int c0) const {
    if (k >= kdim || c0 >= cols) return ushort8{0, 0, 0, 0, 0, 0, 0, 0};
    if (c0 + 8 <= cols) return *(const ushort8 *)(p + (long)k * ld + c0);
    ushort8 v{0, 0, 0, 0, 0, 0, 0, 0}; // ragged tail (cols not %8)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (c0 + j < cols) v[j] = p[(long)k * ld + c0 + j];
    return v;
  }
};

// ---- k-strided (TN) operand routes ----
// One rule for every GEMM with a plain TN operand: the deep pipeline
// (pipe_mix.h) when `pipe_ok`, else the register-staged mix tile. The pipe
// stages TN operands in 16-B column granules, so each caller passes its own
// predicate — use_pipemix() and whatever makes its operands readable that
// way (gemm.hip tn_cols_ok).

// C[M][N] (+)= A[M][K-contiguous] · B(k-strided [K rows][N cols])
template <class WR>
static hipError_t launch_nt_tn_gemm(bool pipe_ok, const void *a, const void *b,
                                    void *c, int M, int N, int K, long lda,
                                    long ldb, const WR &wrt, long ldc,
                                    bool c_f32, hipStream_t s, int splits = 1) {
  if (pipe_ok) {
    NtPipe<PlainNtSrc> sa{{(const uint16_t *)a, lda, M, K}};
    TnPipe<PlainTnSrc> sb{{(const uint16_t *)b, ldb, K, N}};
    return launch_pipe_mix_wr(sa, sb, c, M, N, K, wrt, ldc, c_f32, s, splits);
  }
  GemmLoader la{(const uint16_t *)a, M, lda, K};
  TnRowMajor lb{(const uint16_t *)b, ldb, K, N};
  return launch_mix_gemm_wr(NtStage<GemmLoader>{la}, TnStage<TnRowMajor>{lb},
                            c, M, N, K, wrt, ldc, c_f32, s, splits);
}

// C[M][N] = Σ_k A(k-strided [K rows][M cols]) · B(k-strided [K rows][N cols])
template <class WR>
static hipError_t launch_tn_tn_gemm(bool pipe_ok, const void *a, const void *b,
                                    void *c, int M, int N, int K, long lda,
                                    long ldb, const WR &wrt, long ldc,
                                    bool c_f32, hipStream_t s, int splits = 1) {
  if (pipe_ok) {
    TnPipe<PlainTnSrc> sa{{(const uint16_t *)a, lda, K, M}};
    TnPipe<PlainTnSrc> sb{{(const uint16_t *)b, ldb, K, N}};
    return launch_pipe_mix_wr(sa, sb, c, M, N, K, wrt, ldc, c_f32, s, splits);
  }
  TnRowMajor la{(const uint16_t *)a, lda, K, M};
  TnRowMajor lb{(const uint16_t *)b, ldb, K, N};
  return launch_mix_gemm_wr(TnStage<TnRowMajor>{la}, TnStage<TnRowMajor>{lb},
                            c, M, N, K, wrt, ldc, c_f32, s, splits);
}

// Split-K tail: gemm(out, c_f32, splits) launches the GEMM. splits <= 1
// writes C directly (fp32 iff !out_bf16); otherwise the GEMM fills the fp32
// slabs in `partial` ([splits][len]) and splitk_reduce sums them into C.
template <class GEMM>
static hipError_t launch_splitk(GEMM gemm, float *partial, void *c, long len,
                                int splits, int out_bf16, hipStream_t s) {
  if (splits <= 1) return gemm(c, out_bf16 == 0, 1);
  hipError_t e = gemm((void *)partial, true, splits);
  if (e != hipSuccess) return e;
  return splitk_reduce(partial, splits, len, c, out_bf16, s);
}
