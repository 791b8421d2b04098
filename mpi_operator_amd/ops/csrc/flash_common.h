// What flash_attention.hip (head_dim 64) and flash_attention_d128.hip share:
// the fragment types, the C-layout row map, the [4 k][16 col] subtile image
// and its transpose read, and the packed-batch (VARLEN) sequence lookup.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8a;
typedef __attribute__((ext_vector_type(16))) float float16a;
typedef __attribute__((ext_vector_type(2))) unsigned int uint2a;

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

// row of C-layout register r (32x32 MFMA result) within the wave's 32 rows
DEV_INLINE int fa_crow(int r, int lane) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// u16 offset of element (row, col) in a [4 row][16 col] subtile image of a
// 128-row × 128-col tile (8 column blocks per row block)
DEV_INLINE int fa_sub128(int row, int col) {
  return ((row >> 2) * 8 + (col >> 4)) * 64 + (row & 3) * 16 + (col & 15);
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
