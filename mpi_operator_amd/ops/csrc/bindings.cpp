// PyTorch bindings for the gfx950 kernels. The only TU that includes torch
// headers — kernel TUs are pure HIP and are reached through the extern "C"
// launchers of launchers.h, the one declaration both sides compile against.
// The MPIAMD_* knobs are the inline functions of knobs.h: route_info() and
// the split heuristics here call the same functions the launchers call.
#include <torch/extension.h>

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

#include <vector>

#include "knobs.h"
#include "launchers.h"
#include "philox.h"

namespace {

using at::Tensor;

// Late-stage convs produce few 128x128 output tiles (7x7 spatial ~100
// blocks on 256 CUs): split the reduce dim so fwd/dgrad fill the chip,
// paying one fp32 slab + reduce pass. knobs.h conv_splits_force()
// (MPIAMD_CONV_SPLITS) overrides the heuristic.
int conv_splits(long M, int Ncols, int K) {
  const int force = conv_splits_force();
  if (force >= 1) return force;
  long tiles = ((M + 127) / 128) * ((Ncols + 127) / 128);
  int nk = (K + 63) / 64;
  if (tiles >= 256 || nk < 16) return 1;
  long s = 512 / tiles;
  if (s > nk / 8) s = nk / 8;
  if (s > 16) s = 16;
  return s < 1 ? 1 : (int)s;
}

// split count of the implicit wgrad (reduce dim = output pixels M):
// fill the chip (tiles×splits ≈ budget blocks = 2 WG/CU) but keep ≥8 k-tiles
// per split so each block amortizes its pipeline prologue; a flat 1024
// cap overshot mid shapes (b2 1x1 dw: 256 splits of nk=3 ran at 94 TF
// vs 167 at 64 splits). The target-block budget was tuned on the 4-wave
// pipeline (2 WG/CU); the 8-wave kernel fills at half the workgroups —
// MPIAMD_WGRAD_BUDGET overrides for A/B (default 512)
int wgrad_splits(int Kout, int RSC, long M) {
  int tiles = ((Kout + 127) / 128) * ((RSC + 127) / 128);
  int nk = (int)((M + 63) / 64);
  int splits = std::max(wgrad_budget() / tiles, 1);
  splits = std::min(splits, std::max(nk / 8, 1));
  splits = std::min(splits, 256);
  // multiple of 8 so the split-major grid keeps a panel's N-tile sharers
  // on one XCD ((split + splits*tile) % 8 must not walk with tile)
  if (splits >= 8) splits &= ~7;
  return splits;
}

#define CHK(call)                                                              \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    TORCH_CHECK(e_ == hipSuccess, "HIP kernel failure: ", hipGetErrorString(e_)); \
  } while (0)

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}
using HIPDeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_cl_bf16(const Tensor &t, const char *name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast),
              name, " must be 4-D channels_last");
}

// The streaming NHWC kernels walk 16 B octets of 8 channels with pitch C/8:
// a C that is no multiple of 8 would get a pitch-8 walk over garbage channels.
void check_c8(const Tensor &t, const char *name) {
  TORCH_CHECK(t.size(1) % 8 == 0 && t.size(1) >= 8, name,
              ": channel count must be a positive multiple of 8, got ",
              t.size(1));
}

void check_bn_c(const Tensor &t, const char *name) {
  check_c8(t, name);
  TORCH_CHECK(t.size(1) <= 2048, name, ": BatchNorm kernels need C <= 2048");
  TORCH_CHECK(t.numel() > 0, name, " is empty");
}

// operand of an elementwise kernel that indexes it exactly like `like`
void check_same_cl_bf16(const Tensor &t, const Tensor &like, const char *name) {
  check_cl_bf16(t, name);
  TORCH_CHECK(t.sizes() == like.sizes(), name, " has shape ", t.sizes(),
              ", expected ", like.sizes());
  TORCH_CHECK(t.device() == like.device(), name, " is on another device");
}

// per-channel fp32 vector ([C], dense) read by a kernel
void check_chan_f32(const Tensor &t, int64_t C, const char *name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() == C,
              name, " must be a contiguous fp32 [C] GPU tensor");
}

// ReLU bitmask, one byte per octet: [M][C/8] uint8
void check_relu_mask(const Tensor &t, int64_t octets, const char *name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kByte &&
                  t.is_contiguous() && t.numel() == octets,
              name, " must be a contiguous uint8 GPU tensor of ", octets,
              " bytes (one per 8 channels), got ", t.numel());
}

// Geometry of one convolution as every conv entry point sees it: the input
// side (N, C, H, W), the weight (wK, wC, R, S) and the output side (dN, Kout,
// HO, WO). The kernels derive every address from these numbers alone and
// trust them: operands are walked in 16 B octets of 8 channels (C and Kout
// multiples of 8 — forward too: its split-K reduce walks M*Kout in float4
// groups and drops a tail), batch / channel / spatial extents index both
// tensors, and row counts are ints. An entry point that derives the output
// side itself (forward) passes dN = N, Kout = wK and HO = WO = -1.
struct ConvGeom {
  int HO, WO;
};
ConvGeom check_conv_geometry(const char *op, bool dgrad, int64_t N, int64_t C,
                             int64_t H, int64_t W, int64_t wK, int64_t wC,
                             int64_t R, int64_t S, int64_t dN, int64_t Kout,
                             int64_t HO, int64_t WO, int64_t stride,
                             int64_t pad) {
  if (dgrad) {
    // conv_dgrad routes every stride != 1 to the parity-2 decomposition
    // (conv.hip conv_dgrad_s2), which is stride-2-only by construction.
    TORCH_CHECK(stride == 1 || stride == 2, op,
                " supports stride 1 or 2 only, got ", stride);
  } else {
    TORCH_CHECK(stride >= 1 && stride <= 64, op,
                ": stride must be in [1, 64], got ", stride);
  }
  TORCH_CHECK(pad >= 0 && pad <= 64, op, ": pad must be in [0, 64], got ", pad);
  TORCH_CHECK(R >= 1 && S >= 1 && R * S <= 1024, op, ": kernel ", R, "x", S,
              " out of range");
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1, op, ": empty input ", N, "x", H, "x",
              W);
  TORCH_CHECK(C >= 8 && C % 8 == 0, op,
              " requires C%8==0 (pad the stem input), got C=", C);
  TORCH_CHECK(Kout >= 8 && Kout % 8 == 0, op,
              " requires out-channels %8==0, got ", Kout);
  TORCH_CHECK(wK == Kout && wC == C, op, ": conv channel mismatch, weight is [",
              wK, "][", wC, "], expected [", Kout, "][", C, "]");
  TORCH_CHECK(dN == N, op, ": batch mismatch, ", dN, " output images for ", N,
              " input images");
  TORCH_CHECK(H + 2 * pad >= R && W + 2 * pad >= S, op, ": kernel ", R, "x", S,
              " larger than the padded input");
  int64_t ho = (H + 2 * pad - R) / stride + 1;
  int64_t wo = (W + 2 * pad - S) / stride + 1;
  TORCH_CHECK((HO < 0 || HO == ho) && (WO < 0 || WO == wo), op, ": output is ",
              HO, "x", WO, ", the geometry gives ", ho, "x", wo);
  const int64_t lim = (int64_t)1 << 31;
  TORCH_CHECK(N * H * W < lim && N * ho * wo < lim && R * S * C < lim &&
                  R * S * Kout < lim,
              op, ": GEMM extent does not fit an int");
  return {(int)ho, (int)wo};
}

void check_same_device(const Tensor &t, const Tensor &like, const char *name) {
  TORCH_CHECK(t.device() == like.device(), name, " is on another device");
}

Tensor empty_cl_bf16(int64_t n, int64_t c, int64_t h, int64_t w, const Tensor &like) {
  // memory_format at allocation — .contiguous() on a fresh empty COPIES.
  return at::empty({n, c, h, w}, like.options().dtype(at::kBFloat16),
                   at::MemoryFormat::ChannelsLast);
}

} // namespace

// ------------------------- conv -------------------------
static Tensor conv2d_fwd(const Tensor &x, const Tensor &w, int64_t stride,
                         int64_t pad) {
  check_cl_bf16(x, "x");
  check_cl_bf16(w, "w");
  check_same_device(w, x, "w");
  const ConvGeom g = check_conv_geometry(
      "conv2d_fwd", false, x.size(0), x.size(1), x.size(2), x.size(3),
      w.size(0), w.size(1), w.size(2), w.size(3), x.size(0), w.size(0), -1, -1,
      stride, pad);
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Kout = w.size(0), R = w.size(2), S = w.size(3);
  int HO = g.HO, WO = g.WO;
  Tensor y = empty_cl_bf16(N, Kout, HO, WO, x);
  long M = (long)N * HO * WO;
  int splits = conv_splits(M, Kout, R * S * C);
  Tensor partial;
  float *pp = nullptr;
  if (splits > 1) {
    partial = at::empty({(long)splits, M, (long)Kout},
                        x.options().dtype(at::kFloat));
    pp = partial.data_ptr<float>();
  }
  CHK(conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), N, H, W, C, Kout, R,
               S, (int)stride, (int)pad, HO, WO, splits, pp, cur_stream()));
  return y;
}

static Tensor conv2d_dgrad(const Tensor &dy, const Tensor &w, int64_t H,
                           int64_t W, int64_t stride, int64_t pad) {
  check_cl_bf16(dy, "dy");
  check_cl_bf16(w, "w");
  check_same_device(w, dy, "w");
  check_conv_geometry("conv2d_dgrad", true, dy.size(0), w.size(1), H, W,
                      w.size(0), w.size(1), w.size(2), w.size(3), dy.size(0),
                      dy.size(1), dy.size(2), dy.size(3), stride, pad);
  const HIPDeviceGuard guard(dy.device());
  int N = dy.size(0), Kout = dy.size(1), HO = dy.size(2), WO = dy.size(3);
  int C = w.size(1), R = w.size(2), S = w.size(3);
  Tensor dx = empty_cl_bf16(N, C, H, W, dy);
  long M = (long)N * H * W;
  int splits = stride == 1 ? conv_splits(M, C, R * S * Kout) : 1;
  Tensor partial;
  float *pp = nullptr;
  if (splits > 1) {
    partial = at::empty({(long)splits, M, (long)C},
                        dy.options().dtype(at::kFloat));
    pp = partial.data_ptr<float>();
  }
  CHK(conv_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), N, (int)H,
                 (int)W, C, Kout, R, S, (int)stride, (int)pad, HO, WO, splits,
                 pp, cur_stream()));
  return dx;
}

static Tensor conv2d_wgrad(const Tensor &x, const Tensor &dy, int64_t R,
                           int64_t S, int64_t stride, int64_t pad) {
  check_cl_bf16(x, "x");
  check_cl_bf16(dy, "dy");
  check_same_device(dy, x, "dy");
  check_conv_geometry("conv2d_wgrad", false, x.size(0), x.size(1), x.size(2),
                      x.size(3), dy.size(1), x.size(1), R, S, dy.size(0),
                      dy.size(1), dy.size(2), dy.size(3), stride, pad);
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Kout = dy.size(1), HO = dy.size(2), WO = dy.size(3);
  int RSC = (int)R * S * C;
  long M = (long)N * HO * WO;
  int splits = wgrad_splits(Kout, RSC, M);
  Tensor partial = at::empty({(long)splits, (long)Kout, (long)RSC},
                             x.options().dtype(at::kFloat));
  // dw bf16 (fp32-accumulated in the split-K slabs, rounded once at the
  // reduce) with channels_last memory [Kout][R][S][C]
  Tensor dw = at::empty({(int64_t)Kout, (int64_t)C, R, S},
                        x.options().dtype(at::kBFloat16),
                        at::MemoryFormat::ChannelsLast);
  CHK(conv_wgrad_implicit(dy.data_ptr(), x.data_ptr(),
                          partial.data_ptr<float>(), dw.data_ptr(), N, H, W, C,
                          Kout, (int)R, (int)S, (int)stride, (int)pad, HO, WO,
                          splits, 1, cur_stream()));
  return dw;
}

static void check_ew_first(const Tensor &t, const char *name);
static void check_ew_same(const Tensor &t, const Tensor &first,
                          const char *name);

// c = a + b, bf16 16B-vectorized (the residual-join gradient sum)
static Tensor add_bf16_b(const Tensor &a, const Tensor &b) {
  check_ew_first(a, "a");
  check_ew_same(b, a, "b");
  const HIPDeviceGuard guard(a.device());
  Tensor c = at::empty_like(a);
  CHK(add_bf16(a.data_ptr(), b.data_ptr(), c.data_ptr(), a.numel(), cur_stream()));
  return c;
}

// dx_acc += dgrad(dy, w) for a 1x1 stride-1 conv (bottleneck conv1)
static void conv2d_dgrad_acc(const Tensor &dy, const Tensor &w, Tensor &dx_acc) {
  check_cl_bf16(dy, "dy");
  check_cl_bf16(w, "w");
  check_cl_bf16(dx_acc, "dx_acc");
  check_same_device(w, dy, "w");
  check_same_device(dx_acc, dy, "dx_acc");
  TORCH_CHECK(w.size(2) == 1 && w.size(3) == 1, "acc dgrad is 1x1-only");
  // 1x1 stride 1 pad 0: dx_acc is [N][C][HO][WO], every extent from dy / w
  check_conv_geometry("conv2d_dgrad_acc", true, dx_acc.size(0), dx_acc.size(1),
                      dx_acc.size(2), dx_acc.size(3), w.size(0), w.size(1), 1,
                      1, dy.size(0), dy.size(1), dy.size(2), dy.size(3), 1, 0);
  const HIPDeviceGuard guard(dy.device());
  long M = (long)dy.size(0) * dy.size(2) * dy.size(3);
  CHK(conv_dgrad_1x1_acc(dy.data_ptr(), w.data_ptr(), dx_acc.data_ptr(), M,
                         (int)w.size(1), (int)dy.size(1), cur_stream()));
}

// ------------------------- batchnorm -------------------------
// res (optional, may be undefined): residual tensor folded into the apply
// pass — y = [relu](bn(x) + res), the bottleneck-join fusion.
// conv forward + fused BN partial stats: returns (y, slab). The slab is
// [rows][2][Kout] fp32 and bn_fwd_train_pre takes its row count from the
// tensor: ceil(M/64) bands from the GEMM epilogue on unsplit routes, the
// partials grid from the reduce+stats kernel on split-K routes. Each kind is
// produced only when its flag (fuse_epilogue / fuse_splitk) is set. Allocated with at::empty — the kernels write every entry the
// finalize reads. The slab is EMPTY when no stats were produced (the
// shape's flag is off, or a route without a stats epilogue): the caller
// then runs bn_fwd_train.
static std::vector<Tensor> conv2d_fwd_bn(const Tensor &x, const Tensor &w,
                                         int64_t stride, int64_t pad,
                                         bool fuse_splitk,
                                         bool fuse_epilogue) {
  check_cl_bf16(x, "x");
  check_cl_bf16(w, "w");
  check_same_device(w, x, "w");
  const ConvGeom g = check_conv_geometry(
      "conv2d_fwd_bn", false, x.size(0), x.size(1), x.size(2), x.size(3),
      w.size(0), w.size(1), w.size(2), w.size(3), x.size(0), w.size(0), -1, -1,
      stride, pad);
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Kout = w.size(0), R = w.size(2), S = w.size(3);
  int HO = g.HO, WO = g.WO;
  long M = (long)N * HO * WO;
  int splits = conv_splits(M, Kout, R * S * C);
  auto f32 = x.options().dtype(at::kFloat);
  long rows = conv_fwd_bn_rows(M, C, Kout, R, S, (int)stride, (int)pad, splits);
  if (rows == 0 || (splits > 1 ? !fuse_splitk : !fuse_epilogue)) {
    Tensor y = conv2d_fwd(x, w, stride, pad);
    return {y, at::empty({0}, f32)};
  }
  Tensor y = empty_cl_bf16(N, Kout, HO, WO, x);
  Tensor slab = at::empty({rows, 2, (long)Kout}, f32);
  Tensor partial;
  float *pp = nullptr;
  if (splits > 1) {
    partial = at::empty({(long)splits, M, (long)Kout}, f32);
    pp = partial.data_ptr<float>();
  }
  CHK(conv_fwd_bn(x.data_ptr(), w.data_ptr(), y.data_ptr(), N, H, W, C, Kout,
                  R, S, (int)stride, (int)pad, HO, WO, splits, pp,
                  slab.data_ptr<float>(), cur_stream()));
  return {y, slab};
}

// stride-1 dgrad whose split-K reduce also emits the BN-backward partial
// stats of the BN layer consuming the result as its dy (bx/by/mask/mean/
// invstd are that layer's saved tensors): returns (dy, slab [rows][2][C]).
// The slab is EMPTY when the dgrad does not split (or stride 2): the result
// is then conv2d_dgrad's and the caller runs bn_bwd.
static std::vector<Tensor> conv2d_dgrad_bn(
    const Tensor &dy, const Tensor &w, int64_t H, int64_t W, int64_t stride,
    int64_t pad, const Tensor &bx, const Tensor &by, const Tensor &mean,
    const Tensor &invstd, bool relu, const Tensor &mask) {
  check_cl_bf16(dy, "dy");
  check_cl_bf16(w, "w");
  check_same_device(w, dy, "w");
  check_conv_geometry("conv2d_dgrad_bn", true, dy.size(0), w.size(1), H, W,
                      w.size(0), w.size(1), w.size(2), w.size(3), dy.size(0),
                      dy.size(1), dy.size(2), dy.size(3), stride, pad);
  const HIPDeviceGuard guard(dy.device());
  int N = dy.size(0), Kout = dy.size(1), HO = dy.size(2), WO = dy.size(3);
  int C = w.size(1), R = w.size(2), S = w.size(3);
  long M = (long)N * H * W;
  auto f32 = dy.options().dtype(at::kFloat);
  int splits = stride == 1 ? conv_splits(M, C, R * S * Kout) : 1;
  long rows = conv_dgrad_bn_rows(M, C, Kout, R, S, (int)stride, splits);
  if (rows == 0) return {conv2d_dgrad(dy, w, H, W, stride, pad), at::empty({0}, f32)};
  check_cl_bf16(bx, "bx");
  TORCH_CHECK(bx.size(0) == N && bx.size(1) == C && bx.size(2) == H &&
                  bx.size(3) == W, "bx must have the dgrad output's shape");
  TORCH_CHECK(mean.numel() == C && invstd.numel() == C, "mean/invstd shape");
  const uint8_t *mp = nullptr;
  if (mask.defined() && mask.numel() > 0) {
    TORCH_CHECK(mask.numel() == M * (C / 8), "mask shape");
    mp = mask.data_ptr<uint8_t>();
  }
  if (relu && !mp) {
    check_cl_bf16(by, "by");
    TORCH_CHECK(by.numel() == bx.numel(), "by shape");
  }
  Tensor dx = empty_cl_bf16(N, C, H, W, dy);
  Tensor partial = at::empty({(long)splits, M, (long)C}, f32);
  Tensor slab = at::empty({rows, 2, (long)C}, f32);
  CHK(conv_dgrad_bn(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), N, (int)H,
                    (int)W, C, Kout, R, S, (int)pad, HO, WO, splits,
                    partial.data_ptr<float>(), bx.data_ptr(),
                    by.defined() && by.numel() > 0 ? by.data_ptr() : nullptr, mp, mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    relu ? 1 : 0, slab.data_ptr<float>(), cur_stream()));
  return {dx, slab};
}

// bn_fwd_train consuming a pre-computed stats slab [rows][2][C] (skips
// partials); the row count travels with the tensor
static std::vector<Tensor> bn_fwd_train_pre(
    const Tensor &x, const Tensor &slab, const Tensor &gamma,
    const Tensor &beta, double eps, bool relu, const Tensor &running_mean,
    const Tensor &running_var, double momentum, const Tensor &res) {
  check_cl_bf16(x, "x");
  check_bn_c(x, "x");
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  long M = (long)N * H * W;
  TORCH_CHECK(slab.dim() == 3 && slab.size(0) >= 1 && slab.size(1) == 2 &&
                  slab.size(2) == C && slab.is_contiguous() &&
                  slab.scalar_type() == at::kFloat, "slab must be [rows][2][C] fp32");
  auto f32 = x.options().dtype(at::kFloat);
  Tensor y = empty_cl_bf16(N, C, H, W, x);
  Tensor mean = at::empty({C}, f32), invstd = at::empty({C}, f32);
  Tensor scale = at::empty({C}, f32), shift = at::empty({C}, f32);
  float *rm = running_mean.defined() && running_mean.numel() == C
                  ? running_mean.data_ptr<float>() : nullptr;
  float *rv = rm ? running_var.data_ptr<float>() : nullptr;
  const void *resp = nullptr;
  if (res.defined() && res.numel() > 0) {
    check_same_cl_bf16(res, x, "res");
    resp = res.data_ptr();
  }
  Tensor mask;
  uint8_t *mp = nullptr;
  if (relu) { // 1 bit/element relu mask: backward skips the y re-read
    mask = at::empty({M, (long)C / 8}, x.options().dtype(at::kByte));
    mp = mask.data_ptr<uint8_t>();
  } else {
    mask = at::empty({0}, x.options().dtype(at::kByte));
  }
  CHK(bn_fwd_train_pre_launch(
      slab.data_ptr<float>(), (int)slab.size(0), x.data_ptr(), resp,
      gamma.data_ptr<float>(), beta.data_ptr<float>(), (float)eps,
      relu ? 1 : 0, y.data_ptr(), mp, mean.data_ptr<float>(),
      invstd.data_ptr<float>(), scale.data_ptr<float>(),
      shift.data_ptr<float>(), rm, rv, (float)momentum, M, C, cur_stream()));
  return {y, mean, invstd, mask};
}

static std::vector<Tensor> bn_fwd_train(const Tensor &x, const Tensor &gamma,
                                        const Tensor &beta, double eps,
                                        bool relu, const Tensor &running_mean,
                                        const Tensor &running_var,
                                        double momentum, const Tensor &res) {
  check_cl_bf16(x, "x");
  check_bn_c(x, "x");
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  long M = (long)N * H * W;
  check_chan_f32(gamma, C, "gamma");
  check_chan_f32(beta, C, "beta");
  auto f32 = x.options().dtype(at::kFloat);
  Tensor y = empty_cl_bf16(N, C, H, W, x);
  Tensor mean = at::empty({C}, f32), invstd = at::empty({C}, f32);
  Tensor scale = at::empty({C}, f32), shift = at::empty({C}, f32);
  Tensor partial = at::empty({(long)bn_grid_cap() * 2 * C}, f32);
  float *rm = nullptr, *rv = nullptr;
  if (running_mean.defined() && running_mean.numel() > 0) {
    check_chan_f32(running_mean, C, "running_mean");
    check_chan_f32(running_var, C, "running_var");
    rm = running_mean.data_ptr<float>();
    rv = running_var.data_ptr<float>();
  }
  const void *resp = nullptr;
  if (res.defined() && res.numel() > 0) {
    check_same_cl_bf16(res, x, "res");
    resp = res.data_ptr();
  }
  Tensor mask;
  uint8_t *mp = nullptr;
  if (relu) { // 1 bit/element relu mask: backward skips the y re-read
    mask = at::empty({M, (long)C / 8}, x.options().dtype(at::kByte));
    mp = mask.data_ptr<uint8_t>();
  } else {
    mask = at::empty({0}, x.options().dtype(at::kByte));
  }
  CHK(bn_fwd_train_launch(x.data_ptr(), resp, gamma.data_ptr<float>(),
                          beta.data_ptr<float>(), (float)eps, relu ? 1 : 0,
                          y.data_ptr(), mp, mean.data_ptr<float>(),
                          invstd.data_ptr<float>(), scale.data_ptr<float>(),
                          shift.data_ptr<float>(), partial.data_ptr<float>(),
                          rm, rv, (float)momentum, M, C, cur_stream()));
  return {y, mean, invstd, mask};
}

static Tensor bn_fwd_eval(const Tensor &x, const Tensor &scale,
                          const Tensor &shift, bool relu) {
  check_cl_bf16(x, "x");
  check_bn_c(x, "x");
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  check_chan_f32(scale, C, "scale");
  check_chan_f32(shift, C, "shift");
  Tensor y = empty_cl_bf16(N, C, H, W, x);
  CHK(bn_fwd_eval_launch(x.data_ptr(), scale.data_ptr<float>(),
                         shift.data_ptr<float>(), relu ? 1 : 0,
                         y.data_ptr(), (long)N * H * W, C, cur_stream()));
  return y;
}

// Operand checks shared by bn_bwd and bn_bwd_pre; returns the mask pointer
// (nullptr: the kernels gate dy by y > 0 instead, and then read y).
static const uint8_t *check_bn_bwd_args(const Tensor &dy, const Tensor &x,
                                        const Tensor &y, const Tensor &gamma,
                                        const Tensor &mean,
                                        const Tensor &invstd, bool relu,
                                        const Tensor &mask) {
  check_cl_bf16(x, "x");
  check_bn_c(x, "x");
  check_same_cl_bf16(dy, x, "dy");
  int64_t C = x.size(1);
  check_chan_f32(gamma, C, "gamma");
  check_chan_f32(mean, C, "mean");
  check_chan_f32(invstd, C, "invstd");
  const uint8_t *mp = nullptr;
  if (mask.defined() && mask.numel() > 0) {
    check_relu_mask(mask, x.numel() / 8, "mask");
    mp = mask.data_ptr<uint8_t>();
  }
  if (relu && !mp) check_same_cl_bf16(y, x, "y");
  return mp;
}

static std::vector<Tensor> bn_bwd(const Tensor &dy, const Tensor &x,
                                  const Tensor &y, const Tensor &gamma,
                                  const Tensor &mean, const Tensor &invstd,
                                  bool relu, const Tensor &mask) {
  const uint8_t *mp =
      check_bn_bwd_args(dy, x, y, gamma, mean, invstd, relu, mask);
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  long M = (long)N * H * W;
  auto f32 = x.options().dtype(at::kFloat);
  Tensor dx = empty_cl_bf16(N, C, H, W, x);
  Tensor dgamma = at::empty({C}, f32), dbeta = at::empty({C}, f32);
  Tensor k1 = at::empty({C}, f32), k2 = at::empty({C}, f32), k3 = at::empty({C}, f32);
  Tensor partial = at::empty({(long)bn_grid_cap() * 2 * C}, f32);
  CHK(bn_bwd_launch(dy.data_ptr(), x.data_ptr(), y.data_ptr(), mp,
                    gamma.data_ptr<float>(), mean.data_ptr<float>(),
                    invstd.data_ptr<float>(), relu ? 1 : 0, dx.data_ptr(),
                    dgamma.data_ptr<float>(), dbeta.data_ptr<float>(),
                    k1.data_ptr<float>(), k2.data_ptr<float>(),
                    k3.data_ptr<float>(), partial.data_ptr<float>(), M, C,
                    cur_stream()));
  return {dx, dgamma, dbeta};
}

// bn_bwd starting from the dgrad reduce's backward slab [rows][2][C]
static std::vector<Tensor> bn_bwd_pre(const Tensor &dy, const Tensor &slab,
                                      const Tensor &x, const Tensor &y,
                                      const Tensor &gamma, const Tensor &mean,
                                      const Tensor &invstd, bool relu,
                                      const Tensor &mask) {
  const uint8_t *mp =
      check_bn_bwd_args(dy, x, y, gamma, mean, invstd, relu, mask);
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  long M = (long)N * H * W;
  TORCH_CHECK(slab.is_cuda() && slab.dim() == 3 && slab.size(0) >= 1 &&
                  slab.size(1) == 2 && slab.size(2) == C &&
                  slab.is_contiguous() && slab.scalar_type() == at::kFloat,
              "slab must be [rows][2][C] fp32");
  auto f32 = x.options().dtype(at::kFloat);
  Tensor dx = empty_cl_bf16(N, C, H, W, x);
  Tensor dgamma = at::empty({C}, f32), dbeta = at::empty({C}, f32);
  Tensor k1 = at::empty({C}, f32), k2 = at::empty({C}, f32), k3 = at::empty({C}, f32);
  CHK(bn_bwd_pre_launch(slab.data_ptr<float>(), (int)slab.size(0),
                        dy.data_ptr(), x.data_ptr(), y.data_ptr(), mp,
                        gamma.data_ptr<float>(), mean.data_ptr<float>(),
                        invstd.data_ptr<float>(), relu ? 1 : 0, dx.data_ptr(),
                        dgamma.data_ptr<float>(), dbeta.data_ptr<float>(),
                        k1.data_ptr<float>(), k2.data_ptr<float>(),
                        k3.data_ptr<float>(), M, C, cur_stream()));
  return {dx, dgamma, dbeta};
}

// Residual-join gradient fused with the backward partial stats of the BN
// layer(s) that take it as their dy (the previous bottleneck's bn3 and, with
// ds_x given, its downsample BN):
//   jmask given: dxt = a·jmask + b (add_relu_bwd_add_mask), else dxt = a + b
//   (add_bf16). cons_x/mean/invstd are the consumer BN's saved tensors,
//   cons_mask the ReLU bitmask both consumers gate dxt by.
// Returns (dxt, slab[, slab_ds]), each slab [rows][2][C] for bn_bwd_pre.
static std::vector<Tensor> join_bwd_stats(
    const Tensor &a, const Tensor &jmask, const Tensor &b,
    const Tensor &cons_x, const Tensor &cons_mean, const Tensor &cons_invstd,
    const Tensor &cons_mask, const Tensor &ds_x, const Tensor &ds_mean,
    const Tensor &ds_invstd) {
  check_cl_bf16(a, "a");
  check_cl_bf16(b, "b");
  check_cl_bf16(cons_x, "cons_x");
  const HIPDeviceGuard guard(a.device());
  int N = a.size(0), C = a.size(1), H = a.size(2), W = a.size(3);
  long M = (long)N * H * W;
  TORCH_CHECK(C % 8 == 0 && C / 8 <= 256, "join_bwd_stats needs C%8==0, C<=2048");
  TORCH_CHECK(M >= 1, "empty tensor");
  TORCH_CHECK(b.sizes() == a.sizes() && cons_x.sizes() == a.sizes(),
              "b and cons_x must have a's shape");
  auto check_stat = [&](const Tensor &t, const char *name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                    t.is_contiguous() && t.numel() == C,
                name, " must be a contiguous fp32 [C] GPU tensor");
  };
  auto check_mask = [&](const Tensor &t, const char *name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kByte &&
                    t.is_contiguous() && t.numel() == M * (C / 8),
                name, " must be a contiguous uint8 [M][C/8] GPU tensor");
  };
  check_stat(cons_mean, "cons_mean");
  check_stat(cons_invstd, "cons_invstd");
  check_mask(cons_mask, "cons_mask");
  const uint8_t *jp = nullptr;
  if (jmask.defined() && jmask.numel() > 0) {
    check_mask(jmask, "jmask");
    jp = jmask.data_ptr<uint8_t>();
  }
  const bool has_ds = ds_x.defined() && ds_x.numel() > 0;
  auto f32 = a.options().dtype(at::kFloat);
  long rows = bn_stats_grid(M, C);
  Tensor dxt = empty_cl_bf16(N, C, H, W, a);
  Tensor slab = at::empty({rows, 2, (long)C}, f32);
  Tensor slab_ds;
  const void *xdp = nullptr;
  const float *mdp = nullptr, *vdp = nullptr;
  float *sdp = nullptr;
  if (has_ds) {
    check_cl_bf16(ds_x, "ds_x");
    TORCH_CHECK(ds_x.sizes() == a.sizes(), "ds_x must have a's shape");
    check_stat(ds_mean, "ds_mean");
    check_stat(ds_invstd, "ds_invstd");
    slab_ds = at::empty({rows, 2, (long)C}, f32);
    xdp = ds_x.data_ptr();
    mdp = ds_mean.data_ptr<float>();
    vdp = ds_invstd.data_ptr<float>();
    sdp = slab_ds.data_ptr<float>();
  }
  CHK(bn_join_stats_launch(a.data_ptr(), jp, b.data_ptr(), dxt.data_ptr(),
                           cons_mask.data_ptr<uint8_t>(), cons_x.data_ptr(),
                           cons_mean.data_ptr<float>(),
                           cons_invstd.data_ptr<float>(),
                           slab.data_ptr<float>(), xdp, mdp, vdp, sdp, M, C,
                           cur_stream()));
  if (has_ds) return {dxt, slab, slab_ds};
  return {dxt, slab};
}

// ------------------------- pooling -------------------------
// the argmax byte holds r*K + s, so K*K must fit in a uint8
static void check_pool_geom(int64_t K, int64_t stride, int64_t pad) {
  TORCH_CHECK(K >= 1 && K <= 15 && stride >= 1 && pad >= 0 && pad < K,
              "maxpool needs 1 <= K <= 15, stride >= 1, 0 <= pad < K; got K=",
              K, " stride=", stride, " pad=", pad);
}

static std::vector<Tensor> maxpool_fwd(const Tensor &x, int64_t K,
                                       int64_t stride, int64_t pad) {
  check_cl_bf16(x, "x");
  check_c8(x, "x");
  check_pool_geom(K, stride, pad);
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(H + 2 * pad >= K && W + 2 * pad >= K,
              "maxpool window larger than the padded input");
  int HO = (H + 2 * (int)pad - (int)K) / (int)stride + 1;
  int WO = (W + 2 * (int)pad - (int)K) / (int)stride + 1;
  Tensor y = empty_cl_bf16(N, C, HO, WO, x);
  Tensor idx = at::empty({N, HO, WO, C}, x.options().dtype(at::kByte));
  CHK(maxpool_fwd_launch(x.data_ptr(), y.data_ptr(), idx.data_ptr<uint8_t>(),
                         N, H, W, HO, WO, C, (int)K, (int)stride, (int)pad,
                         cur_stream()));
  return {y, idx};
}

static Tensor maxpool_bwd(const Tensor &dy, const Tensor &idx, int64_t H,
                          int64_t W, int64_t K, int64_t stride, int64_t pad) {
  check_cl_bf16(dy, "dy");
  check_c8(dy, "dy");
  check_pool_geom(K, stride, pad);
  const HIPDeviceGuard guard(dy.device());
  int N = dy.size(0), C = dy.size(1), HO = dy.size(2), WO = dy.size(3);
  TORCH_CHECK(H + 2 * pad >= K && W + 2 * pad >= K &&
                  HO == (H + 2 * pad - K) / stride + 1 &&
                  WO == (W + 2 * pad - K) / stride + 1,
              "dy is not the pooled shape of an input of ", H, "x", W);
  // idx is [N][HO][WO][C] uint8: one argmax byte per dy element
  TORCH_CHECK(idx.is_cuda() && idx.device() == dy.device() &&
                  idx.scalar_type() == at::kByte && idx.is_contiguous() &&
                  idx.numel() == dy.numel(),
              "idx must be a contiguous uint8 GPU tensor with one byte per "
              "dy element");
  Tensor dx = empty_cl_bf16(N, C, H, W, dy);
  CHK(maxpool_bwd_launch(dy.data_ptr(), idx.data_ptr<uint8_t>(), dx.data_ptr(),
                         N, (int)H, (int)W, HO, WO, C, (int)K, (int)stride,
                         (int)pad, cur_stream()));
  return dx;
}

// ------------------------- gap -------------------------
static Tensor gap_fwd_b(const Tensor &x) {
  check_cl_bf16(x, "x");
  check_c8(x, "x");
  TORCH_CHECK(x.size(2) * x.size(3) >= 1, "x has no pixels");
  const HIPDeviceGuard guard(x.device());
  int N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  Tensor y = at::empty({N, C}, x.options());
  CHK(gap_fwd(x.data_ptr(), y.data_ptr(), N, HW, C, cur_stream()));
  return y;
}

static Tensor gap_bwd_b(const Tensor &dy, int64_t H, int64_t W) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16);
  TORCH_CHECK(dy.dim() == 2, "dy must be [N][C]");
  check_c8(dy, "dy");
  TORCH_CHECK(H >= 1 && W >= 1, "gap_bwd needs H, W >= 1");
  const HIPDeviceGuard guard(dy.device());
  Tensor dyc = dy.contiguous();
  int N = dy.size(0), C = dy.size(1);
  Tensor dx = empty_cl_bf16(N, C, H, W, dy);
  CHK(gap_bwd(dyc.data_ptr(), dx.data_ptr(), N, (int)(H * W), C, cur_stream()));
  return dx;
}

// ------------------------- layernorm -------------------------
static std::vector<Tensor> layernorm_fwd(const Tensor &x, const Tensor &gamma,
                                         const Tensor &beta, double eps) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  const HIPDeviceGuard guard(x.device());
  Tensor xc = x.contiguous();
  long M = xc.numel() / xc.size(-1);
  int N = xc.size(-1);
  auto f32 = x.options().dtype(at::kFloat);
  Tensor y = at::empty_like(xc);
  Tensor mean = at::empty({M}, f32), rstd = at::empty({M}, f32);
  CHK(ln_fwd(xc.data_ptr(), gamma.data_ptr<float>(), beta.data_ptr<float>(),
             y.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(), M,
             N, (float)eps, cur_stream()));
  return {y, mean, rstd};
}

// y = LN(a + b) with the sum materialized for backward (one pass instead
// of a separate residual add)
static std::vector<Tensor> layernorm_add_fwd(const Tensor &a, const Tensor &b,
                                             const Tensor &gamma,
                                             const Tensor &beta, double eps) {
  const HIPDeviceGuard guard(a.device());
  Tensor ac = a.contiguous(), bc = b.contiguous();
  TORCH_CHECK(ac.sizes() == bc.sizes());
  long M = ac.numel() / ac.size(-1);
  int N = ac.size(-1);
  auto f32 = a.options().dtype(at::kFloat);
  Tensor sum = at::empty_like(ac);
  Tensor y = at::empty_like(ac);
  Tensor mean = at::empty({M}, f32), rstd = at::empty({M}, f32);
  CHK(ln_fwd_add(ac.data_ptr(), bc.data_ptr(), gamma.data_ptr<float>(),
                 beta.data_ptr<float>(), sum.data_ptr(), y.data_ptr(),
                 mean.data_ptr<float>(), rstd.data_ptr<float>(), M, N,
                 (float)eps, cur_stream()));
  return {y, sum, mean, rstd};
}

static std::vector<Tensor> layernorm_bwd(const Tensor &dy, const Tensor &x,
                                         const Tensor &gamma,
                                         const Tensor &mean,
                                         const Tensor &rstd) {
  const HIPDeviceGuard guard(x.device());
  Tensor dyc = dy.contiguous(), xc = x.contiguous();
  long M = xc.numel() / xc.size(-1);
  int N = xc.size(-1);
  auto f32 = x.options().dtype(at::kFloat);
  // slab rows must cover ln_bwd's stats grid (≤512 by construction)
  Tensor partial = at::empty({512, 2L * N}, f32);
  Tensor dgb = at::empty({2L * N}, f32);
  Tensor dx = at::empty_like(xc);
  CHK(ln_bwd(dyc.data_ptr(), xc.data_ptr(), gamma.data_ptr<float>(),
             mean.data_ptr<float>(), rstd.data_ptr<float>(), dx.data_ptr(),
             partial.data_ptr<float>(), dgb.data_ptr<float>(), M, N, nullptr,
             cur_stream()));
  return {dx, dgb.narrow(0, 0, N), dgb.narrow(0, N, N)};
}

// ------------------------- dropout -------------------------
// The device random-number state of philox.h: int64 (seed, offset)
static void check_rng_state(const Tensor &state, const Tensor &like) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong &&
                  state.is_contiguous() && state.dim() == 1 &&
                  state.numel() == 2,
              "state must be a contiguous int64 [2] GPU tensor (seed, offset)");
  TORCH_CHECK(state.device() == like.device(), "state is on another device");
}

struct DropParams {
  uint32_t site, thr;
  float scale;
};
static DropParams check_drop_params(double p, int64_t site) {
  DropParams d;
  TORCH_CHECK(dropout_thr_scale(p, &d.thr, &d.scale),
              "dropout: p must be in [0, 1) with round(p * 65536) <= 65535, "
              "got ", p);
  TORCH_CHECK(site >= 0 && site <= (int64_t)UINT32_MAX,
              "dropout: site must fit a uint32, got ", site);
  d.site = (uint32_t)site;
  return d;
}

// dense bf16 GPU tensor walked in octets by one Philox call each
static void check_drop_bf16(const Tensor &t, const char *name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, name,
              " must be a bf16 GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(dropout_numel_ok(t.numel()), name,
              ": element count must be a positive multiple of 8 below 2^35, "
              "got ", t.numel());
}

static void check_drop_same(const Tensor &t, const Tensor &like,
                            const char *name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
                  t.scalar_type() == at::kBFloat16 && t.is_contiguous() &&
                  t.sizes() == like.sizes(),
              name, " must be a contiguous bf16 tensor of shape ",
              like.sizes(), " on the first operand's GPU");
}

// keep bitmask, one byte per octet, of the given shape
static void check_keep_mask(const Tensor &mask, at::IntArrayRef shape,
                            const Tensor &like) {
  TORCH_CHECK(mask.is_cuda() && mask.device() == like.device() &&
                  mask.scalar_type() == at::kByte && mask.is_contiguous() &&
                  mask.sizes() == shape,
              "mask must be a contiguous uint8 GPU tensor of shape ", shape,
              " (one byte per 8 elements), got ", mask.sizes());
}

// fp32 [N] LayerNorm vector on the activation's device
static void check_ln_vec(const Tensor &t, int64_t n, const Tensor &like,
                         const char *name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
                  t.scalar_type() == at::kFloat && t.is_contiguous() &&
                  t.numel() == n,
              name, " must be a contiguous fp32 GPU tensor of ", n,
              " elements");
}

static void rng_tick_b(const Tensor &state) {
  check_rng_state(state, state);
  const HIPDeviceGuard guard(state.device());
  CHK(rng_tick(state.data_ptr<int64_t>(), cur_stream()));
}

// y = keep ? x / (1 - p_eff) : 0; returns {y, mask [numel/8] uint8}
static std::vector<Tensor> dropout_fwd_b(const Tensor &x, const Tensor &state,
                                         double p, int64_t site) {
  check_drop_bf16(x, "x");
  check_rng_state(state, x);
  const DropParams d = check_drop_params(p, site);
  const HIPDeviceGuard guard(x.device());
  Tensor y = at::empty_like(x);
  Tensor mask = at::empty({x.numel() / 8}, x.options().dtype(at::kByte));
  CHK(dropout_fwd(x.data_ptr(), state.data_ptr<int64_t>(), d.site, d.thr,
                  d.scale, y.data_ptr(), mask.data_ptr<uint8_t>(), x.numel(),
                  cur_stream()));
  return {y, mask};
}

static Tensor dropout_bwd_b(const Tensor &dy, const Tensor &mask, double p) {
  check_drop_bf16(dy, "dy");
  check_keep_mask(mask, {dy.numel() / 8}, dy);
  const DropParams d = check_drop_params(p, 0);
  const HIPDeviceGuard guard(dy.device());
  Tensor dx = at::empty_like(dy);
  CHK(dropout_bwd(dy.data_ptr(), mask.data_ptr<uint8_t>(), d.scale,
                  dx.data_ptr(), dy.numel(), cur_stream()));
  return dx;
}

// y = LN(a + dropout(b)); returns {y, s, mean, rstd, mask [M][N/8] uint8}
static std::vector<Tensor> layernorm_drop_add_fwd(
    const Tensor &a, const Tensor &b, const Tensor &gamma, const Tensor &beta,
    double eps, const Tensor &state, double p, int64_t site) {
  TORCH_CHECK(a.dim() >= 1, "a must have a feature dimension");
  check_drop_bf16(a, "a");
  check_drop_same(b, a, "b");
  const int64_t N = a.size(-1);
  TORCH_CHECK(N % 8 == 0 && N >= 8,
              "layernorm_drop_add_fwd: N must be a positive multiple of 8, "
              "got ", N);
  check_ln_vec(gamma, N, a, "gamma");
  check_ln_vec(beta, N, a, "beta");
  check_rng_state(state, a);
  const DropParams d = check_drop_params(p, site);
  const HIPDeviceGuard guard(a.device());
  const int64_t M = a.numel() / N;
  auto f32 = a.options().dtype(at::kFloat);
  Tensor sum = at::empty_like(a);
  Tensor y = at::empty_like(a);
  Tensor mean = at::empty({M}, f32), rstd = at::empty({M}, f32);
  Tensor mask = at::empty({M, N / 8}, a.options().dtype(at::kByte));
  CHK(ln_fwd_drop_add(a.data_ptr(), b.data_ptr(), gamma.data_ptr<float>(),
                      beta.data_ptr<float>(), state.data_ptr<int64_t>(),
                      d.site, d.thr, d.scale, sum.data_ptr(), y.data_ptr(),
                      mean.data_ptr<float>(), rstd.data_ptr<float>(),
                      mask.data_ptr<uint8_t>(), M, (int)N, (float)eps,
                      cur_stream()));
  return {y, sum, mean, rstd, mask};
}

// returns {da, db, dgamma, dbeta}: da = dLN/ds, db = da through the mask
static std::vector<Tensor> layernorm_drop_add_bwd(
    const Tensor &dy, const Tensor &s, const Tensor &gamma, const Tensor &mean,
    const Tensor &rstd, const Tensor &mask, double p) {
  TORCH_CHECK(s.dim() >= 1, "s must have a feature dimension");
  check_drop_bf16(s, "s");
  check_drop_same(dy, s, "dy");
  const int64_t N = s.size(-1);
  TORCH_CHECK(N % 8 == 0 && N >= 8 && N <= 2048,
              "layernorm_drop_add_bwd: N must be a multiple of 8 in "
              "[8, 2048], got ", N);
  const int64_t M = s.numel() / N;
  check_ln_vec(gamma, N, s, "gamma");
  check_ln_vec(mean, M, s, "mean");
  check_ln_vec(rstd, M, s, "rstd");
  check_keep_mask(mask, {M, N / 8}, s);
  const DropParams d = check_drop_params(p, 0);
  const HIPDeviceGuard guard(s.device());
  auto f32 = s.options().dtype(at::kFloat);
  // slab rows must cover ln_bwd's stats grid (≤512 by construction)
  Tensor partial = at::empty({512, 2L * N}, f32);
  Tensor dgb = at::empty({2L * N}, f32);
  Tensor da = at::empty_like(s), db = at::empty_like(s);
  CHK(ln_bwd_drop(dy.data_ptr(), s.data_ptr(), gamma.data_ptr<float>(),
                  mean.data_ptr<float>(), rstd.data_ptr<float>(),
                  mask.data_ptr<uint8_t>(), d.scale, da.data_ptr(),
                  db.data_ptr(), partial.data_ptr<float>(),
                  dgb.data_ptr<float>(), M, (int)N, nullptr, cur_stream()));
  return {da, db, dgb.narrow(0, 0, N), dgb.narrow(0, N, N)};
}

// ------------------------- linear -------------------------
static Tensor linear_fwd(const Tensor &x, const Tensor &w, const Tensor &b) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  const HIPDeviceGuard guard(x.device());
  Tensor xc = x.contiguous(), wc = w.contiguous();
  int M = xc.size(0), K = xc.size(1), N = wc.size(0);
  TORCH_CHECK(K % 8 == 0, "linear requires in_features %8==0");
  Tensor y = at::empty({M, N}, xc.options());
  // bias folded into the GEMM epilogue (fp32; accept bf16 bias (BERT) or
  // fp32 — the classifier keeps an fp32 bias for exactness)
  Tensor bf = b.scalar_type() == at::kFloat ? b.contiguous()
                                            : b.to(at::kFloat).contiguous();
  int fsp = gemm_fwd_splits(M, N, K);
  Tensor part;
  float *pp = nullptr;
  if (fsp > 1) {
    part = at::empty({fsp, (long)M * N}, x.options().dtype(at::kFloat));
    pp = part.data_ptr<float>();
  }
  CHK(gemm_nt_bias_sk(xc.data_ptr(), wc.data_ptr(), bf.data_ptr<float>(), pp,
                      y.data_ptr(), M, N, K, K, K, N, fsp, cur_stream()));
  return y;
}

static std::vector<Tensor> linear_bwd(const Tensor &dy, const Tensor &x,
                                      const Tensor &w) {
  const HIPDeviceGuard guard(x.device());
  Tensor dyc = dy.contiguous(), xc = x.contiguous(), wc = w.contiguous();
  int M = xc.size(0), K = xc.size(1), N = wc.size(0);
  auto f32 = x.options().dtype(at::kFloat);
  // dx = dy @ w: A = dy [M][N] k-contiguous; B = w [N rows][K cols]
  // k-strided (TN-staged in LDS — no transpose buffer). The NT operand's
  // reduce dim must be %8 (16 B load granule): zero-pad dy's N if ragged.
  long Np = (N + 7) / 8 * 8;
  Tensor dyp = dyc;
  if (Np != N) {
    dyp = at::zeros({M, Np}, dyc.options());
    dyp.narrow(1, 0, N).copy_(dyc);
  }
  Tensor dx = at::empty({M, K}, xc.options());
  int dx_splits = gemm_nt_tn_splits(M, K, N);
  Tensor dxp = dx_splits > 1 ? at::empty({dx_splits, (long)M * K}, f32) : dx;
  CHK(gemm_nt_tn_sk(dyp.data_ptr(), wc.data_ptr(),
                    dx_splits > 1 ? dxp.data_ptr<float>() : nullptr,
                    dx.data_ptr(), M, K, N, Np, K, K, dx_splits,
                    cur_stream()));
  // dw = dy^T @ x: both operands k-strided (k = batch row m) → fp32.
  // split-K when the [N][K] tile grid underfills the chip (K_reduce = M).
  // The PADDED dyp (lda = Np) keeps the vocab-ragged head on the pipe
  // route (tn_cols_ok's padded-stride contract).
  // dw in the weight's own dtype: bf16 params take the rounding inside the
  // GEMM epilogue / split-K reduce instead of an extra fp32 tensor + torch
  // cast kernel per weight per step
  bool wbf = wc.scalar_type() == at::kBFloat16;
  Tensor dw = at::empty({N, K}, wbf ? wc.options() : f32);
  int dw_splits = gemm_tn_tn_splits(N, K, M);
  Tensor dwp = dw_splits > 1
                   ? at::empty({dw_splits, (long)N * K}, f32)
                   : dw;
  CHK(gemm_tn_tn_sk(dyp.data_ptr(),
                    xc.data_ptr(),
                    dw_splits > 1 ? dwp.data_ptr<float>() : nullptr,
                    dw.data_ptr(), N, K, M, Np, K, K, dw_splits, wbf ? 1 : 0,
                    cur_stream()));
  // every colsum path writes all N entries — no zero-init needed
  Tensor db = at::empty({N}, f32);
  int chunks = colsum_chunks(M, N);
  Tensor dbp = chunks > 0 ? at::empty({chunks, (long)N}, f32) : db;
  CHK(colsum_bf16(dyc.data_ptr(), dbp.data_ptr<float>(),
                  db.data_ptr<float>(), M, N, N, cur_stream()));
  return {dx, dw, db};
}

// dx only (side-stream wgrad mode: the main stream runs the dgrad chain
// while linear_wgrad_only runs concurrently on a second stream)
static Tensor linear_dgrad(const Tensor &dy, const Tensor &w) {
  const HIPDeviceGuard guard(dy.device());
  Tensor dyc = dy.contiguous(), wc = w.contiguous();
  int M = dyc.size(0), N = wc.size(0), K = wc.size(1);
  auto f32 = dy.options().dtype(at::kFloat);
  long Np = (N + 7) / 8 * 8;
  Tensor dyp = dyc;
  if (Np != N) {
    dyp = at::zeros({M, Np}, dyc.options());
    dyp.narrow(1, 0, N).copy_(dyc);
  }
  Tensor dx = at::empty({M, K}, dyc.options());
  int dx_splits = gemm_nt_tn_splits(M, K, N);
  Tensor dxp = dx_splits > 1 ? at::empty({dx_splits, (long)M * K}, f32) : dx;
  CHK(gemm_nt_tn_sk(dyp.data_ptr(), wc.data_ptr(),
                    dx_splits > 1 ? dxp.data_ptr<float>() : nullptr,
                    dx.data_ptr(), M, K, N, Np, K, K, dx_splits,
                    cur_stream()));
  return dx;
}

// dx accumulated in place into `acc` (acc += dy @ w) — residual-join
// backward without the separate add pass
static Tensor linear_dgrad_acc(const Tensor &dy, const Tensor &w,
                               Tensor acc) {
  const HIPDeviceGuard guard(dy.device());
  Tensor dyc = dy.contiguous(), wc = w.contiguous();
  int M = dyc.size(0), N = wc.size(0), K = wc.size(1);
  TORCH_CHECK(N % 8 == 0, "linear_dgrad_acc requires out_features %8");
  TORCH_CHECK(acc.is_contiguous() && acc.size(0) == M && acc.size(1) == K);
  CHK(gemm_nt_tn_acc(dyc.data_ptr(), wc.data_ptr(), acc.data_ptr(), M, K, N,
                     N, K, K, cur_stream()));
  return acc;
}

// dw/db only (FFN backward computes fc2's dx separately with the fused
// dgelu epilogue — re-running the full linear_bwd would pay that GEMM twice)
static std::vector<Tensor> linear_wgrad_only(const Tensor &dy,
                                             const Tensor &x) {
  const HIPDeviceGuard guard(x.device());
  Tensor dyc = dy.contiguous(), xc = x.contiguous();
  int M = xc.size(0), K = xc.size(1), N = dyc.size(1);
  auto f32 = x.options().dtype(at::kFloat);
  bool wbf = xc.scalar_type() == at::kBFloat16; // dw matches the weight dtype
  Tensor dw = at::empty({N, K}, wbf ? xc.options() : f32);
  int dw_splits = gemm_tn_tn_splits(N, K, M);
  Tensor dwp =
      dw_splits > 1 ? at::empty({dw_splits, (long)N * K}, f32) : dw;
  CHK(gemm_tn_tn_sk(dyc.data_ptr(), xc.data_ptr(),
                    dw_splits > 1 ? dwp.data_ptr<float>() : nullptr,
                    dw.data_ptr(), N, K, M, N, K, K, dw_splits, wbf ? 1 : 0,
                    cur_stream()));
  Tensor db = at::empty({N}, f32);
  int chunks = colsum_chunks(M, N);
  Tensor dbp = chunks > 0 ? at::empty({chunks, (long)N}, f32) : db;
  CHK(colsum_bf16(dyc.data_ptr(), dbp.data_ptr<float>(),
                  db.data_ptr<float>(), M, N, N, cur_stream()));
  return {dw, db};
}

// ------------------------- fused attention -------------------------
// qkv: [B, S, 3, H, 64] (the fused projection output, untransposed);
// returns (ctx [B, S, H*64], probs [B, H, S, S] for the torch backward)
static std::vector<Tensor> attn_fwd(const Tensor &qkv, int64_t heads,
                                    double scale,
                                    const c10::optional<Tensor> &mask,
                                    bool want_probs) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3 && qkv.size(4) == 64,
              "qkv must be [B,S,3,H,64]");
  TORCH_CHECK(qkv.is_contiguous());
  const HIPDeviceGuard guard(qkv.device());
  int B = qkv.size(0), S = qkv.size(1), H = qkv.size(3);
  TORCH_CHECK(H == heads);
  TORCH_CHECK(S <= 256, "fused attention supports seq <= 256");
  Tensor ctx = at::empty({B, S, (long)H * 64}, qkv.options());
  Tensor probs;
  const float *mp = nullptr;
  Tensor maskc;
  if (mask.has_value()) {
    maskc = mask->to(at::kFloat).contiguous();
    TORCH_CHECK(maskc.numel() == (long)B * S, "mask must be [B,S] additive");
    mp = maskc.data_ptr<float>();
  }
  void *pp = nullptr;
  if (want_probs) {
    probs = at::empty({B, (long)H, S, S}, qkv.options());
    pp = probs.data_ptr();
  }
  CHK(attn_fwd_launch(qkv.data_ptr(), ctx.data_ptr(), pp, mp, B, S, H,
                      (float)scale, cur_stream()));
  if (!want_probs) probs = at::empty({0}, qkv.options());
  return {ctx, probs};
}

static Tensor attn_bwd(const Tensor &qkv, const Tensor &dctx,
                       const Tensor &probs, double scale) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16);
  const HIPDeviceGuard guard(qkv.device());
  int B = qkv.size(0), S = qkv.size(1), H = qkv.size(3);
  TORCH_CHECK(S == 128 && qkv.size(4) == 64, "fused attn bwd: S=128, D=64");
  TORCH_CHECK(qkv.is_contiguous() && probs.is_contiguous());
  Tensor dc = dctx.contiguous();
  Tensor dqkv = at::empty_like(qkv);
  CHK(attn_bwd_launch(qkv.data_ptr(), dc.data_ptr(), probs.data_ptr(),
                      dqkv.data_ptr(), B, S, H, (float)scale, cur_stream()));
  return dqkv;
}

// ------------------- tiled attention (any S, key mask) -------------------
// qkv: [B, S, 3, H, 64]; returns (ctx [B, S, H*64], lse [B, H, S] fp32).
// No probs: the backward recomputes P from lse.
static void flash_check_qkv(const Tensor &qkv, int64_t heads) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3 && qkv.size(4) == 64,
              "qkv must be [B,S,3,H,64]");
  TORCH_CHECK(qkv.is_contiguous());
  TORCH_CHECK(qkv.size(3) == heads);
  TORCH_CHECK(qkv.size(0) >= 1 && qkv.size(1) >= 1);
}

static Tensor flash_mask(const c10::optional<Tensor> &mask, long B, long S) {
  Tensor maskc;
  if (mask.has_value()) {
    maskc = mask->to(at::kFloat).contiguous();
    TORCH_CHECK(maskc.is_cuda() && maskc.numel() == B * S,
                "mask must be [B,S] additive");
  }
  return maskc;
}

static std::vector<Tensor> flash_attn_fwd(const Tensor &qkv, int64_t heads,
                                          double scale,
                                          const c10::optional<Tensor> &mask) {
  flash_check_qkv(qkv, heads);
  const HIPDeviceGuard guard(qkv.device());
  int B = qkv.size(0), S = qkv.size(1), H = qkv.size(3);
  Tensor maskc = flash_mask(mask, B, S);
  Tensor ctx = at::empty({B, S, (long)H * 64}, qkv.options());
  Tensor lse = at::empty({B, (long)H, S}, qkv.options().dtype(at::kFloat));
  CHK(flash_attn_fwd_launch(
      qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr<float>(),
      maskc.defined() ? maskc.data_ptr<float>() : nullptr, B, S, H,
      (float)scale, cur_stream()));
  return {ctx, lse};
}

static Tensor flash_attn_bwd(const Tensor &qkv, const Tensor &ctx,
                             const Tensor &dctx, const Tensor &lse,
                             double scale,
                             const c10::optional<Tensor> &mask) {
  flash_check_qkv(qkv, qkv.dim() == 5 ? qkv.size(3) : 0);
  const HIPDeviceGuard guard(qkv.device());
  int B = qkv.size(0), S = qkv.size(1), H = qkv.size(3);
  TORCH_CHECK(ctx.is_cuda() && ctx.scalar_type() == at::kBFloat16 &&
              ctx.is_contiguous() && ctx.numel() == (long)B * S * H * 64,
              "ctx must be [B,S,H*64] bf16");
  TORCH_CHECK(dctx.is_cuda() && dctx.scalar_type() == at::kBFloat16 &&
              dctx.numel() == ctx.numel(), "dctx must be [B,S,H*64] bf16");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
              lse.is_contiguous() && lse.numel() == (long)B * H * S,
              "lse must be [B,H,S] fp32");
  Tensor maskc = flash_mask(mask, B, S);
  Tensor dc = dctx.contiguous();
  Tensor delta = at::empty_like(lse);
  Tensor dqkv = at::empty_like(qkv);
  CHK(flash_attn_bwd_launch(
      qkv.data_ptr(), ctx.data_ptr(), dc.data_ptr(), lse.data_ptr<float>(),
      delta.data_ptr<float>(),
      maskc.defined() ? maskc.data_ptr<float>() : nullptr, dqkv.data_ptr(), B,
      S, H, (float)scale, cur_stream()));
  return dqkv;
}

// ------------- attention with dropout on the probabilities -------------
// The mask scheme is philox.h's attention scheme (reference.py
// attn_dropout_keep); state is the device (seed, offset) pair.
struct AttnDropShape {
  int B, S, H;
};
static AttnDropShape check_attn_drop_qkv(const Tensor &qkv, int64_t heads,
                                         const char *name) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16, name,
              " must be a bf16 GPU tensor");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3 && qkv.size(4) == 64 &&
                  qkv.size(0) >= 1 && qkv.size(1) >= 1 && qkv.size(3) >= 1,
              name, " must be [B,S,3,H,64], got ", qkv.sizes());
  TORCH_CHECK(qkv.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(heads < 0 || qkv.size(3) == heads, name, " has ", qkv.size(3),
              " heads, expected ", heads);
  TORCH_CHECK(attn_dropout_shape_ok(qkv.size(0), qkv.size(3), qkv.size(1)),
              "attention dropout: B*H*ceil(S/16)*2*S must be below 2^32, got ",
              qkv.sizes());
  return {(int)qkv.size(0), (int)qkv.size(1), (int)qkv.size(3)};
}

static const float *attn_drop_mask(const c10::optional<Tensor> &mask,
                                   const Tensor &like, long B, long S,
                                   Tensor &maskc) {
  if (!mask.has_value()) return nullptr;
  TORCH_CHECK(mask->is_cuda() && mask->device() == like.device() &&
                  mask->numel() == B * S,
              "mask must be an additive [B,S] tensor on qkv's GPU");
  maskc = mask->to(at::kFloat).contiguous();
  return maskc.data_ptr<float>();
}

static void check_attn_ctx(const Tensor &t, const Tensor &qkv,
                           const AttnDropShape &d, const char *name) {
  TORCH_CHECK(t.is_cuda() && t.device() == qkv.device() &&
                  t.scalar_type() == at::kBFloat16 && t.is_contiguous() &&
                  t.numel() == (long)d.B * d.S * d.H * 64,
              name, " must be a contiguous bf16 [B,S,H*64] tensor on qkv's GPU");
}

// returns (ctx [B,S,H*64], signed_probs [B,H,S,S]: bf16(P), sign bit set
// where dropped)
static std::vector<Tensor> attn_drop_fwd_b(const Tensor &qkv, int64_t heads,
                                           double scale,
                                           const c10::optional<Tensor> &mask,
                                           const Tensor &state, double p,
                                           int64_t site) {
  const AttnDropShape d = check_attn_drop_qkv(qkv, heads, "qkv");
  TORCH_CHECK(d.S <= 256, "fused attention supports seq <= 256, got ", d.S);
  check_rng_state(state, qkv);
  const DropParams dp = check_drop_params(p, site);
  const HIPDeviceGuard guard(qkv.device());
  Tensor maskc;
  const float *mp = attn_drop_mask(mask, qkv, d.B, d.S, maskc);
  Tensor ctx = at::empty({d.B, d.S, (long)d.H * 64}, qkv.options());
  Tensor probs = at::empty({d.B, (long)d.H, d.S, d.S}, qkv.options());
  CHK(attn_drop_fwd_launch(qkv.data_ptr(), ctx.data_ptr(), probs.data_ptr(),
                           mp, state.data_ptr<int64_t>(), dp.site, dp.thr,
                           dp.scale, d.B, d.S, d.H, (float)scale,
                           cur_stream()));
  return {ctx, probs};
}

static Tensor attn_drop_bwd_b(const Tensor &qkv, const Tensor &dctx,
                              const Tensor &signed_probs, double scale,
                              double p) {
  const AttnDropShape d = check_attn_drop_qkv(qkv, -1, "qkv");
  TORCH_CHECK(d.S == 128, "fused attention backward: S must be 128, got ",
              d.S);
  check_attn_ctx(dctx, qkv, d, "dctx");
  TORCH_CHECK(signed_probs.is_cuda() &&
                  signed_probs.device() == qkv.device() &&
                  signed_probs.scalar_type() == at::kBFloat16 &&
                  signed_probs.is_contiguous() &&
                  signed_probs.numel() == (long)d.B * d.H * d.S * d.S,
              "signed_probs must be a contiguous bf16 [B,H,S,S] tensor on "
              "qkv's GPU");
  const DropParams dp = check_drop_params(p, 0);
  const HIPDeviceGuard guard(qkv.device());
  Tensor dqkv = at::empty_like(qkv);
  CHK(attn_drop_bwd_launch(qkv.data_ptr(), dctx.data_ptr(),
                           signed_probs.data_ptr(), dqkv.data_ptr(), dp.scale,
                           d.B, d.S, d.H, (float)scale, cur_stream()));
  return dqkv;
}

// returns (ctx [B,S,H*64], lse [B,H,S] fp32 of the UNDROPPED softmax)
static std::vector<Tensor> flash_attn_drop_fwd_b(
    const Tensor &qkv, int64_t heads, double scale,
    const c10::optional<Tensor> &mask, const Tensor &state, double p,
    int64_t site) {
  const AttnDropShape d = check_attn_drop_qkv(qkv, heads, "qkv");
  check_rng_state(state, qkv);
  const DropParams dp = check_drop_params(p, site);
  const HIPDeviceGuard guard(qkv.device());
  Tensor maskc;
  const float *mp = attn_drop_mask(mask, qkv, d.B, d.S, maskc);
  Tensor ctx = at::empty({d.B, d.S, (long)d.H * 64}, qkv.options());
  Tensor lse = at::empty({d.B, (long)d.H, d.S}, qkv.options().dtype(at::kFloat));
  CHK(flash_attn_drop_fwd_launch(qkv.data_ptr(), ctx.data_ptr(),
                                 lse.data_ptr<float>(), mp,
                                 state.data_ptr<int64_t>(), dp.site, dp.thr,
                                 dp.scale, d.B, d.S, d.H, (float)scale,
                                 cur_stream()));
  return {ctx, lse};
}

// state, p, site: what the forward was given (state unchanged since)
static Tensor flash_attn_drop_bwd_b(const Tensor &qkv, const Tensor &ctx,
                                    const Tensor &dctx, const Tensor &lse,
                                    double scale,
                                    const c10::optional<Tensor> &mask,
                                    const Tensor &state, double p,
                                    int64_t site) {
  const AttnDropShape d = check_attn_drop_qkv(qkv, -1, "qkv");
  check_attn_ctx(ctx, qkv, d, "ctx");
  check_attn_ctx(dctx, qkv, d, "dctx");
  TORCH_CHECK(lse.is_cuda() && lse.device() == qkv.device() &&
                  lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
                  lse.numel() == (long)d.B * d.H * d.S,
              "lse must be a contiguous fp32 [B,H,S] tensor on qkv's GPU");
  check_rng_state(state, qkv);
  const DropParams dp = check_drop_params(p, site);
  const HIPDeviceGuard guard(qkv.device());
  Tensor maskc;
  const float *mp = attn_drop_mask(mask, qkv, d.B, d.S, maskc);
  Tensor delta = at::empty_like(lse);
  Tensor dqkv = at::empty_like(qkv);
  CHK(flash_attn_drop_bwd_launch(
      qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr<float>(),
      delta.data_ptr<float>(), mp, state.data_ptr<int64_t>(), dp.site, dp.thr,
      dp.scale, dqkv.data_ptr(), d.B, d.S, d.H, (float)scale, cur_stream()));
  return dqkv;
}

// ------------------ packed (varlen) tiled attention ------------------
// qkv [T,3,H,64]: N sequence slots back to back, cu_seqlens device int32
// [N+1] (cu[0] = 0, non-decreasing, cu[N] <= T, no length above max_seqlen:
// preconditions, never read on the host — nothing here syncs). Returns
// (ctx [T,H*64], lse [H,T] fp32); rows at or past cu[N] are zeros.
struct VarlenShape {
  int N, T, H, max_seqlen;
};
static VarlenShape check_varlen_qkv(const Tensor &qkv, int64_t heads,
                                    const Tensor &cu, int64_t max_seqlen) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16,
              "qkv must be a bf16 GPU tensor");
  TORCH_CHECK(qkv.dim() == 4 && qkv.size(1) == 3 && qkv.size(3) == 64 &&
                  qkv.size(0) >= 1 && qkv.size(2) >= 1,
              "qkv must be [T,3,H,64], got ", qkv.sizes());
  TORCH_CHECK(qkv.is_contiguous(), "qkv must be contiguous");
  TORCH_CHECK(heads < 0 || qkv.size(2) == heads, "qkv has ", qkv.size(2),
              " heads, expected ", heads);
  TORCH_CHECK(qkv.size(0) < (1L << 31), "T must fit an int32");
  TORCH_CHECK(cu.is_cuda() && cu.device() == qkv.device() &&
                  cu.scalar_type() == at::kInt && cu.dim() == 1 &&
                  cu.is_contiguous() && cu.numel() >= 2,
              "cu_seqlens must be a contiguous 1-D int32 tensor of at least "
              "2 elements on qkv's GPU");
  TORCH_CHECK(max_seqlen >= 1 && max_seqlen < (1L << 31),
              "max_seqlen must be a positive int32, got ", max_seqlen);
  long N = cu.numel() - 1;
  TORCH_CHECK(N * qkv.size(2) < (1L << 31), "N*H must fit an int32");
  return {(int)N, (int)qkv.size(0), (int)qkv.size(2), (int)max_seqlen};
}

static void check_varlen_ctx(const Tensor &t, const Tensor &qkv,
                             const VarlenShape &d, const char *name) {
  TORCH_CHECK(t.is_cuda() && t.device() == qkv.device() &&
                  t.scalar_type() == at::kBFloat16 && t.is_contiguous() &&
                  t.numel() == (long)d.T * d.H * 64,
              name, " must be a contiguous bf16 [T,H*64] tensor on qkv's GPU");
}

static void check_varlen_lse(const Tensor &lse, const Tensor &qkv,
                             const VarlenShape &d) {
  TORCH_CHECK(lse.is_cuda() && lse.device() == qkv.device() &&
                  lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
                  lse.numel() == (long)d.H * d.T,
              "lse must be a contiguous fp32 [H,T] tensor on qkv's GPU");
}

static void check_varlen_drop_shape(const VarlenShape &d) {
  TORCH_CHECK(attn_dropout_shape_ok(d.N, d.H, d.max_seqlen),
              "attention dropout: N*H*ceil(max_seqlen/16)*2*max_seqlen must "
              "be below 2^32, got N=", d.N, " H=", d.H, " max_seqlen=",
              d.max_seqlen);
}

static std::vector<Tensor> flash_attn_varlen_fwd(const Tensor &qkv,
                                                 const Tensor &cu_seqlens,
                                                 int64_t max_seqlen,
                                                 int64_t heads, double scale) {
  const VarlenShape d = check_varlen_qkv(qkv, heads, cu_seqlens, max_seqlen);
  const HIPDeviceGuard guard(qkv.device());
  Tensor ctx = at::empty({d.T, (long)d.H * 64}, qkv.options());
  Tensor lse = at::empty({(long)d.H, d.T}, qkv.options().dtype(at::kFloat));
  CHK(flash_attn_varlen_fwd_launch(
      qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr<float>(),
      cu_seqlens.data_ptr<int>(), d.N, d.T, d.max_seqlen, d.H, (float)scale,
      cur_stream()));
  return {ctx, lse};
}

static Tensor flash_attn_varlen_bwd(const Tensor &qkv, const Tensor &ctx,
                                    const Tensor &dctx, const Tensor &lse,
                                    const Tensor &cu_seqlens,
                                    int64_t max_seqlen, double scale) {
  const VarlenShape d = check_varlen_qkv(qkv, -1, cu_seqlens, max_seqlen);
  check_varlen_ctx(ctx, qkv, d, "ctx");
  check_varlen_ctx(dctx, qkv, d, "dctx");
  check_varlen_lse(lse, qkv, d);
  const HIPDeviceGuard guard(qkv.device());
  Tensor delta = at::empty_like(lse);
  Tensor dqkv = at::empty_like(qkv);
  CHK(flash_attn_varlen_bwd_launch(
      qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr<float>(),
      delta.data_ptr<float>(), cu_seqlens.data_ptr<int>(), dqkv.data_ptr(),
      d.N, d.T, d.max_seqlen, d.H, (float)scale, cur_stream()));
  return dqkv;
}

static std::vector<Tensor> flash_attn_varlen_drop_fwd_b(
    const Tensor &qkv, const Tensor &cu_seqlens, int64_t max_seqlen,
    int64_t heads, double scale, const Tensor &state, double p,
    int64_t site) {
  const VarlenShape d = check_varlen_qkv(qkv, heads, cu_seqlens, max_seqlen);
  check_varlen_drop_shape(d);
  check_rng_state(state, qkv);
  const DropParams dp = check_drop_params(p, site);
  const HIPDeviceGuard guard(qkv.device());
  Tensor ctx = at::empty({d.T, (long)d.H * 64}, qkv.options());
  Tensor lse = at::empty({(long)d.H, d.T}, qkv.options().dtype(at::kFloat));
  CHK(flash_attn_varlen_drop_fwd_launch(
      qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr<float>(),
      cu_seqlens.data_ptr<int>(), state.data_ptr<int64_t>(), dp.site, dp.thr,
      dp.scale, d.N, d.T, d.max_seqlen, d.H, (float)scale, cur_stream()));
  return {ctx, lse};
}

// state, p, site: what the forward was given (state unchanged since)
static Tensor flash_attn_varlen_drop_bwd_b(
    const Tensor &qkv, const Tensor &ctx, const Tensor &dctx,
    const Tensor &lse, const Tensor &cu_seqlens, int64_t max_seqlen,
    double scale, const Tensor &state, double p, int64_t site) {
  const VarlenShape d = check_varlen_qkv(qkv, -1, cu_seqlens, max_seqlen);
  check_varlen_drop_shape(d);
  check_varlen_ctx(ctx, qkv, d, "ctx");
  check_varlen_ctx(dctx, qkv, d, "dctx");
  check_varlen_lse(lse, qkv, d);
  check_rng_state(state, qkv);
  const DropParams dp = check_drop_params(p, site);
  const HIPDeviceGuard guard(qkv.device());
  Tensor delta = at::empty_like(lse);
  Tensor dqkv = at::empty_like(qkv);
  CHK(flash_attn_varlen_drop_bwd_launch(
      qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr<float>(),
      delta.data_ptr<float>(), cu_seqlens.data_ptr<int>(),
      state.data_ptr<int64_t>(), dp.site, dp.thr, dp.scale, dqkv.data_ptr(),
      d.N, d.T, d.max_seqlen, d.H, (float)scale, cur_stream()));
  return dqkv;
}

// ------------------------- fused FFN (GELU) -------------------------
// fc1 forward with the bias+GELU in the epilogue: returns (g, h_pre)
static std::vector<Tensor> linear_gelu_fwd(const Tensor &x, const Tensor &w,
                                           const Tensor &b) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous());
  const HIPDeviceGuard guard(x.device());
  int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K);
  Tensor bias = b.to(at::kFloat).contiguous();
  Tensor g = at::empty({M, N}, x.options());
  Tensor deriv = at::empty({M, N}, x.options()); // gelu'(h), for backward
  CHK(gemm_nt_gelu_bias(x.data_ptr(), w.data_ptr(), bias.data_ptr<float>(),
                        deriv.data_ptr(), g.data_ptr(), M, N, K, K, K, N,
                        cur_stream()));
  return {g, deriv};
}

// fc2-dx with dgelu fused: dh = (dy·w2) ⊙ gelu'(h_pre)
static Tensor linear_gelu_dgrad(const Tensor &dy, const Tensor &w,
                                const Tensor &pre) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16);
  TORCH_CHECK(dy.is_contiguous() && w.is_contiguous() && pre.is_contiguous());
  const HIPDeviceGuard guard(dy.device());
  int M = dy.size(0), K = dy.size(1), N = w.size(1);
  TORCH_CHECK(pre.size(0) == M && pre.size(1) == N);
  Tensor dh = at::empty({M, N}, dy.options());
  Tensor wt; // w^T scratch: unlocks the NT pipe256 route on full-tile shapes
  void *wtp = nullptr;
  if (gemm_gelubwd_wants_wt(M, N, K)) {
    wt = at::empty({N, K}, dy.options());
    wtp = wt.data_ptr();
  }
  CHK(gemm_nt_tn_gelubwd(dy.data_ptr(), w.data_ptr(), pre.data_ptr(),
                         dh.data_ptr(), M, N, K, K, N, N, wtp, cur_stream()));
  return dh;
}

// ------------------------- softmax xent -------------------------
static std::vector<Tensor> softmax_xent_fwd(const Tensor &logits,
                                            const Tensor &target) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16);
  const HIPDeviceGuard guard(logits.device());
  int B = logits.size(0), V = logits.size(1);
  auto f32 = logits.options().dtype(at::kFloat);
  Tensor probs = at::empty({B, V}, f32);
  Tensor loss = at::empty({}, f32);
  CHK(softmax_xent_fwd_launch(logits.data_ptr(), target.data_ptr<long>(),
                              probs.data_ptr<float>(), loss.data_ptr<float>(),
                              B, V, cur_stream()));
  return {loss, probs};
}

static Tensor softmax_xent_bwd(const Tensor &probs, const Tensor &target,
                               const Tensor &dloss) {
  const HIPDeviceGuard guard(probs.device());
  int B = probs.size(0), V = probs.size(1);
  TORCH_CHECK(dloss.is_cuda() && dloss.scalar_type() == at::kFloat &&
              dloss.numel() == 1, "dloss must be a device fp32 scalar");
  Tensor d = at::empty({B, V}, probs.options().dtype(at::kBFloat16));
  CHK(softmax_xent_bwd_launch(probs.data_ptr<float>(), target.data_ptr<long>(),
                              d.data_ptr(), B, V, dloss.data_ptr<float>(),
                              cur_stream()));
  return d;
}

// MLM masked CE: fwd reads bf16 logits once, saves [B][2] stats + the
// (loss_sum, valid_count) pair; bwd recomputes probs from the bf16 logits
// (no fp32 probs materialization — 4× less HBM at vocab scale).
static std::vector<Tensor> masked_xent_fwd(const Tensor &logits,
                                           const Tensor &target,
                                           int64_t ignore_index) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16);
  TORCH_CHECK(logits.is_contiguous());
  const HIPDeviceGuard guard(logits.device());
  int B = logits.size(0), V = logits.size(1);
  auto f32 = logits.options().dtype(at::kFloat);
  Tensor stats = at::empty({B, 2}, f32);
  Tensor out = at::empty({2}, f32); // loss_sum, valid_count
  CHK(masked_xent_fwd_launch(logits.data_ptr(), target.data_ptr<long>(),
                             stats.data_ptr<float>(), out.data_ptr<float>(),
                             B, V, V, ignore_index, cur_stream()));
  return {out, stats};
}

static Tensor masked_xent_bwd(const Tensor &logits, const Tensor &target,
                              const Tensor &stats, const Tensor &out,
                              const Tensor &dloss, int64_t ignore_index) {
  const HIPDeviceGuard guard(logits.device());
  int B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(dloss.is_cuda() && dloss.scalar_type() == at::kFloat &&
              dloss.numel() == 1, "dloss must be a device fp32 scalar");
  Tensor d = at::empty({B, V}, logits.options());
  CHK(masked_xent_bwd_launch(logits.data_ptr(), target.data_ptr<long>(),
                             stats.data_ptr<float>(), out.data_ptr<float>(),
                             dloss.data_ptr<float>(), d.data_ptr(), B, V, V,
                             ignore_index, cur_stream()));
  return d;
}

// --------------- fused MLM head: decoder GEMM + masked CE ---------------
// The decoder writes logits into a [M][Vp] padded-vocab buffer (Vp =
// roundup(V, 8)); CE reads rows with stride Vp; backward re-derives
// probabilities into a padded dlogits whose pad columns the kernel zeroes,
// so the dx/dw GEMMs and db colsum consume it DIRECTLY (lda = Vp) — no
// per-step [M][Vp] zero-fill + strided pad copy (prof8: ~180 us/step), and
// no unpadded fp32/bf16 logits round-trips. Reference role: the MLM
// pretraining head of the out-of-tree BERT images.
static std::vector<Tensor> mlm_head_fwd(const Tensor &h, const Tensor &w,
                                        const Tensor &b, const Tensor &target,
                                        int64_t ignore_index) {
  TORCH_CHECK(h.is_cuda() && h.scalar_type() == at::kBFloat16 && h.dim() == 2);
  TORCH_CHECK(h.is_contiguous() && w.is_contiguous());
  TORCH_CHECK(b.scalar_type() == at::kFloat, "mlm bias must be fp32");
  const HIPDeviceGuard guard(h.device());
  int M = h.size(0), K = h.size(1), V = w.size(0);
  TORCH_CHECK(w.size(1) == K && target.numel() == M);
  long Vp = ((long)V + 7) / 8 * 8;
  auto f32 = h.options().dtype(at::kFloat);
  Tensor logits = at::empty({M, Vp}, h.options());
  Tensor bc = b.contiguous();
  CHK(gemm_nt_bias(h.data_ptr(), w.data_ptr(), bc.data_ptr<float>(),
                   logits.data_ptr(), M, V, K, K, K, Vp, cur_stream()));
  Tensor stats = at::empty({M, 2}, f32);
  Tensor out = at::empty({2}, f32); // loss_sum, valid_count
  CHK(masked_xent_fwd_launch(logits.data_ptr(), target.data_ptr<long>(),
                             stats.data_ptr<float>(), out.data_ptr<float>(),
                             M, V, Vp, ignore_index, cur_stream()));
  return {out, logits, stats};
}

static std::vector<Tensor> mlm_head_bwd(const Tensor &logits, int64_t V64,
                                        const Tensor &target,
                                        const Tensor &stats, const Tensor &out,
                                        const Tensor &dloss, const Tensor &h,
                                        const Tensor &w, int64_t ignore_index) {
  const HIPDeviceGuard guard(h.device());
  int M = logits.size(0), V = (int)V64, K = h.size(1);
  long Vp = logits.size(1);
  TORCH_CHECK(dloss.is_cuda() && dloss.scalar_type() == at::kFloat &&
              dloss.numel() == 1, "dloss must be a device fp32 scalar");
  auto f32 = h.options().dtype(at::kFloat);
  Tensor dlog = at::empty_like(logits);
  CHK(masked_xent_bwd_launch(logits.data_ptr(), target.data_ptr<long>(),
                             stats.data_ptr<float>(), out.data_ptr<float>(),
                             dloss.data_ptr<float>(), dlog.data_ptr(), M, V,
                             Vp, ignore_index, cur_stream()));
  // dh = dlog . w (reduce over padded vocab; pads are zero)
  Tensor dh = at::empty({M, K}, h.options());
  int dx_splits = gemm_nt_tn_splits(M, K, V);
  Tensor dhp = dx_splits > 1 ? at::empty({dx_splits, (long)M * K}, f32) : dh;
  CHK(gemm_nt_tn_sk(dlog.data_ptr(), w.data_ptr(),
                    dx_splits > 1 ? dhp.data_ptr<float>() : nullptr,
                    dh.data_ptr(), M, K, V, Vp, K, K, dx_splits,
                    cur_stream()));
  // dw (tied embedding grad) in the weight dtype straight from the GEMM
  bool wbf = w.scalar_type() == at::kBFloat16;
  Tensor dw = at::empty({(long)V, K}, wbf ? w.options() : f32);
  int dw_splits = gemm_tn_tn_splits(V, K, M);
  Tensor dwp = dw_splits > 1 ? at::empty({dw_splits, (long)V * K}, f32) : dw;
  CHK(gemm_tn_tn_sk(dlog.data_ptr(), h.data_ptr(),
                    dw_splits > 1 ? dwp.data_ptr<float>() : nullptr,
                    dw.data_ptr(), V, K, M, Vp, K, K, dw_splits, wbf ? 1 : 0,
                    cur_stream()));
  // db over the PADDED width: pads are zero, so summing Vp columns keeps
  // the %8-vectorized colsum8 slab path (the ragged V route ran 2-B scalar
  // loads at ~4x off bandwidth); the bias grad is the leading V entries
  Tensor db_pad = at::empty({Vp}, f32);
  int chunks = colsum_chunks(M, (int)Vp);
  Tensor dbp = chunks > 0 ? at::empty({chunks, Vp}, f32) : db_pad;
  CHK(colsum_bf16(dlog.data_ptr(), dbp.data_ptr<float>(),
                  db_pad.data_ptr<float>(), M, (int)Vp, Vp, cur_stream()));
  return {dh, dw, db_pad.narrow(0, 0, V)};
}

// ------------------------- add-relu -------------------------
// The elementwise kernels index every operand with one linear octet index:
// all operands must be dense bf16 GPU tensors of one shape and one memory
// layout, with a whole number of 8-element octets.
static void check_ew_first(const Tensor &t, const char *name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, name,
              " must be a bf16 GPU tensor");
  TORCH_CHECK(t.is_contiguous() ||
                  (t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast)),
              name, " must be contiguous or 4-D channels_last");
  TORCH_CHECK(t.numel() % 8 == 0, name,
              ": element count must be a multiple of 8, got ", t.numel());
}

static void check_ew_same(const Tensor &t, const Tensor &first,
                          const char *name) {
  TORCH_CHECK(t.is_cuda() && t.device() == first.device() &&
                  t.scalar_type() == at::kBFloat16,
              name, " must be a bf16 tensor on the first operand's GPU");
  // size-1 dims make strides ambiguous, so compare formats, not strides
  const bool cl = first.dim() == 4 &&
                  first.is_contiguous(at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(t.sizes() == first.sizes() &&
                  (cl ? t.is_contiguous(at::MemoryFormat::ChannelsLast)
                      : t.is_contiguous()),
              name, " must have the first operand's shape and memory layout (",
              first.sizes(), "), got ", t.sizes());
}

static Tensor add_relu_fwd_b(const Tensor &a, const Tensor &b) {
  check_cl_bf16(a, "a");
  check_ew_first(a, "a");
  check_ew_same(b, a, "b");
  const HIPDeviceGuard guard(a.device());
  Tensor y = at::empty_like(a);
  CHK(add_relu_fwd(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), cur_stream()));
  return y;
}

static Tensor add_relu_bwd_b(const Tensor &dy, const Tensor &y) {
  check_ew_first(dy, "dy");
  check_ew_same(y, dy, "y");
  const HIPDeviceGuard guard(dy.device());
  Tensor dx = at::empty_like(dy);
  CHK(add_relu_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dy.numel(), cur_stream()));
  return dx;
}

static Tensor add_relu_bwd_add_b(const Tensor &dy, const Tensor &y,
                                 const Tensor &dx0) {
  check_ew_first(dy, "dy");
  check_ew_same(y, dy, "y");
  check_ew_same(dx0, dy, "dx0");
  const HIPDeviceGuard guard(dy.device());
  Tensor out = at::empty_like(dx0);
  CHK(add_relu_bwd_add(dy.data_ptr(), y.data_ptr(), dx0.data_ptr(),
                       out.data_ptr(), dy.numel(), cur_stream()));
  return out;
}

// join backward off the bn relu-mask (1 byte per 8 channels): dxt =
// dx0 + dy·mask — drops the full y re-read
static Tensor add_relu_bwd_add_mask_b(const Tensor &dy, const Tensor &mask,
                                      const Tensor &dx0) {
  check_ew_first(dy, "dy");
  check_ew_same(dx0, dy, "dx0");
  check_relu_mask(mask, dy.numel() / 8, "mask");
  const HIPDeviceGuard guard(dy.device());
  Tensor out = at::empty_like(dx0);
  CHK(add_relu_bwd_add_mask(dy.data_ptr(), mask.data_ptr(), dx0.data_ptr(),
                            out.data_ptr(), dy.numel(), cur_stream()));
  return out;
}

// ------------------------- sgd -------------------------
static void sgd_step(std::vector<Tensor> masters, std::vector<Tensor> grads,
                     std::vector<Tensor> momenta, std::vector<Tensor> outs,
                     double lr, double mu, double wd, bool nesterov) {
  TORCH_CHECK(!masters.empty());
  const HIPDeviceGuard guard(masters[0].device());
  std::vector<SgdDesc> by_dtype[2]; // 0: f32 grads, 1: bf16 grads
  for (size_t i = 0; i < masters.size(); ++i) {
    SgdDesc d;
    d.grad = grads[i].data_ptr();
    d.master = masters[i].data_ptr<float>();
    d.mom = momenta[i].data_ptr<float>();
    d.out = outs[i].numel() > 0 ? (uint16_t *)outs[i].data_ptr() : nullptr;
    d.numel = masters[i].numel();
    by_dtype[grads[i].scalar_type() == at::kBFloat16 ? 1 : 0].push_back(d);
  }
  for (int t = 0; t < 2; ++t)
    if (!by_dtype[t].empty())
      CHK(sgd_step_launch(by_dtype[t].data(), (int)by_dtype[t].size(), t,
                          (float)lr, (float)mu, (float)wd, nesterov ? 1 : 0,
                          cur_stream()));
}

// ------------------------- adamw / lamb -------------------------
// Descriptors grouped by grad dtype (0: f32, 1: bf16), as sgd_step does.
// Every stream of a tensor must be dense with the param's numel: the kernels
// index all of them with one linear offset.
struct OptGroups {
  std::vector<OptDesc> by_dtype[2];
  int blocks = 0;  // partials-slab slots the whole list needs
  int tensors = 0;
};

static OptGroups opt_groups(const std::vector<Tensor> &masters,
                            const std::vector<Tensor> &grads,
                            const std::vector<Tensor> &exp_avgs,
                            const std::vector<Tensor> &exp_avg_sqs,
                            const std::vector<Tensor> &outs,
                            const Tensor &scalars) {
  size_t n = masters.size();
  TORCH_CHECK(n > 0 && grads.size() == n && exp_avgs.size() == n &&
              exp_avg_sqs.size() == n && outs.size() == n,
              "optimizer step: tensor lists must be non-empty and equal length");
  TORCH_CHECK(scalars.is_cuda() && scalars.scalar_type() == at::kFloat &&
              scalars.is_contiguous() && scalars.numel() >= 8,
              "optimizer step: scalar block must be >= 8 fp32 on GPU");
  OptGroups g;
  for (size_t i = 0; i < n; ++i) {
    const Tensor &w = masters[i], &gr = grads[i], &m = exp_avgs[i],
                 &v = exp_avg_sqs[i], &o = outs[i];
    const int64_t ne = w.numel();
    const bool gbf = gr.scalar_type() == at::kBFloat16;
    TORCH_CHECK(w.is_cuda() && gr.is_cuda() && m.is_cuda() && v.is_cuda(),
                "optimizer step: tensors must be on GPU");
    TORCH_CHECK(w.scalar_type() == at::kFloat && m.scalar_type() == at::kFloat &&
                v.scalar_type() == at::kFloat &&
                (gbf || gr.scalar_type() == at::kFloat),
                "optimizer step: master/exp_avg/exp_avg_sq fp32, grad fp32 or bf16");
    TORCH_CHECK(gr.numel() == ne && m.numel() == ne && v.numel() == ne &&
                w.is_non_overlapping_and_dense() &&
                gr.is_non_overlapping_and_dense() &&
                m.is_non_overlapping_and_dense() &&
                v.is_non_overlapping_and_dense(),
                "optimizer step: tensor ", i, " streams must be dense and equal-sized");
    OptDesc d;
    d.grad = gr.data_ptr();
    d.master = w.data_ptr<float>();
    d.m = m.data_ptr<float>();
    d.v = v.data_ptr<float>();
    d.out = nullptr;
    if (o.numel() > 0) {
      TORCH_CHECK(o.is_cuda() && o.scalar_type() == at::kBFloat16 &&
                  o.numel() == ne && o.is_non_overlapping_and_dense(),
                  "optimizer step: working copy ", i, " must be dense bf16");
      d.out = (uint16_t *)o.data_ptr();
    }
    d.numel = ne;
    g.by_dtype[gbf ? 1 : 0].push_back(d);
  }
  for (int t = 0; t < 2; ++t) {
    g.blocks += optim_block_count(g.by_dtype[t].data(), (int)g.by_dtype[t].size());
    g.tensors += (int)g.by_dtype[t].size();
  }
  return g;
}

static void check_slab(const Tensor &t, int64_t need, const char *name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
              t.is_contiguous() && t.numel() >= need,
              "optimizer step: ", name, " must hold >= ", need, " fp32 on GPU");
}

// grad-norm partials (only when clipping) and the step-state tick
static void opt_tick(const OptGroups &g, const Tensor &scalars,
                     const Tensor &partials, double beta1, double beta2,
                     double max_grad_norm) {
  const bool clip = max_grad_norm > 0.0;
  if (clip) {
    check_slab(partials, g.blocks, "partials");
    int base = 0;
    for (int t = 0; t < 2; ++t) {
      const auto &v = g.by_dtype[t];
      if (v.empty()) continue;
      CHK(l2norm_partials_launch(v.data(), (int)v.size(), t,
                                 partials.data_ptr<float>(), base, cur_stream()));
      base += optim_block_count(v.data(), (int)v.size());
    }
  }
  CHK(optim_tick_launch(scalars.data_ptr<float>(),
                        clip ? partials.data_ptr<float>() : nullptr, g.blocks,
                        beta1, beta2, clip ? max_grad_norm : 0.0, cur_stream()));
}

static void adam_step(std::vector<Tensor> masters, std::vector<Tensor> grads,
                      std::vector<Tensor> exp_avgs,
                      std::vector<Tensor> exp_avg_sqs, std::vector<Tensor> outs,
                      Tensor scalars, Tensor partials, double beta1,
                      double beta2, double eps, double wd, bool adam_w_mode,
                      double max_grad_norm) {
  TORCH_CHECK(!masters.empty());
  const HIPDeviceGuard guard(masters[0].device());
  OptGroups g = opt_groups(masters, grads, exp_avgs, exp_avg_sqs, outs, scalars);
  opt_tick(g, scalars, partials, beta1, beta2, max_grad_norm);
  for (int t = 0; t < 2; ++t)
    if (!g.by_dtype[t].empty())
      CHK(adam_step_launch(g.by_dtype[t].data(), (int)g.by_dtype[t].size(), t,
                           scalars.data_ptr<float>(), beta1, beta2, eps, wd,
                           adam_w_mode ? 1 : 0, cur_stream()));
}

// partials: 3 slabs of `blocks` slots (grad norm | sum w^2 | sum u^2);
// ratio: one slot per tensor
static void lamb_step(std::vector<Tensor> masters, std::vector<Tensor> grads,
                      std::vector<Tensor> exp_avgs,
                      std::vector<Tensor> exp_avg_sqs, std::vector<Tensor> outs,
                      Tensor scalars, Tensor partials, Tensor ratio,
                      double beta1, double beta2, double eps, double wd,
                      bool adam_w_mode, double max_grad_norm) {
  TORCH_CHECK(!masters.empty());
  const HIPDeviceGuard guard(masters[0].device());
  OptGroups g = opt_groups(masters, grads, exp_avgs, exp_avg_sqs, outs, scalars);
  check_slab(partials, 3 * (int64_t)g.blocks, "partials");
  check_slab(ratio, g.tensors, "ratio");
  opt_tick(g, scalars, partials, beta1, beta2, max_grad_norm);
  float *pw = partials.data_ptr<float>() + g.blocks;
  float *pu = pw + g.blocks;
  int block_base = 0, tensor_base = 0;
  for (int t = 0; t < 2; ++t) {
    const auto &v = g.by_dtype[t];
    if (v.empty()) continue;
    CHK(lamb_step_launch(v.data(), (int)v.size(), t, scalars.data_ptr<float>(),
                         pw, pu, block_base, ratio.data_ptr<float>(),
                         tensor_base, beta1, beta2, eps, wd,
                         adam_w_mode ? 1 : 0, cur_stream()));
    block_base += optim_block_count(v.data(), (int)v.size());
    tensor_base += (int)v.size();
  }
}

// ------------------------- raw gemm (tests) -------------------------
static Tensor gemm_nt_b(const Tensor &a, const Tensor &b, bool c_f32) {
  const HIPDeviceGuard guard(a.device());
  Tensor ac = a.contiguous(), bc = b.contiguous();
  int M = ac.size(0), K = ac.size(1), N = bc.size(0);
  TORCH_CHECK(bc.size(1) == K);
  TORCH_CHECK(K % 8 == 0, "gemm_nt requires K%8==0");
  Tensor c = at::empty({M, N}, ac.options().dtype(c_f32 ? at::kFloat : at::kBFloat16));
  CHK(gemm_nt(ac.data_ptr(), bc.data_ptr(), c.data_ptr(), M, N, K, K, K, N,
              c_f32 ? 1 : 0, cur_stream()));
  return c;
}

// ------------------- route introspection (host only) -------------------
// Resolved value of every C++ MPIAMD_* knob: the knobs.h functions the
// launchers themselves call (inline, so one static per process). Touches no
// device.
static py::dict route_info() {
  py::dict d;
  d["pipemix"] = use_pipemix();
  d["pipe8"] = use_pipe8();
  d["p256x16"] = use_p256x16();
  d["gemm256"] = use_gemm256();
  d["pipe"] = use_pipe();
  d["pipent"] = use_pipent();
  d["glds"] = use_glds();
  d["onebuf"] = use_onebuf();
  d["splitmajor"] = use_splitmajor();
  d["sk_cpx"] = use_sk_cpx();
  d["fwd_sk"] = fwd_sk_on();
  d["dx_sk"] = dx_sk_mode(); // -1 shape-aware default, 0 never, 1 always
  d["linear_sk"] = linear_sk_on();
  d["gelu_deriv"] = gelu_deriv_mode();
  d["gelubwd_wt"] = gelubwd_wt_on();
  d["pipegather"] = use_pipegather();
  d["pipegather_wgrad"] = use_pipegather_wgrad();
  d["pipes2"] = use_pipes2();
  d["ln_spec"] = ln_spec();
  d["ln2"] = ln2_mode();
  d["bn_grid"] = bn_grid_cap();
  d["bn_apply_grid"] = bn_apply_grid_cap();
  d["conv_splits_force"] = conv_splits_force(); // -1 = heuristic
  d["wgrad_budget"] = wgrad_budget();
  return d;
}

static const char *nt_route(int M, int N, int K, int splits) {
  static const char *const names[] = {"pipe256", "nt256", "pipemix", "glds",
                                      "reg"};
  int r = gemm_nt_route_id(M, N, K, splits);
  TORCH_CHECK(r >= 0 && r < 5, "unknown NT route id ", r);
  return names[r];
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("route_info", &route_info);
  m.def("nt_route", &nt_route, py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("splits") = 1);
  // 16-byte-store GEMM epilogue on/off for the whole process; returns the
  // previous value (A/B lever and the tests' scalar reference)
  m.def("set_epilogue_vec",
        [](bool on) { return gemm_set_epilogue_vec(on ? 1 : 0) != 0; });
  // software-pipelined BN statistics producers / line-coalesced BN finalize
  // on/off for the whole process; each returns the previous value (A/B
  // levers and the tests' reference: the kernels they replace)
  m.def("set_bn_pipelined",
        [](bool on) { return bn_set_pipelined(on ? 1 : 0) != 0; });
  m.def("set_bn_finalize_coalesced",
        [](bool on) { return bn_set_finalize_coalesced(on ? 1 : 0) != 0; });
  // finalize slice width override for tools/bn_bench.py: 0 the built-in
  // table, -1 the bands kernel, 8 or 16 that width; returns the previous one
  m.def("set_bn_finalize_ch", [](int ch) {
    int prev = bn_set_finalize_ch(ch);
    TORCH_CHECK(prev != -2, "set_bn_finalize_ch: ch must be 0, -1, 8 or 16");
    return prev;
  });
  // does the fc2-dx GEMM of dy [M][K] · w2 [K][N] take the transpose-plus-
  // pipe256 route (MPIAMD_GELUBWD_WT)? The route's own predicate.
  m.def("gelubwd_wt_route", [](int M, int N, int K) {
    return gemm_gelubwd_wants_wt(M, N, K) != 0;
  });
  // split counts as conv2d_fwd / conv2d_dgrad (reduce extent K, before the
  // launcher's clamp to K's 64-deep tiles) and conv2d_wgrad resolve them
  m.def("conv_splits", [](int64_t M, int Ncols, int K) {
    return conv_splits((long)M, Ncols, K);
  }, py::arg("M"), py::arg("Ncols"), py::arg("K"));
  m.def("conv_wgrad_splits", [](int Kout, int RSC, int64_t M) {
    return wgrad_splits(Kout, RSC, (long)M);
  }, py::arg("Kout"), py::arg("RSC"), py::arg("M"));
  m.def("conv2d_fwd", &conv2d_fwd);
  m.def("conv2d_dgrad", &conv2d_dgrad);
  m.def("conv2d_fwd_bn", &conv2d_fwd_bn, py::arg("x"), py::arg("w"),
        py::arg("stride"), py::arg("pad"), py::arg("fuse_splitk") = true,
        py::arg("fuse_epilogue") = true);
  m.def("conv2d_dgrad_bn", &conv2d_dgrad_bn);
  m.def("bn_bwd_pre", &bn_bwd_pre);
  m.def("join_bwd_stats", &join_bwd_stats);
  m.def("bn_fwd_train_pre", &bn_fwd_train_pre);
  m.def("conv2d_wgrad", &conv2d_wgrad);
  m.def("conv2d_dgrad_acc", &conv2d_dgrad_acc);
  m.def("add_bf16", &add_bf16_b);
  m.def("bn_fwd_train", &bn_fwd_train);
  m.def("bn_fwd_eval", &bn_fwd_eval);
  m.def("bn_bwd", &bn_bwd);
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("gap_fwd", &gap_fwd_b);
  m.def("gap_bwd", &gap_bwd_b);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("layernorm_add_fwd", &layernorm_add_fwd);
  m.def("rng_tick", &rng_tick_b);
  m.def("dropout_fwd", &dropout_fwd_b, py::arg("x"), py::arg("state"),
        py::arg("p"), py::arg("site"));
  m.def("dropout_bwd", &dropout_bwd_b, py::arg("dy"), py::arg("mask"),
        py::arg("p"));
  m.def("layernorm_drop_add_fwd", &layernorm_drop_add_fwd, py::arg("a"),
        py::arg("b"), py::arg("gamma"), py::arg("beta"), py::arg("eps"),
        py::arg("state"), py::arg("p"), py::arg("site"));
  m.def("layernorm_drop_add_bwd", &layernorm_drop_add_bwd, py::arg("dy"),
        py::arg("s"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"),
        py::arg("mask"), py::arg("p"));
  m.def("linear_fwd", &linear_fwd);
  m.def("linear_bwd", &linear_bwd);
  m.def("linear_dgrad", &linear_dgrad);
  m.def("linear_dgrad_acc", &linear_dgrad_acc);
  m.def("softmax_xent_fwd", &softmax_xent_fwd);
  m.def("masked_xent_fwd", &masked_xent_fwd);
  m.def("mlm_head_fwd", &mlm_head_fwd);
  m.def("mlm_head_bwd", &mlm_head_bwd);
  m.def("linear_gelu_fwd", &linear_gelu_fwd);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("flash_attn_fwd", &flash_attn_fwd);
  m.def("flash_attn_bwd", &flash_attn_bwd);
  m.def("attn_drop_fwd", &attn_drop_fwd_b, py::arg("qkv"), py::arg("heads"),
        py::arg("scale"), py::arg("mask"), py::arg("state"), py::arg("p"),
        py::arg("site"));
  m.def("attn_drop_bwd", &attn_drop_bwd_b, py::arg("qkv"), py::arg("dctx"),
        py::arg("signed_probs"), py::arg("scale"), py::arg("p"));
  m.def("flash_attn_drop_fwd", &flash_attn_drop_fwd_b, py::arg("qkv"),
        py::arg("heads"), py::arg("scale"), py::arg("mask"), py::arg("state"),
        py::arg("p"), py::arg("site"));
  m.def("flash_attn_drop_bwd", &flash_attn_drop_bwd_b, py::arg("qkv"),
        py::arg("ctx"), py::arg("dctx"), py::arg("lse"), py::arg("scale"),
        py::arg("mask"), py::arg("state"), py::arg("p"), py::arg("site"));
  m.def("flash_attn_varlen_fwd", &flash_attn_varlen_fwd, py::arg("qkv"),
        py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("heads"),
        py::arg("scale"));
  m.def("flash_attn_varlen_bwd", &flash_attn_varlen_bwd, py::arg("qkv"),
        py::arg("ctx"), py::arg("dctx"), py::arg("lse"),
        py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("scale"));
  m.def("flash_attn_varlen_drop_fwd", &flash_attn_varlen_drop_fwd_b,
        py::arg("qkv"), py::arg("cu_seqlens"), py::arg("max_seqlen"),
        py::arg("heads"), py::arg("scale"), py::arg("state"), py::arg("p"),
        py::arg("site"));
  m.def("flash_attn_varlen_drop_bwd", &flash_attn_varlen_drop_bwd_b,
        py::arg("qkv"), py::arg("ctx"), py::arg("dctx"), py::arg("lse"),
        py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("scale"),
        py::arg("state"), py::arg("p"), py::arg("site"));
  m.def("linear_wgrad_only", &linear_wgrad_only);
  m.def("linear_gelu_dgrad", &linear_gelu_dgrad);
  m.def("masked_xent_bwd", &masked_xent_bwd);
  m.def("softmax_xent_bwd", &softmax_xent_bwd);
  m.def("add_relu_fwd", &add_relu_fwd_b);
  m.def("add_relu_bwd", &add_relu_bwd_b);
  m.def("add_relu_bwd_add", &add_relu_bwd_add_b);
  m.def("add_relu_bwd_add_mask", &add_relu_bwd_add_mask_b);
  m.def("sgd_step", &sgd_step);
  m.def("adam_step", &adam_step);
  m.def("lamb_step", &lamb_step);
  m.def("gemm_nt", &gemm_nt_b);
  m.def("mfma_probe", [](const Tensor &a, const Tensor &b) {
    const HIPDeviceGuard guard(a.device());
    Tensor d = at::empty({16, 16}, a.options().dtype(at::kFloat));
    CHK(mfma_probe(a.contiguous().data_ptr(), b.contiguous().data_ptr(),
                   d.data_ptr<float>(), cur_stream()));
    return d;
  });
}
