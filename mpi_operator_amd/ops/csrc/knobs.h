// The one definition of every MPIAMD_* environment knob of the C++ side.
// Host only. Each knob is read once per process into a function-local
// static of an inline function, so the launchers in every TU and
// route_info() in bindings.cpp call the very same function and see the very
// same value. docs/tuning.md carries one table row per knob;
// tests/test_knob_routes.py takes the knob names from the knob_*("MPIAMD_…")
// calls below.
#pragma once

#include <climits>
#include <cstdlib>

// the only getenv of csrc/
inline const char *knob_env(const char *name) { return getenv(name); }

// flag that is ON unless the value starts with '0'
inline bool knob_on(const char *name) {
  const char *e = knob_env(name);
  return !(e && e[0] == '0');
}

// flag that is OFF unless the value starts with '1'
inline bool knob_off(const char *name) {
  const char *e = knob_env(name);
  return e && e[0] == '1';
}

// integer within [lo, hi], else (unset, unparsable, out of range) `fallback`
inline int knob_int(const char *name, long lo, long hi, int fallback) {
  const char *e = knob_env(name);
  long v = e ? atol(e) : lo - 1;
  return (v >= lo && v <= hi) ? (int)v : fallback;
}

// ---- pipe_mix.h: the 128²-tile deep pipeline and its gather routes -------

// MPIAMD_PIPEMIX=0 reverts every pipe_mix route to the round-1 register-
// staged mix_gemm tile (A/B lever).
inline bool use_pipemix() {
  static const bool on = knob_on("MPIAMD_PIPEMIX");
  return on;
}

// The conv GATHER routes measured net-negative on the 4-WAVE pipeline
// (3296 vs 3390 same-box), but the verdict REVERSED under the 8-wave
// kernel: 3742 -> 3820 img/s ResNet101 / 6508 ResNet50 same-box — the
// extra VALU of the gather ptr16 hides behind the doubled wave count.
// Default ON; MPIAMD_PIPEGATHER=0 reverts to the register-staged mix
// gathers.
inline bool use_pipegather() {
  static const bool on = knob_on("MPIAMD_PIPEGATHER");
  return use_pipemix() && on;
}

// wgrad-only override: the -2.9% PIPEGATHER measurement bundled fwd/dgrad
// and wgrad gathers; A/B'd alone the Xcol wgrad pipe WINS (3566 -> 3573
// img/s ResNet101, 6129 ResNet50 same-box) — default ON.
// The three gates nest: MPIAMD_PIPEMIX=0 reverts everything,
// MPIAMD_PIPEGATHER=0 reverts the fwd, dgrad AND wgrad gathers, and
// MPIAMD_PIPEGATHER_WGRAD=0 reverts the wgrad gather alone to the
// register-staged mix gather. (Until PIPEGATHER defaulted on this was
// `(pipemix && wgrad) || pipegather`, which made WGRAD=0 a no-op and left
// wgrad on the pipe under PIPEGATHER=0.)
inline bool use_pipegather_wgrad() {
  static const bool on = knob_on("MPIAMD_PIPEGATHER_WGRAD");
  return use_pipegather() && on;
}

// Stride-2 dgrad parity GEMMs on the pipe (conv.hip conv_dgrad_s2);
// MPIAMD_PIPES2=0 keeps them on DgradS2Stage while every other gather
// stays on the pipe (A/B lever).
inline bool use_pipes2() {
  static const bool on = knob_on("MPIAMD_PIPES2");
  return use_pipegather() && on;
}

// XCD fold also applies under split-K: the 2-D grid dispatches x-fastest,
// so within each split slice consecutive tile ids still round-robin the
// XCDs and the fold restores contiguous tile bands per XCD L2.
// MPIAMD_SK_CPX=0 restores the old splits==1-only gate for A/B.
inline bool use_sk_cpx() {
  static const bool on = knob_on("MPIAMD_SK_CPX");
  return on;
}

// Default ON: same-box A/B with the 8-wave kernel on every pipe route —
// BERT-Large bs32 1421 -> 1468 seq/s, bs8 607 -> 684, ResNet101
// 3560 -> 3697 img/s. The extra waves (16/CU vs 8 at the same 64 KiB LDS
// footprint) buy more than the duplicated B-frag LDS reads cost.
// MPIAMD_PIPE8=0 reverts to the 4-wave kernel.
inline bool use_pipe8() {
  static const bool on = knob_on("MPIAMD_PIPE8");
  return on;
}

// ---- pipe256.h ------------------------------------------------------------

// Default ON: +0.4% same-box on BOTH models (BERT 1513->1520 seq/s,
// ResNet101 3812->3829 img/s). MPIAMD_P256X16=0 reverts to 8 waves.
inline bool use_p256x16() {
  static const bool on = knob_on("MPIAMD_P256X16");
  return on;
}

// ---- mix_gemm.h: the register-staged tile and the NT route choice --------

// MPIAMD_SPLITMAJOR=1: split-major dispatch of the mix split-K grid.
// default OFF: the standalone-harness win (+16-28% on synthetic TnTn
// wgrad shapes) did not transfer to the full model (-0.4% same-box on the
// bench) — real wgrads gather B via XcolStage and use smaller splits
inline bool use_splitmajor() {
  static const bool on = knob_off("MPIAMD_SPLITMAJOR");
  return on;
}

// MPIAMD_GEMM_ONEBUF=1: single-LDS-buffer mix tile (register-staged
// operands only, see launch_mix_gemm_wr). Default OFF.
inline bool use_onebuf() {
  static const bool on = knob_off("MPIAMD_GEMM_ONEBUF");
  return on;
}

// MPIAMD_GEMM256=0: no 256²-tile family (128² everywhere).
inline bool use_gemm256() {
  static const bool on = knob_on("MPIAMD_GEMM256");
  return on;
}

// 4-phase deep pipeline (pipe256.h) for K%64 full-tile shapes;
// MPIAMD_PIPE=0 reverts to the round-1 BK=32 3-buffer kernel (gemm256.h)
inline bool use_pipe() {
  static const bool on = knob_on("MPIAMD_PIPE");
  return on;
}

// MPIAMD_PIPENT=0 reverts just the NT 128² pipe fallback (bisect lever).
inline bool use_pipent() {
  static const bool on = knob_on("MPIAMD_PIPENT");
  return on;
}

// MPIAMD_GLDS=0: register-staged loads instead of global_load_lds in the
// mix tile.
inline bool use_glds() {
  static const bool on = knob_on("MPIAMD_GLDS");
  return on;
}

// ---- gemm.hip: linear-layer split-K and GELU routes -----------------------

// Forward split-K (fc2-class M=4096/N=1024 shapes give 256 pipe-mix
// workgroups = exactly 1/CU, half the block slots idle; deep K amortizes
// the fp32 slab + bias-reduce pass). Measured same-box +0.7% on BERT-Large
// bs32 (1372 -> 1381): default ON, MPIAMD_FWD_SK=0 disables. Heuristic
// shared with the dw path.
inline bool fwd_sk_on() {
  static const bool on = knob_on("MPIAMD_FWD_SK");
  return on;
}

// MPIAMD_GELU_DERIV (default 1): fwd saves gelu'(h) so bwd is exp-free;
// =0 restores the save-pre/recompute-tanh pair for A/B.
inline bool gelu_deriv_mode() {
  static const bool on = knob_on("MPIAMD_GELU_DERIV");
  return on;
}

// MPIAMD_GELUBWD_WT=1: fc2-dx via transpose + pipe256. Default OFF; the
// measured verdict sits at gemm.hip gemm_gelubwd_wants_wt.
inline bool gelubwd_wt_on() {
  static const bool on = knob_off("MPIAMD_GELUBWD_WT");
  return on;
}

// dx split-K, SHAPE-aware after three verdict flips: under the 8-wave
// pipeline a 256-workgroup dx grid fills the chip and the slab+reduce tax
// loses (bs32: 1542 with splits vs 1553 without), but SMALL grids still
// need it badly (bs8's 64-wg dx: 690 with splits vs 614 without; so does
// bert-base's 192-wg grid). Split only when tiles < 256.
// MPIAMD_DX_SK: 0 = never split, 1 = always use the dw heuristic.
inline int dx_sk_mode() { // -1 = shape-aware default
  static const int mode =
      knob_env("MPIAMD_DX_SK") ? (knob_off("MPIAMD_DX_SK") ? 1 : 0) : -1;
  return mode;
}

// split-K of the weight-gradient GEMM (gemm.hip gemm_tn_tn_splits): default
// ON, MPIAMD_LINEAR_SK=0 disables.
inline bool linear_sk_on() {
  static const bool on = knob_on("MPIAMD_LINEAR_SK");
  return on;
}

// ---- layernorm.hip ---------------------------------------------------------

// LN C8 specialization: same-box A/B at BERT-Large bs32 showed the
// compile-time octet loops LOSE 2.4% (1384 vs 1415; ln_bwd_dx 15.5->24.1
// us) — the unrolled form costs more than the runtime loop at M=4096
// despite lower VGPRs. Default OFF; MPIAMD_LN_SPEC=1 enables for
// small-shape A/Bs.
inline bool ln_spec() {
  static const bool on = knob_off("MPIAMD_LN_SPEC");
  return on;
}

// MPIAMD_LN2=1: 2-row-interleaved dx kernel (ln_bwd_dx2_k) for N <= 1024
// (A/B lever). Default OFF.
inline bool ln2_mode() {
  static const bool on = knob_off("MPIAMD_LN2");
  return on;
}

// ---- batchnorm.hip ---------------------------------------------------------

// Partials grid cap: 512 measured best THREE times now — flat 1024 lost
// 6.6%, and the channel-aware cap (up to 4096 bands for narrow layers)
// lost 4.4% (3363 vs 3517 same-box) even with the bands finalize: the
// deeper slab costs more in finalize reads + L2 pressure than the extra
// partials parallelism buys. MPIAMD_BN_GRID overrides within [1, 8192] for
// A/Bs; the launchers and the bindings' slab allocation both call this.
inline int bn_grid_cap() {
  static const int cap = knob_int("MPIAMD_BN_GRID", 1, 8192, 512);
  return cap;
}

// cap 2048 measured best (3846-3854 vs 3833-3834 img/s at 4096, 3800
// at 8192, four-sample same-box sweep); MPIAMD_BN_APPLY_GRID overrides
// within [64, 16384]
inline int bn_apply_grid_cap() {
  static const int cap = knob_int("MPIAMD_BN_APPLY_GRID", 64, 16384, 2048);
  return cap;
}

// ---- bindings.cpp: conv split counts ---------------------------------------

// MPIAMD_CONV_SPLITS=n (n >= 1) forces the conv fwd/dgrad split count;
// -1 = the heuristic (bindings.cpp conv_splits).
inline int conv_splits_force() {
  static const int force = knob_int("MPIAMD_CONV_SPLITS", 1, INT_MAX, -1);
  return force;
}

// target-block budget of the conv-wgrad split count (conv2d_wgrad);
// MPIAMD_WGRAD_BUDGET overrides within [64, 2048] for A/B (default 512)
inline int wgrad_budget() {
  static const int budget = knob_int("MPIAMD_WGRAD_BUDGET", 64, 2048, 512);
  return budget;
}
