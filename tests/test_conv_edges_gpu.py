"""conv2d fwd / dgrad / wgrad (and the accumulating 1x1 dgrad) per element
against fp64, at the geometries where the implicit GEMM's index arithmetic
can go wrong: H != W, R != S, pad above the half-kernel, even and 5x5
kernels, every stride-2 parity layout (1, 2 and 4 live parities, live parity
(1,1)), tiles that straddle images, images with an odd pixel count (the wgrad
odd/even pixel carry), C/8 no power of two, a ragged k-tile, a second column
tile of 8, split-K in fwd/dgrad/wgrad, stride 3 and a single output pixel.

Each comparison is |out - ref| <= 2^-8 |ref| + n 2^-24 T per element, with the
references, T and n of conv_refs.py (derived, not measured; elements no term
reaches must be exactly 0). tests/test_conv_refs_cpu.py shows that this bound
passes torch's fp32 convolution rounded once and fails a dropped border tap,
exchanged H/W or R/S, pad-1, a stale or unwritten dx row, a missing split-K
slab and a wgrad pixel from the wrong image. Outputs are NaN-poisoned (best
effort, see conv_refs.poison) before every call.

Worst observed |out - ref| / bound over all cases of this file on an MI355X
(1.0 = at the bound), first run, bounds as derived:

  output        rel     abs_i              worst ratio
  conv.y        2^-8    R*S*C 2^-24 T      0.990
  conv.dx       2^-8    R*S*Kout 2^-24 T   0.985
  conv.dw       2^-8    N*HO*WO 2^-24 T    0.990
  conv.dx_acc   2^-8    (Kout+1) 2^-24 T   0.985

As with the streaming kernels the bf16 outputs sit just under 1: half a bf16
ulp is 2^-8 of a value at the bottom of its binade, and among thousands of
elements one is nearly there; the fp32 sum's share of the bound is barely
used. The whole file (19 tests) took 2.3 s wall in that run, 1.5 s of it the
first case's cold extension load; no other case took more than 0.1 s.

Before the fix that came with this file, k1x1-s2-p1 failed: conv_dgrad_s2 sent
every single-live-parity shape to Stride2ZeroWriter, which clears the
siblings at (h+1, w+1) and so, with the live parity at (1,1), never wrote row
0 and column 0 of dx (512 of 2240 elements read back the NaN poison).
"""
import functools

import pytest
import torch

import conv_refs as cr
from conv_refs import CASES, REL_BF16

pytestmark = pytest.mark.gpu

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def ext():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def check_out(out, shape, ref, abs_i, name):
    assert tuple(out.shape) == tuple(shape), (name, out.shape, shape)
    assert out.dtype == torch.bfloat16, (name, out.dtype)
    assert out.is_contiguous(memory_format=torch.channels_last), name
    cr.assert_close(out, ref, REL_BF16, abs_i, name)


def expect_splits(M, ncols, K, heuristic):
    """The fwd/dgrad split count this process resolves for a GEMM of M rows,
    ncols columns and reduce extent K: the forced count under
    MPIAMD_CONV_SPLITS, else the heuristic's, which must be `heuristic`."""
    force = ext().route_info()["conv_splits_force"]
    got = ext().conv_splits(M, ncols, K)
    assert got == (force if force >= 1 else heuristic), (got, force, heuristic)


@pytest.mark.parametrize("name", list(CASES))
def test_conv_edges(name):
    e = ext()
    r = cr.case_refs(name)
    N, C, H, W, K, R, S, st, pad = geom = r["geom"]
    HO, WO = cr.out_hw(geom)
    x, w, dy = r["x"].to(DEV), r["w"].to(DEV), r["dy"].to(DEV)

    if name == "splitk":  # the heuristic halves K in fwd and in dgrad
        assert cr.conv_splits_model(N * HO * WO, K, R * S * C) == 2
        expect_splits(N * HO * WO, K, R * S * C, 2)
        expect_splits(N * H * W, C, R * S * K, 2)
    if name == "wgrad-8way" and e.route_info()["wgrad_budget"] == 512:
        assert e.conv_wgrad_splits(K, R * S * C, N * HO * WO) == 8

    cr.poison((N, K, HO, WO), x)
    y = e.conv2d_fwd(x, w, st, pad)
    check_out(y, (N, K, HO, WO), r["y"], r["y_abs"], f"conv.y[{name}]")

    if name in cr.NO_DGRAD:
        with pytest.raises(RuntimeError, match="stride 1 or 2"):
            e.conv2d_dgrad(dy, w, H, W, st, pad)
    else:
        cr.poison((N, C, H, W), x)
        dx = e.conv2d_dgrad(dy, w, H, W, st, pad)
        check_out(dx, (N, C, H, W), r["dx"], r["dx_abs"], f"conv.dx[{name}]")

    cr.poison((K, C, R, S), x)
    dw = e.conv2d_wgrad(x, dy, R, S, st, pad)
    check_out(dw, (K, C, R, S), r["dw"], r["dw_abs"], f"conv.dw[{name}]")


def test_conv_dgrad_acc():
    N, C, H, W, K = cr.ACC_GEOM
    dy = cr.rand_bf16((N, K, H, W), 7, device=DEV)
    w = cr.rand_bf16((K, C, 1, 1), 8, scale=0.5, device=DEV)
    dx0 = cr.rand_bf16((N, C, H, W), 9, device=DEV)
    ref, abs_i = cr.dgrad_acc_ref(dy, w, dx0)
    dx = dx0.clone(memory_format=torch.preserve_format)
    ext().conv2d_dgrad_acc(dy, w, dx)
    check_out(dx, (N, C, H, W), ref, abs_i, "conv.dx_acc")
    assert not torch.equal(dx, dx0)


# ------------------------------------------------------ argument checks
def _bad_calls():
    """Calls every conv entry point must refuse. Each is either refused by
    the per-binding checks that preceded check_conv_geometry (C % 8 through
    conv2d_fwd, channel mismatch, Kout % 8 and stride 0 / 3 through
    conv2d_dgrad), or mismatched in the direction in which a kernel launched
    regardless would stay inside its buffers: the tensor whose extent the
    launcher takes is the smaller one, and the gathers bounds-check H and W."""
    e = ext()

    def t(*shape, seed=60):
        return cr.rand_bf16(shape, seed, device=DEV)

    x16, x12 = t(2, 16, 6, 5), t(2, 12, 6, 5)
    w16, w12, w8 = t(24, 16, 3, 3), t(24, 12, 3, 3), t(24, 8, 3, 3)
    dy24 = t(2, 24, 6, 5)        # the 3x3 stride-1 pad-1 output of x16
    dy12, wq12 = t(2, 12, 6, 5), t(12, 16, 3, 3)
    dy_s2 = t(2, 24, 3, 3)       # 3x3 stride-2 pad-1 output of 6x5
    dy_more = t(3, 24, 6, 5)     # wgrad takes N from x: dy rows 0..2*30 read
    dy_low = t(2, 24, 5, 5)      # HO one short of the formula's 6
    w_more = t(32, 16, 3, 3)     # dgrad takes Kout from dy: rows 0..23 read
    w1, w1_more = t(24, 16, 1, 1), t(32, 16, 1, 1)
    acc, acc_more = t(2, 16, 6, 5), t(3, 16, 6, 5)
    v16 = torch.ones(16, device=DEV)
    eu8 = torch.empty(0, dtype=torch.uint8, device=DEV)

    def dgrad_bn(stride):
        return e.conv2d_dgrad_bn(dy_s2 if stride != 1 else dy24, w16, 6, 5,
                                 stride, 1, x16, x16, v16, v16, True, eu8)

    return [
        ("fwd-C12", lambda: e.conv2d_fwd(x12, w12, 1, 1)),
        ("fwd-w-channels", lambda: e.conv2d_fwd(x16, w8, 1, 1)),
        ("fwd_bn-C12", lambda: e.conv2d_fwd_bn(x12, w12, 1, 1, False, False)),
        ("dgrad-stride0", lambda: e.conv2d_dgrad(dy24, w16, 6, 5, 0, 1)),
        ("dgrad-stride3", lambda: e.conv2d_dgrad(dy_s2, w16, 6, 5, 3, 1)),
        ("dgrad_bn-stride3", lambda: dgrad_bn(3)),
        ("dgrad-Kout12", lambda: e.conv2d_dgrad(dy12, wq12, 6, 5, 1, 1)),
        ("dgrad-w-more-Kout", lambda: e.conv2d_dgrad(dy24, w_more, 6, 5, 1, 1)),
        ("dgrad-HO-small", lambda: e.conv2d_dgrad(dy_low, w16, 6, 5, 1, 1)),
        ("wgrad-dy-more-images", lambda: e.conv2d_wgrad(x16, dy_more, 3, 3, 1, 1)),
        ("wgrad-HO-small", lambda: e.conv2d_wgrad(x16, dy_low, 3, 3, 1, 1)),
        ("dgrad_acc-dy-fewer-images",
         lambda: e.conv2d_dgrad_acc(dy24, w1, acc_more)),
        ("dgrad_acc-w-more-Kout", lambda: e.conv2d_dgrad_acc(dy24, w1_more, acc)),
    ]


def test_conv_bindings_reject_bad_arguments():
    accepted = []
    for name, call in _bad_calls():
        try:
            call()
        except RuntimeError:
            continue
        accepted.append(name)
    torch.cuda.synchronize()
    assert not accepted, f"accepted without an error: {accepted}"
