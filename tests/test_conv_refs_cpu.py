"""The convolution tests, tested (no GPU): for every geometry of
conv_refs.CASES the unfold-based fp64 references must agree with torch's own
convolutions in fp64, a correct low-precision implementation (torch's fp32
convolution of the bf16 inputs, rounded once to bf16) must pass the
per-element bound, and the subtly wrong results a broken index computation
would give must fail it: a dropped border tap, H and W exchanged in the
gather, pad-1, R and S exchanged, a stale uncovered dx row, an unwritten dx
row, a missing split-K slab, a wgrad pixel taken from the wrong image.
test_geometries_keep_their_edges pins what each geometry is there to reach."""
import pytest
import torch

import conv_refs as cr
import stream_refs as sr
from conv_refs import CASES, REL_BF16

F = torch.nn.functional
G = torch.nn.grad
NAMES = list(CASES)


def passes(out, ref, abs_i, rel=REL_BF16):
    return sr.check_close(out, ref, rel, abs_i, "t")[0]


def honest(name):
    """torch's fp32 convolutions of the bf16 inputs: (y, dx, dw) in fp32."""
    r = cr.case_refs(name)
    N, C, H, W, K, R, S, st, pad = r["geom"]
    x, w, dy = r["x"].float(), r["w"].float(), r["dy"].float()
    y = F.conv2d(x, w, stride=st, padding=pad)
    dx = G.conv2d_input((N, C, H, W), w, dy, stride=st, padding=pad)
    dw = G.conv2d_weight(x, (K, C, R, S), dy, stride=st, padding=pad)
    return y, dx, dw


# ---- an fp32 implicit GEMM by index arithmetic, the way the stagers gather:
# cols[n, (ho,wo), (r,s,c)] = x[n, h, w, c] or 0, with the knobs a wrong
# kernel would have
def gather_cols(x, geom, swap_hw=False, pad_eff=None, swap_rs=False):
    N, C, H, W, K, R, S, st, pad = geom
    HO, WO = cr.out_hw(geom)
    pe = pad if pad_eff is None else pad_eff
    Hb, Wb = (W, H) if swap_hw else (H, W)  # extents the gather believes in
    xf = x.float().permute(0, 2, 3, 1).reshape(N, H * W, C)
    ho = torch.arange(HO)[:, None]
    wo = torch.arange(WO)[None, :]
    cols = []
    for t in range(R * S):
        r, s = divmod(t, R) if swap_rs else divmod(t, S)
        h, w_ = ho * st - pe + r, wo * st - pe + s
        ok = ((h >= 0) & (h < Hb) & (w_ >= 0) & (w_ < Wb)).reshape(-1)
        idx = (h * Wb + w_).clamp(0, H * W - 1).reshape(-1)
        cols.append(xf[:, idx] * ok[None, :, None])
    return torch.cat(cols, 2)  # [N, HO*WO, R*S*C]


def w_rsc(w):
    return w.float().permute(0, 2, 3, 1).reshape(w.shape[0], -1)  # [K, (r,s,c)]


def fwd_gemm(x, w, geom, k_end=None, **kw):
    N, C, H, W, K, R, S, st, pad = geom
    HO, WO = cr.out_hw(geom)
    cols, wm = gather_cols(x, geom, **kw), w_rsc(w)
    y = cols[..., :k_end] @ wm[:, :k_end].t()  # [N, L, K]
    return y.permute(0, 2, 1).reshape(N, K, HO, WO)


def is_gather(geom):
    N, C, H, W, K, R, S, st, pad = geom
    return not (R == 1 and S == 1 and st == 1 and pad == 0)


# --------------------------------------------------- 1. the reference itself
@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_torch_fp64(name):
    r = cr.case_refs(name)
    N, C, H, W, K, R, S, st, pad = r["geom"]
    x, w, dy = r["x"].double(), r["w"].double(), r["dy"].double()
    want = dict(
        y=F.conv2d(x, w, stride=st, padding=pad),
        dx=G.conv2d_input((N, C, H, W), w, dy, stride=st, padding=pad),
        dw=G.conv2d_weight(x, (K, C, R, S), dy, stride=st, padding=pad))
    for key, t in want.items():
        assert r[key].shape == t.shape and r[key].dtype == torch.float64
        err = float((r[key] - t).abs().max())
        assert err <= 1e-12 * max(float(t.abs().max()), 1e-300), (key, err)
        # T dominates |ref| and is 0 exactly where no term reaches
        n = cr.summands(r["geom"])[key]
        T = r[key + "_abs"] / (n * cr.U32)
        assert bool((T >= r[key].abs() * (1 - 1e-12)).all()), key
        assert bool((r[key][T == 0] == 0).all()), key


# --------------------------------------- 2. a correct implementation passes
@pytest.mark.parametrize("name", NAMES)
def test_fp32_conv_rounded_once_passes(name):
    r = cr.case_refs(name)
    y, dx, dw = honest(name)
    for key, t in (("y", y), ("dx", dx), ("dw", dw)):
        ok, worst, msg = sr.check_close(sr.bf16r(t), r[key], REL_BF16,
                                        r[key + "_abs"], f"{key}[{name}]")
        assert ok, msg
        # an fp32 output is held to the absolute part alone
        ok, worst, msg = sr.check_close(t, r[key], 0, r[key + "_abs"],
                                        f"{key}.f32[{name}]")
        assert ok, msg
    # so does the index-arithmetic GEMM the mutants below are cut from
    yg = fwd_gemm(r["x"], r["w"], r["geom"])
    assert passes(sr.bf16r(yg), r["y"], r["y_abs"]), name


def test_dgrad_acc_reference():
    N, C, H, W, K = cr.ACC_GEOM
    dy = cr.rand_bf16((N, K, H, W), 7)
    w = cr.rand_bf16((K, C, 1, 1), 8, scale=0.5)
    dx0 = cr.rand_bf16((N, C, H, W), 9)
    ref, abs_i = cr.dgrad_acc_ref(dy, w, dx0)
    good = dx0.float() + G.conv2d_input((N, C, H, W), w.float(), dy.float())
    assert passes(sr.bf16r(good), ref, abs_i)
    # the accumulation forgotten, or done on a rounded dgrad
    assert not passes(sr.bf16r(good - dx0.float()), ref, abs_i)
    twice = sr.bf16r(sr.bf16r(good - dx0.float()).float() + dx0.float())
    assert not passes(twice, ref, abs_i)


# ----------------------------------------------------- 3. the mutants fail
def failing(mutant, applies):
    """Names of the applicable geometries on which `mutant(name)` (a list of
    (out, ref, abs_i)) misses the bound; every applicable one is tried."""
    names = [n for n in NAMES if applies(CASES[n])]
    assert names, "mutant applies to no geometry"
    bad = []
    for n in names:
        if not all(passes(o, ref, a) for o, ref, a in mutant(n)):
            bad.append(n)
    return names, bad


def test_mutant_dropped_border_tap():
    def mutant(name):
        r = cr.case_refs(name)
        N, C, H, W, K, R, S, st, pad = r["geom"]
        HO, WO = cr.out_hw(r["geom"])
        y = honest(name)[0].clone()
        x, w = r["x"].float(), r["w"].float()
        border = [(ho, wo) for ho in range(HO) for wo in range(WO)
                  if ho in (0, HO - 1) or wo in (0, WO - 1)]
        for ho, wo in border:
            taps = [(rr, ss) for rr in range(R) for ss in range(S)
                    if 0 <= ho * st - pad + rr < H and 0 <= wo * st - pad + ss < W]
            if taps:
                rr, ss = taps[0]
                h, w_ = ho * st - pad + rr, wo * st - pad + ss
                y[0, :, ho, wo] -= w[:, :, rr, ss] @ x[0, :, h, w_]
                return [(sr.bf16r(y), r["y"], r["y_abs"])]
        raise AssertionError(f"{name}: no border pixel with a live tap")

    names, bad = failing(mutant, lambda g: True)
    assert bad == names, set(names) - set(bad)


def test_mutant_h_w_exchanged():
    def mutant(name):
        r = cr.case_refs(name)
        y = fwd_gemm(r["x"], r["w"], r["geom"], swap_hw=True)
        return [(sr.bf16r(y), r["y"], r["y_abs"])]

    names, bad = failing(mutant, lambda g: g[2] != g[3] and is_gather(g))
    assert bad == names, set(names) - set(bad)
    assert {"nonsq-3x3", "nonsq-3x3-s2"} <= set(names)


def test_mutant_pad_minus_one():
    def mutant(name):
        r = cr.case_refs(name)
        y = fwd_gemm(r["x"], r["w"], r["geom"], pad_eff=r["geom"][8] - 1)
        return [(sr.bf16r(y), r["y"], r["y_abs"])]

    names, bad = failing(mutant, lambda g: g[8] >= 1)
    assert bad == names, set(names) - set(bad)


def test_mutant_r_s_exchanged():
    def mutant(name):
        r = cr.case_refs(name)
        y = fwd_gemm(r["x"], r["w"], r["geom"], swap_rs=True)
        return [(sr.bf16r(y), r["y"], r["y_abs"])]

    names, bad = failing(mutant, lambda g: g[5] != g[6])
    assert bad == names and len(names) >= 3, (names, bad)


def test_mutant_stale_last_dx_row():
    def mutant(name):
        r = cr.case_refs(name)
        dx = sr.bf16r(honest(name)[1]).clone()
        dx[:, :, -1, :] = 2.0 ** -7
        return [(dx, r["dx"], r["dx_abs"])]

    names, bad = failing(mutant, lambda g: g[7] == 2)
    assert bad == names, set(names) - set(bad)
    assert "k2x2-s2" in bad


def test_mutant_unwritten_dx_row0():
    name = "k1x1-s2-p1"
    r = cr.case_refs(name)
    dx = sr.bf16r(honest(name)[1]).clone()
    assert passes(dx, r["dx"], r["dx_abs"])
    # row 0 and column 0 belong to dead parities: exactly 0 is required
    assert float(r["dx"][:, :, 0, :].abs().max()) == 0.0
    assert float(r["dx_abs"][:, :, 0, :].abs().max()) == 0.0
    dx[:, :, 0, :] = float("nan")
    assert not passes(dx, r["dx"], r["dx_abs"])


def test_mutant_split_k_slab_omitted():
    name = "splitk"
    r = cr.case_refs(name)
    N, C, H, W, K, R, S, st, pad = r["geom"]
    nk = (R * S * C + 63) // 64
    assert cr.conv_splits_model(N * H * W, K, R * S * C) == 2 and nk % 2 == 0
    full = fwd_gemm(r["x"], r["w"], r["geom"])
    assert passes(sr.bf16r(full), r["y"], r["y_abs"])
    half = fwd_gemm(r["x"], r["w"], r["geom"], k_end=nk // 2 * 64)
    assert not passes(sr.bf16r(half), r["y"], r["y_abs"])


def test_mutant_wgrad_pixel_from_wrong_image():
    """The pixel after an image boundary (ho = wo = 0 of image 1) gathered
    with the carry into n missed: its patch comes from image 0."""
    def mutant(name):
        r = cr.case_refs(name)
        N, C, H, W, K, R, S, st, pad = r["geom"]
        cols = gather_cols(r["x"], r["geom"])  # [N, L, RSC]
        dym = r["dy"].float().reshape(N, K, -1)
        assert passes(sr.bf16r(torch.einsum("nkl,nlj->kj", dym, cols)
                               .reshape(K, R, S, C).permute(0, 3, 1, 2)),
                      r["dw"], r["dw_abs"]), name
        cols = cols.clone()
        cols[1, 0] = cols[0, 0]
        dw = torch.einsum("nkl,nlj->kj", dym, cols)
        dw = dw.reshape(K, R, S, C).permute(0, 3, 1, 2)
        return [(sr.bf16r(dw), r["dw"], r["dw_abs"])]

    # where pad >= R or S the first pixel's window is all padding either way
    names, bad = failing(
        mutant, lambda g: g[0] >= 2 and g[8] < g[5] and g[8] < g[6])
    assert bad == names, set(names) - set(bad)
    assert "nonsq-3x3" in bad and "wgrad-8way" in bad


# ------------------------------------------- 4. what each geometry reaches
def test_geometries_keep_their_edges():
    g = CASES
    hw = {n: cr.out_hw(g[n]) for n in g}
    pix = {n: hw[n][0] * hw[n][1] for n in g}
    M = {n: g[n][0] * pix[n] for n in g}

    # every case is tiny: one test stays far below a second of GPU work
    assert all(M[n] * g[n][5] * g[n][6] * g[n][1] * g[n][4] < 2 ** 26 for n in g)

    n = "nonsq-3x3"
    N, C, H, W, K, R, S, st, pad = g[n]
    assert H != W and M[n] == 351 and M[n] % 128 and M[n] > 128
    assert pix[n] == 117 and pix[n] % 2 == 1 and pix[n] < 128 < 2 * pix[n]
    assert K < 128 and N >= 3

    n = "nonsq-3x3-s2"
    N, C, H, W, K, R, S, st, pad = g[n]
    assert st == 2 and hw[n] == (7, 5) and pix[n] == 35
    assert len(cr.live_parities(g[n])) == 4
    assert {(H - p + 1) // 2 for p in (0, 1)}.isdisjoint(
        {(W - p + 1) // 2 for p in (0, 1)})  # H2 != W2 for every parity pair

    for n, (rr, ss) in (("k1x3", (1, 3)), ("k3x1", (3, 1))):
        N, C, H, W, K, R, S, st, pad = g[n]
        assert (R, S) == (rr, ss) and H != W
        assert pad > (min(R, S) - 1) // 2
    # first and last output row (column) of k1x3 (k3x1) see only padding
    assert float(cr.case_refs("k1x3")["y_abs"][:, :, (0, -1), :].max()) == 0.0
    assert float(cr.case_refs("k3x1")["y_abs"][:, :, :, (0, -1)].max()) == 0.0
    assert g["k1x3"][2:4] == g["k3x1"][2:4][::-1]

    assert g["k5x5"][5:7] == (5, 5) and g["k5x5"][2] != g["k5x5"][3]
    assert g["k3x3-p0"][8] == 0 and g["k3x3-p0"][5] == 3
    n = "k3x3-p2"
    assert g[n][8] > (g[n][5] - 1) // 2
    assert hw[n][0] > g[n][2] and hw[n][1] > g[n][3]

    n = "k1x1-s2"
    assert g[n][5:9] == (1, 1, 2, 0) and g[n][2] % 2 == 0 and g[n][3] % 2 == 1
    assert cr.live_parities(g[n]) == [(0, 0)]
    n = "k1x1-s2-p1"
    assert g[n][5:9] == (1, 1, 2, 1) and cr.live_parities(g[n]) == [(1, 1)]
    assert g[n][:5] == g["k1x1-s2"][:5]

    n = "k2x2-s2"
    N, C, H, W, K, R, S, st, pad = g[n]
    assert R % 2 == 0 and S % 2 == 0 and st == 2
    assert len(cr.live_parities(g[n])) == 4
    assert (hw[n][0] - 1) * st - pad + R - 1 < H - 1  # no window covers row H-1
    assert float(cr.case_refs(n)["dx_abs"][:, :, -1, :].max()) == 0.0

    n = "k1x3-s2"
    assert g[n][7] == 2 and len(cr.live_parities(g[n])) == 2

    n = "splitk"
    N, C, H, W, K, R, S, st, pad = g[n]
    assert R * S * C == 1152 and H != W
    assert cr.conv_splits_model(M[n], K, R * S * C) == 2          # fwd
    assert cr.conv_splits_model(N * H * W, C, R * S * K) == 2     # dgrad

    n = "c24-k136"
    N, C, H, W, K, R, S, st, pad = g[n]
    c8 = C // 8
    assert C % 8 == 0 and c8 & (c8 - 1) and C & (C - 1)
    assert R * S * C == 216 and (R * S * C) % 64
    assert K == 128 + 8

    n = "s3"
    assert g[n][7] == 3 and n in cr.NO_DGRAD
    assert [k for k in g if g[k][7] not in (1, 2)] == list(cr.NO_DGRAD)

    n = "wgrad-8way"
    N, C, H, W, K, R, S, st, pad = g[n]
    assert M[n] == 4495 and M[n] % 2 == 1 and (M[n] + 63) // 64 == 71
    assert M[n] % 64 and pix[n] % 2 == 1
    assert cr.wgrad_splits_model(K, R * S * C, M[n]) == 8
    assert 71 % 8  # the splits do not share the k-tiles evenly

    assert M["one-pixel-3x3"] == 1 and M["one-pixel-1x1"] == 1
    assert g["one-pixel-3x3"][5] == 3 and g["one-pixel-1x1"][5] == 1

    # an image with an odd pixel count: the wgrad odd/even carry crosses it
    assert sum(pix[k] % 2 == 1 and g[k][0] >= 2 for k in g) >= 3
    # every dgrad-able case is stride 1 or 2 and every C, Kout is whole octets
    assert all(g[k][1] % 8 == 0 and g[k][4] % 8 == 0 for k in g)

    N, C, H, W, K = cr.ACC_GEOM
    assert (N, C, H, W, K) == (3, 16, 9, 13, 24) and (N * H * W) % 2 == 1
