"""The streaming-kernel tests, tested: on small odd-M shapes the fp32 torch
implementation of each operation (rounded to bf16, the E[x^2] - mean^2
variance the kernels use) must pass the fp64 references and bounds of
stream_refs.py, and the subtly wrong results a broken row geometry would give
must fail them: the last row left unwritten, one 8-channel octet zeroed, the
second-to-last row gated by the last row's mask byte, running_var without
M/(M-1), the max-pool scatter sent to window position idx+1."""
import pytest
import torch

import stream_refs as sr
from stream_refs import REL_BF16

EPS, MOM = 1e-5, 0.3
SHAPE = (3, 24, 5, 7)  # M = 105 (odd), C8 = 3
F = torch.nn.functional


def c_(v):
    return v[None, :, None, None]


def params(C, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    rm0 = torch.randn(C, generator=g)
    rv0 = torch.rand(C, generator=g) + 0.5
    return gamma, beta, rm0, rv0


def bn_fwd_f32(x, gamma, beta, relu, res, rm0, rv0, unbiased=True):
    d = (0, 2, 3)
    xf = x.float()
    M = xf.numel() // xf.shape[1]
    mean = xf.mean(d)
    var = ((xf * xf).mean(d) - mean * mean).clamp_min(0)
    invstd = (var + EPS).rsqrt()
    scale = gamma * invstd
    shift = beta - mean * scale
    f = xf * c_(scale) + c_(shift)
    if res is not None:
        f = f + res.float()
    if relu:
        f = f.clamp_min(0)
    unbias = M / (M - 1) if unbiased else 1.0
    rm = rm0 * (1 - MOM) + mean * MOM
    rv = rv0 * (1 - MOM) + var * unbias * MOM
    return sr.bf16r(f), mean, invstd, rm, rv


def bn_bwd_f32(dy, x, pos, gamma, mean, invstd):
    d = (0, 2, 3)
    dyf, xf = dy.float(), x.float()
    if pos is not None:
        dyf = dyf * pos
    M = xf.numel() // xf.shape[1]
    xhat = (xf - c_(mean)) * c_(invstd)
    dbeta = dyf.sum(d)
    dgamma = (dyf * xhat).sum(d)
    k1 = gamma * invstd
    dx = c_(k1) * dyf - c_(k1 * dbeta / M) - c_(k1 * dgamma / M) * xhat
    return sr.bf16r(dx), dgamma, dbeta


def last_row_unwritten(t):
    t = t.clone()
    t[-1, :, -1, -1] = 0
    return t


def octet_zeroed(t, n=1, c8=1, h=2, w=3):
    t = t.clone()
    t[n, 8 * c8:8 * c8 + 8, h, w] = 0
    return t


def passes(out, ref, rel, abs_i):
    return sr.check_close(out, ref, rel, abs_i, "t")[0]


# ---------------------------------------------------------------- comparator
def test_comparator_reports_count_and_worst_index():
    ref = torch.ones(2, 3, dtype=torch.float64)
    out = ref.clone()
    out[1, 2] += 1.0
    out[0, 1] += 0.5
    ok, worst, msg = sr.check_close(out, ref, 0.25, 0.0, "demo")
    assert not ok and worst == pytest.approx(4.0)
    assert "2 of 6" in msg and "(1, 2)" in msg
    # per element, not max-over-max: one small element off by its own size
    ref = torch.tensor([1000.0, 1e-3], dtype=torch.float64)
    assert not passes(torch.tensor([1000.0, 0.0]), ref, REL_BF16, 0.0)
    assert not passes(torch.tensor([1000.0, float("nan")]), ref, 1.0, 1.0)
    assert passes(ref.float(), ref, REL_BF16, 0.0)
    with pytest.raises(AssertionError, match="1 of 2 elements differ"):
        sr.assert_equal(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 3.0]), "eq")


def test_mask_pack_layout():
    g = torch.Generator().manual_seed(0)
    pos = torch.rand(SHAPE, generator=g) > 0.5
    m = sr.pack_mask(pos)
    N, C, H, W = SHAPE
    assert m.shape == (N * H * W, C // 8) and m.dtype == torch.uint8
    # row m = (n, h, w); bit j of byte c8 is channel 8*c8 + j
    n, h, w, c = 2, 3, 4, 13
    row = (n * H + h) * W + w
    assert bool(m[row, c // 8] >> (c % 8) & 1) == bool(pos[n, c, h, w])
    assert torch.equal(sr.unpack_mask(m, SHAPE), pos)


# ---------------------------------------------------------------- BN forward
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("offset", [True, False])
def test_bn_fwd_reference_separates(relu, with_res, offset):
    x = sr.bn_input(SHAPE, offset=offset, seed=1)
    gamma, beta, rm0, rv0 = params(SHAPE[1], 2)
    res = sr.rand_bf16(SHAPE, 3, scale=2.0) if with_res else None
    ref = sr.bn_fwd_ref(x, gamma, beta, EPS, relu, res, rm0, rv0, MOM)
    y, mean, invstd, rm, rv = bn_fwd_f32(x, gamma, beta, relu, res, rm0, rv0)
    if offset:
        assert float((ref["mean"] ** 2 / ref["var"]).max()) > 60
    assert passes(y, ref["y"], REL_BF16, ref["y_abs"])
    assert passes(mean, ref["mean"], 0, ref["mean_abs"])
    assert passes(invstd, ref["invstd"], 0, ref["invstd_abs"])
    assert passes(rm, ref["running_mean"], 0, ref["running_mean_abs"])
    assert passes(rv, ref["running_var"], 0, ref["running_var_abs"])
    # mutations
    assert not passes(last_row_unwritten(y), ref["y"], REL_BF16, ref["y_abs"])
    if not relu:  # with ReLU a zero octet can be the right answer
        assert not passes(octet_zeroed(y), ref["y"], REL_BF16, ref["y_abs"])
    rv_biased = bn_fwd_f32(x, gamma, beta, relu, res, rm0, rv0, unbiased=False)[4]
    assert not passes(rv_biased, ref["running_var"], 0, ref["running_var_abs"])
    # two bf16 ulps off in one element are caught (one ulp is the bound at
    # the top of a binade)
    y1 = y.clone()
    i = torch.unravel_index(torch.argmax(y.float().abs()), y.shape)
    y1.view(torch.int16)[i] += 2
    assert not passes(y1, ref["y"], REL_BF16, ref["y_abs"])


def test_bn_fwd_single_row():
    """M = 1: var = 0, invstd = rsqrt(eps), y = beta (+ res)."""
    shape = (1, 64, 1, 1)
    x = sr.bn_input(shape, seed=4)
    gamma, beta, rm0, rv0 = params(64, 5)
    ref = sr.bn_fwd_ref(x, gamma, beta, EPS, False, None, rm0, rv0, MOM)
    assert float(ref["var"].abs().max()) == 0.0
    assert torch.allclose(ref["invstd"], torch.full_like(ref["invstd"], EPS ** -0.5))
    assert torch.allclose(ref["y"].reshape(-1), beta.double(), atol=1e-12)
    assert torch.equal(ref["running_var"], rv0.double() * (1 - MOM))


# ---------------------------------------------------------------- BN backward
@pytest.mark.parametrize("relu", [True, False])
def test_bn_bwd_reference_separates(relu):
    x = sr.bn_input(SHAPE, seed=6)
    gamma, beta, rm0, rv0 = params(SHAPE[1], 7)
    y, mean, invstd, _, _ = bn_fwd_f32(x, gamma, beta, relu, None, rm0, rv0)
    dy = sr.rand_bf16(SHAPE, 8, shift=0.25)
    pos = (y > 0) if relu else None
    ref = sr.bn_bwd_ref(dy, x, pos, gamma, mean, invstd)
    dx, dgamma, dbeta = bn_bwd_f32(dy, x, pos, gamma, mean, invstd)
    assert passes(dx, ref["dx"], REL_BF16, ref["dx_abs"])
    assert passes(dgamma, ref["dgamma"], 0, ref["dgamma_abs"])
    assert passes(dbeta, ref["dbeta"], 0, ref["dbeta_abs"])
    assert not passes(last_row_unwritten(dx), ref["dx"], REL_BF16, ref["dx_abs"])
    assert not passes(octet_zeroed(dx), ref["dx"], REL_BF16, ref["dx_abs"])
    # a dropped last row in the statistics
    dyz = last_row_unwritten(dy)
    _, dg2, db2 = bn_bwd_f32(dyz, x, pos, gamma, mean, invstd)
    assert not passes(dg2, ref["dgamma"], 0, ref["dgamma_abs"])
    assert not passes(db2, ref["dbeta"], 0, ref["dbeta_abs"])
    if relu:
        # second-to-last row gated by the last row's mask byte
        mask = sr.pack_mask(pos)
        assert not torch.equal(mask[-2], mask[-1])
        wrong = mask.clone()
        wrong[-2] = mask[-1]
        dxm, _, _ = bn_bwd_f32(dy, x, sr.unpack_mask(wrong, SHAPE), gamma,
                               mean, invstd)
        assert not passes(dxm, ref["dx"], REL_BF16, ref["dx_abs"])


# ---------------------------------------------------------------- add + mask
def test_add_mask_reference_separates():
    dy = sr.rand_bf16(SHAPE, 9)
    dx0 = sr.rand_bf16(SHAPE, 10)
    g = torch.Generator().manual_seed(11)
    N, C, H, W = SHAPE
    mask = torch.randint(0, 256, (N * H * W, C // 8), generator=g, dtype=torch.uint8)

    def cand(m):
        gate = sr.unpack_mask(m, SHAPE)
        return sr.bf16r(dy.float() * gate + dx0.float())

    ref = cand(mask)
    sr.assert_equal(cand(mask), ref, "add_mask")
    for bad in (last_row_unwritten(ref), octet_zeroed(ref)):
        with pytest.raises(AssertionError):
            sr.assert_equal(bad, ref, "add_mask")
    assert not torch.equal(mask[-2], mask[-1])
    wrong = mask.clone()
    wrong[-2] = mask[-1]
    with pytest.raises(AssertionError):
        sr.assert_equal(cand(wrong), ref, "add_mask")


# ---------------------------------------------------------------- max-pool
POOLS = [(3, 2, 1), (3, 1, 1), (2, 2, 0)]


@pytest.mark.parametrize("K,stride,pad", POOLS)
def test_pool_pattern_is_tie_free(K, stride, pad):
    """At the largest H, W the GPU tests use; n and c only shift the pattern,
    so a few of each are as good as all of them."""
    for d in [(dr, ds) for dr in range(-2, 3) for ds in range(-2, 3)]:
        assert d == (0, 0) or (97 * d[0] + 41 * d[1]) % 251 != 0
    for shift in (-125, -251):
        x = sr.pool_pattern((2, 8, 259, 261), shift=shift)
        assert torch.equal(x.float().to(torch.bfloat16), x)  # exact in bf16
        assert int(x.float().abs().max()) <= 251
        assert sr.pool_tied_windows(x, K, stride, pad) == 0
    assert float(sr.pool_pattern((2, 8, 9, 9), shift=-251).float().max()) < 0


@pytest.mark.parametrize("K,stride,pad", POOLS)
def test_pool_bwd_reference_separates(K, stride, pad):
    shape = (2, 16, 15, 17)
    x = sr.pool_pattern(shape)
    HO = (shape[2] + 2 * pad - K) // stride + 1
    WO = (shape[3] + 2 * pad - K) // stride + 1
    dy = sr.rand_bf16((2, 16, HO, WO), 12)
    y, idx, dx, dx_abs = sr.pool_ref(x, dy, K, stride, pad)
    # every window position is some window's argmax
    assert sorted(idx.unique().tolist()) == list(range(K * K))
    yf = F.max_pool2d(x.float().contiguous(), K, stride, pad)
    assert torch.equal(y.float(), yf)
    cand = sr.bf16r(sr.pool_scatter(dy, idx, shape, K, stride, pad).float())
    assert passes(cand, dx, REL_BF16, dx_abs)
    if float(dx[-1, :, -1, -1].abs().max()) > 0:  # else zero is the answer
        assert not passes(last_row_unwritten(cand), dx, REL_BF16, dx_abs)
    assert not passes(octet_zeroed(cand, h=1, w=1), dx, REL_BF16, dx_abs) or \
        float(dx[1, 8:16, 1, 1].abs().max()) == 0
    shifted = sr.bf16r(sr.pool_scatter(dy, idx + 1, shape, K, stride, pad).float())
    assert not passes(shifted, dx, REL_BF16, dx_abs)


def test_pool_all_negative_pads_as_minus_infinity():
    x = sr.pool_pattern((2, 16, 15, 17), shift=-251)
    y, idx, _, _ = sr.pool_ref(x, None, 3, 2, 1)
    assert float(y.float().max()) < 0  # a zero pad would win every border


# ---------------------------------------------------------------- the rest
def test_xent_reference_extremes():
    g = torch.Generator().manual_seed(13)
    for base in (90.0, -90.0, 0.0):
        logits = sr.bf16r(base + 4 * (torch.rand(5, 1000, generator=g) * 2 - 1))
        tgt = torch.randint(0, 1000, (5,), generator=g)
        loss, loss_abs, probs, probs_abs = sr.xent_ref(logits, tgt)
        lf = F.cross_entropy(logits.float(), tgt)
        assert passes(lf, loss, 0, loss_abs)
        assert passes(F.softmax(logits.float(), 1), probs, 0, probs_abs)
        # no max-subtraction: overflow (or underflow to 0/0) must fail; at
        # logits in [-4, 4] it passes, which is why those cases exist
        e = logits.float().exp()
        assert passes(e / e.sum(1, keepdim=True), probs, 0, probs_abs) == (base == 0)
    one = torch.zeros(3, 1, dtype=torch.bfloat16)
    loss, _, probs, _ = sr.xent_ref(one, torch.zeros(3, dtype=torch.long))
    assert float(loss) == 0 and torch.equal(probs, torch.ones_like(probs))
    d, _ = sr.xent_bwd_ref(probs, torch.zeros(3, dtype=torch.long), 0.37)
    assert float(d.abs().max()) == 0


@pytest.mark.parametrize("nesterov", [False, True])
def test_sgd_reference_matches_fp32(nesterov):
    from mpi_operator_amd.ops import reference as ref
    g = torch.Generator().manual_seed(14)
    p = torch.randn(8193, generator=g)
    gr = sr.bf16r(torch.randn(8193, generator=g))
    m = torch.randn(8193, generator=g).abs()
    out = torch.empty(8193, dtype=torch.bfloat16)
    p_ref, p_abs, m_ref, m_abs = sr.sgd_ref(p, gr, m, 0.1, 0.9, 0.01, nesterov)
    p2, m2 = p.clone(), m.clone()
    ref.sgd_momentum_step([p2], [gr], [m2], [out], 0.1, 0.9, 0.01, nesterov)
    assert passes(p2, p_ref, sr.REL_F32, p_abs)
    assert passes(m2, m_ref, sr.REL_F32, m_abs)
    assert passes(out, p_ref, REL_BF16, p_abs)
    # the other nesterov setting, and a missing weight decay, are caught
    p3, m3 = p.clone(), m.clone()
    ref.sgd_momentum_step([p3], [gr], [m3], [out], 0.1, 0.9, 0.01, not nesterov)
    assert not passes(p3, p_ref, sr.REL_F32, p_abs)
    p4, m4 = p.clone(), m.clone()
    ref.sgd_momentum_step([p4], [gr], [m4], [out], 0.1, 0.9, 0.0, nesterov)
    assert not passes(m4, m_ref, sr.REL_F32, m_abs)
