"""The memory-bound NHWC kernels (BatchNorm, add/ReLU joins, pooling, softmax
cross-entropy, SGD) against fp64 references, at the shapes where their loops
repeat: capped grids that wrap, the second row/octet chain present for some
lanes only, idle row lanes (C8 no power of two), odd row counts, and inputs
whose mean dwarfs their variance.

Every comparison is per element, |out - ref| <= rel*|ref| + abs_i, with the
bounds of stream_refs.py (derived from the number formats, not measured), or
torch.equal where the result is a sum of two bf16 values, a max, a copy or a
select. tests/test_stream_refs_cpu.py shows that these bounds pass a correct
fp32 implementation and fail a dropped row, a zeroed octet, a wrong mask byte.

Worst observed |out - ref| / bound over all cases of this file on an MI355X
(1.0 = at the bound), first run, bounds as derived:

  output                  rel     abs_i                        worst ratio
  bn.mean                 0       2^-18 mean|x|                0.028
  bn.invstd               0       invstd 2^-18 (1+mean^2/var)  0.035
  bn.running_mean         0       2^-18 of its summands        0.044
  bn.running_var          0       2^-18 of its summands        0.032
  bn.y                    2^-8    2^-16 (|x sc|+|sh|+|res|)    0.992
  bn.eval_y               2^-8    2^-16 (|x sc|+|sh|)          0.992
  bn.dbeta                0       2^-18 sum|dy m|              0.021
  bn.dgamma               0       2^-18 sum|dy m xhat|         0.022
  bn.dx                   2^-8    2^-16 (|k1 dy|+|k2|+|k3 xh|) 0.992
  gap_fwd                 2^-8    2^-16 mean|x|                0.973
  gap_bwd                 2^-8    2^-16 |dy|/HW                0.915
  maxpool.dx              2^-8    2^-16 sum|dy| of the pixel   0.992
  xent.loss               0       2^-18 mean(|lse|+|max|+|xt|) 0.040
  xent.probs              0       2^-18 p                      0.153
  xent.dlogits            2^-8    2^-16 (p + onehot) scale     0.992
  sgd.momentum            2^-22   2^-22 sum|terms|             0.224
  sgd.master              2^-22   2^-22 sum|terms|             0.319
  sgd.out                 2^-8    2^-22 sum|terms|             0.995

The bf16 outputs sit at 0.99: half a bf16 ulp is 2^-8 of a value at the bottom
of its binade, and among millions of elements one is always there. The fp32
statistics use 2-5% of their bound (the chains are shorter than the ~600
adds the derivation allows for, and their errors do not all align). The
bit-exact kernels (add_bf16, add_relu_fwd/bwd/bwd_add/bwd_add_mask, maxpool
y and idx, the BN ReLU mask) are compared with torch.equal and have no row.
"""
import functools

import pytest
import torch

import stream_refs as sr
from stream_refs import REL_BF16, REL_F32, STAT

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.3
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def ext():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def empty_u8():
    return torch.empty(0, dtype=torch.uint8)


# ================================================================= BatchNorm
# (N, C, H, W)                      M        what it reaches
BN_FULL = [
    (3, 64, 211, 209),    # 132297: C8=8, 32 rows/block; partials grid capped at
                          # 512 (five pair-trips); apply grid capped at 2048,
                          # second-row chain taken, second trip for 1225 rows
    (1, 192, 223, 185),   # 41255: C8=24, 10 rows/block, 16 idle threads; apply
                          # stride 20480 rows, second trip for the tail
    (1, 2048, 63, 67),    # 4221: C8=256, 1 row/block; both caps hit, second
                          # row present for some blocks only
]
BN_LIGHT = [
    (5, 8, 461, 457),     # 1053385: C8=1, 256 rows/block; apply stride 524288
    (1, 24, 9, 7),        # 63: C8=3, 85 rows/block, one idle thread, one block
    (1, 64, 1, 1),        # 1: unbias guard, var = 0, invstd = rsqrt(eps)
]


@functools.lru_cache(maxsize=None)
def bn_inputs(shape, offset=True):
    """Inputs of one shape, made once and never modified."""
    C = shape[1]
    x = sr.bn_input(shape, offset=offset, seed=20, device=DEV)
    g = torch.Generator().manual_seed(21)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    rm0 = torch.randn(C, generator=g).to(DEV)
    rv0 = (torch.rand(C, generator=g) + 0.5).to(DEV)
    res = sr.rand_bf16(shape, 22, scale=2.0, device=DEV)
    dy = sr.rand_bf16(shape, 23, shift=0.25, device=DEV)
    return x, gamma, beta, rm0, rv0, res, dy


def run_bn_fwd(shape, relu, with_res, offset=True):
    x, gamma, beta, rm0, rv0, res, _ = bn_inputs(shape, offset)
    rm, rv = rm0.clone(), rv0.clone()
    y, mean, invstd, mask = ext().bn_fwd_train(
        x, gamma, beta, EPS, relu, rm, rv, MOM,
        res if with_res else torch.empty(0))
    return y, mean, invstd, mask, rm, rv


def check_bn_fwd(shape, relu, with_res, offset=True):
    x, gamma, beta, rm0, rv0, res, _ = bn_inputs(shape, offset)
    y, mean, invstd, mask, rm, rv = run_bn_fwd(shape, relu, with_res, offset)
    ref = sr.bn_fwd_ref(x, gamma, beta, EPS, relu, res if with_res else None,
                        rm0, rv0, MOM)
    N, C, H, W = shape
    M = N * H * W
    if offset and M > 1:
        assert float((ref["mean"] ** 2 / ref["var"]).max()) > 60
    sr.assert_close(mean, ref["mean"], 0, ref["mean_abs"], "bn.mean")
    if M > 1:
        sr.assert_close(invstd, ref["invstd"], 0, ref["invstd_abs"], "bn.invstd")
    else:  # both moments of one bf16 value are exact in fp32: var is 0
        assert float(ref["var"].abs().max()) == 0
        sr.assert_close(invstd, torch.full_like(ref["invstd"], EPS ** -0.5),
                        STAT, 0, "bn.invstd")
    sr.assert_close(rm, ref["running_mean"], 0, ref["running_mean_abs"],
                    "bn.running_mean")
    sr.assert_close(rv, ref["running_var"], 0, ref["running_var_abs"],
                    "bn.running_var")
    sr.assert_close(y, ref["y"], REL_BF16, ref["y_abs"], "bn.y")
    if relu:
        assert mask.shape == (M, C // 8) and mask.dtype == torch.uint8
        sr.assert_equal(mask, sr.pack_mask(y > 0), "bn.mask")
        assert float(y.float().min()) >= 0
    else:
        assert mask.numel() == 0


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape", BN_FULL, ids=str)
def test_bn_fwd_train(shape, relu, with_res):
    check_bn_fwd(shape, relu, with_res)


@pytest.mark.parametrize("shape", BN_LIGHT, ids=str)
def test_bn_fwd_train_edge_shapes(shape):
    check_bn_fwd(shape, True, True)


def test_bn_fwd_train_zero_mean():
    check_bn_fwd(BN_FULL[0], True, False, offset=False)


def check_bn_bwd(shape, mode, offset=True):
    """mode: 'mask' (the forward's bitmask), 'y' (empty mask: y > 0 re-read)
    or 'norelu'."""
    x, gamma, beta, _, _, _, dy = bn_inputs(shape, offset)
    relu = mode != "norelu"
    y, mean, invstd, mask, _, _ = run_bn_fwd(shape, relu, False, offset)
    dx, dgamma, dbeta = ext().bn_bwd(dy, x, y, gamma, mean, invstd, relu,
                                     mask if mode == "mask" else empty_u8())
    ref = sr.bn_bwd_ref(dy, x, (y > 0) if relu else None, gamma, mean, invstd)
    sr.assert_close(dbeta, ref["dbeta"], 0, ref["dbeta_abs"], "bn.dbeta")
    sr.assert_close(dgamma, ref["dgamma"], 0, ref["dgamma_abs"], "bn.dgamma")
    sr.assert_close(dx, ref["dx"], REL_BF16, ref["dx_abs"], "bn.dx")


@pytest.mark.parametrize("mode", ["mask", "y", "norelu"])
@pytest.mark.parametrize("shape", BN_FULL, ids=str)
def test_bn_bwd(shape, mode):
    check_bn_bwd(shape, mode)


@pytest.mark.parametrize("shape", BN_LIGHT, ids=str)
def test_bn_bwd_edge_shapes(shape):
    check_bn_bwd(shape, "mask")


def test_bn_bwd_zero_mean():
    check_bn_bwd(BN_FULL[0], "mask", offset=False)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape", [BN_FULL[0], BN_FULL[1], BN_LIGHT[1]], ids=str)
def test_bn_fwd_eval(shape, relu):
    from mpi_operator_amd.ops import functional as Fx
    x, gamma, beta, rm0, rv0, _, _ = bn_inputs(shape)
    rm = rm0 * 8  # running mean of the size of the data's own
    y = Fx.bn_relu_eval(x, gamma, beta, rm, rv0, EPS, relu)
    ref, y_abs = sr.bn_eval_ref(x, gamma, beta, rm, rv0, EPS, relu)
    sr.assert_close(y, ref, REL_BF16, y_abs, "bn.eval_y")


# ================================================================= elementwise
# the grid is capped at 2048 x 256 = 524288 octets
EW_SHAPES = [
    (5, 64, 165, 160),    # n8 = 1056000 > 2 x 524288: second trip, and
                          # add_bf16's i2 valid for some lanes only
    (3, 64, 149, 147),    # n8 = 525672: i2 taken for 1384 octets only
]


@functools.lru_cache(maxsize=None)
def ew_inputs(shape):
    N, C, H, W = shape
    a = sr.rand_bf16(shape, 30, device=DEV)
    b = sr.rand_bf16(shape, 31, device=DEV)
    dy = sr.rand_bf16(shape, 32, device=DEV)
    dx0 = sr.rand_bf16(shape, 33, device=DEV)
    y = torch.relu(a.float() + b.float()).to(torch.bfloat16)  # ~half exactly 0
    g = torch.Generator().manual_seed(34)
    mask = torch.randint(0, 256, (N * H * W, C // 8), generator=g,
                         dtype=torch.uint8).to(DEV)
    return a, b, dy, dx0, y, mask


@pytest.mark.parametrize("shape", EW_SHAPES, ids=str)
def test_add_kernels_bit_exact(shape):
    a, b, dy, dx0, y, mask = ew_inputs(shape)
    zero_frac = float((y == 0).float().mean())
    assert 0.4 < zero_frac < 0.6, zero_frac
    e = ext()
    bf = torch.bfloat16
    sr.assert_equal(e.add_bf16(a, b), (a.float() + b.float()).to(bf), "add_bf16")
    sr.assert_equal(e.add_relu_fwd(a, b), y, "add_relu_fwd")
    zero = torch.zeros_like(dy)
    sr.assert_equal(e.add_relu_bwd(dy, y), torch.where(y > 0, dy, zero),
                    "add_relu_bwd")
    fz = torch.zeros_like(dy, dtype=torch.float32)
    sr.assert_equal(e.add_relu_bwd_add(dy, y, dx0),
                    (torch.where(y > 0, dy.float(), fz) + dx0.float()).to(bf),
                    "add_relu_bwd_add")
    gate = sr.unpack_mask(mask, shape)
    sr.assert_equal(e.add_relu_bwd_add_mask(dy, mask, dx0),
                    (torch.where(gate, dy.float(), fz) + dx0.float()).to(bf),
                    "add_relu_bwd_add_mask")


@pytest.mark.parametrize("shape", [
    (2049, 2048, 1, 1),   # 524544 tasks: second trip
    (3, 24, 5, 7),        # C8 = 3, odd HW
    (4, 2048, 7, 7),      # the ResNet head
], ids=str)
def test_gap_fwd(shape):
    x = sr.rand_bf16(shape, 35, scale=2.0, shift=0.5, device=DEV)
    y = ext().gap_fwd(x)
    xd = x.double()
    sr.assert_close(y, xd.mean((2, 3)), REL_BF16,
                    sr.ABS_TERM * xd.abs().mean((2, 3)), "gap_fwd")


def test_gap_bwd():
    N, C, H, W = 48, 2048, 7, 7  # 602112 tasks: second trip
    dy = sr.rand_bf16((N, C), 36, device=DEV)
    dx = ext().gap_bwd(dy, H, W)
    assert dx.shape == (N, C, H, W)
    assert dx.is_contiguous(memory_format=torch.channels_last)
    ref = (dy.double() / (H * W))[:, :, None, None].expand(N, C, H, W)
    sr.assert_close(dx, ref, REL_BF16, sr.ABS_TERM * ref.abs(), "gap_bwd")


# ================================================================= max-pool
@pytest.mark.parametrize("shape,K,stride,pad,shift", [
    ((2, 16, 15, 17), 3, 2, 1, -125),
    ((2, 16, 15, 17), 3, 1, 1, -125),   # overlapping windows: several
                                        # windows scatter into one pixel
    ((2, 16, 15, 17), 2, 2, 0, -125),
    ((4, 64, 259, 261), 3, 2, 1, -125),  # 544960 fwd tasks, 2.16M bwd tasks:
                                         # both loops wrap
    ((2, 24, 15, 17), 3, 2, 1, -125),   # C8 = 3
    ((2, 16, 15, 17), 3, 2, 1, -251),   # all negative: padding is -inf, not 0
], ids=str)
def test_maxpool(shape, K, stride, pad, shift):
    x = sr.pool_pattern(shape, shift=shift, device=DEV)
    N, C, H, W = shape
    HO = (H + 2 * pad - K) // stride + 1
    WO = (W + 2 * pad - K) // stride + 1
    dy = sr.rand_bf16((N, C, HO, WO), 40, device=DEV)
    y_ref, idx_ref, dx_ref, dx_abs = sr.pool_ref(x, dy, K, stride, pad)
    y, idx = ext().maxpool_fwd(x, K, stride, pad)
    sr.assert_equal(y, y_ref, "maxpool.y")
    if shift == -251:
        assert float(y.float().max()) < 0
    sr.assert_equal(idx, idx_ref, "maxpool.idx")
    dx = ext().maxpool_bwd(dy, idx, H, W, K, stride, pad)
    sr.assert_close(dx, dx_ref, REL_BF16, dx_abs, "maxpool.dx")


# ================================================================= softmax-xent
@pytest.mark.parametrize("B,V,base", [
    (525, 1000, 0.0),     # 525000 backward tasks: the grid-stride loop wraps
    (64, 257, 0.0),       # one past a block width
    (64, 1000, 90.0),     # without the max-subtraction exp overflows ...
    (64, 1000, -90.0),    # ... or every term underflows
])
def test_softmax_xent(B, V, base):
    g = torch.Generator().manual_seed(41)
    logits = sr.bf16r(base + 4 * (torch.rand(B, V, generator=g) * 2 - 1)).to(DEV)
    tgt = torch.randint(0, V, (B,), generator=g).to(DEV)
    tgt[0], tgt[1] = 0, V - 1
    loss, probs = ext().softmax_xent_fwd(logits, tgt)
    loss_ref, loss_abs, probs_ref, probs_abs = sr.xent_ref(logits, tgt)
    sr.assert_close(loss, loss_ref, 0, loss_abs, "xent.loss")
    sr.assert_close(probs, probs_ref, 0, probs_abs, "xent.probs")
    dloss = torch.full((1,), 0.37, device=DEV)
    d = ext().softmax_xent_bwd(probs, tgt, dloss)
    d_ref, d_abs = sr.xent_bwd_ref(probs, tgt, float(dloss))
    sr.assert_close(d, d_ref, REL_BF16, d_abs, "xent.dlogits")


def test_softmax_xent_single_class():
    logits = sr.rand_bf16((8, 1), 42, scale=4.0, device=DEV)
    tgt = torch.zeros(8, dtype=torch.long, device=DEV)
    loss, probs = ext().softmax_xent_fwd(logits, tgt)
    assert float(loss) == 0.0
    assert torch.equal(probs, torch.ones_like(probs))
    d = ext().softmax_xent_bwd(probs, tgt, torch.full((1,), 0.37, device=DEV))
    assert float(d.float().abs().max()) == 0.0


# ================================================================= SGD
def run_sgd(sizes, grad_dtype, nesterov, fp32_params=()):
    """One fused call over tensors of `sizes`; those at the indices in
    fp32_params have no bf16 working copy. Checked against the fp64 algebra."""
    from mpi_operator_amd.ops import functional as Fx
    lr, mu, wd = 0.1, 0.9, 0.01
    g = torch.Generator().manual_seed(43)
    p0 = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    gr = [torch.randn(n, generator=g).to(grad_dtype).to(DEV) for n in sizes]
    m0 = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    outs = [None if i in fp32_params else
            torch.full((n,), float("nan"), dtype=torch.bfloat16, device=DEV)
            for i, n in enumerate(sizes)]
    p, m = [t.clone() for t in p0], [t.clone() for t in m0]
    Fx.sgd_momentum_step(p, gr, m, outs, lr, mu, wd, nesterov)
    for i, n in enumerate(sizes):
        p_ref, p_abs, m_ref, m_abs = sr.sgd_ref(p0[i], gr[i], m0[i], lr, mu,
                                                wd, nesterov)
        tag = f"[{i}:{n}]"
        sr.assert_close(m[i], m_ref, REL_F32, m_abs, "sgd.momentum" + tag)
        sr.assert_close(p[i], p_ref, REL_F32, p_abs, "sgd.master" + tag)
        if outs[i] is not None:
            sr.assert_close(outs[i], p_ref, REL_BF16, p_abs, "sgd.out" + tag)


SGD_SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 100, 127, 128, 129,
             255, 256, 257, 500, 511, 512, 513, 1000, 1023, 1024, 1025, 2047,
             2048, 2049, 2055, 3000, 4095, 4096, 4097, 5000, 6001, 7000, 8191,
             8192,  # index 39: the last tensor of the first 40-tensor launch
             8193,  # index 40: the first of the second; a one-element tail block
             8200, 9000, 12, 24, 16385, 3]


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_sgd_many_tensors_bf16_grads(nesterov):
    assert len(SGD_SIZES) >= 45 and SGD_SIZES[39] == 8192 and SGD_SIZES[40] == 8193
    run_sgd(SGD_SIZES, torch.bfloat16, nesterov, fp32_params=(3, 20, 40))


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_sgd_fp32_grads_interior_blocks(nesterov):
    # two interior blocks (base + 8192 <= numel) and a 13-element tail
    run_sgd([8192 * 2 + 13, 8192, 5], torch.float32, nesterov, fp32_params=(1,))


# ================================================================= validation
def _bn_args(C=16, shape=None):
    shape = shape or (2, C, 3, 5)
    x = sr.rand_bf16(shape, 50, device=DEV)
    v = lambda: torch.ones(shape[1], device=DEV)  # noqa: E731
    return x, v


def _bad_calls():
    """(id, callable) pairs; every callable must raise on the host, before
    any launch. C = 12 is no multiple of 8: (2,12,3,5) has 360 = 8 x 45
    elements, so the channel check decides; (1,12,3,3) has 108."""
    e = ext()
    x16, v16 = _bn_args(16)
    x12, v12 = _bn_args(12)
    other = sr.rand_bf16((2, 16, 5, 3), 51, device=DEV)   # same numel, other shape
    small = sr.rand_bf16((1, 16, 3, 5), 52, device=DEV)
    odd = sr.rand_bf16((1, 12, 3, 3), 53, device=DEV)     # numel % 8 == 4
    f32 = x16.float()
    M16 = 2 * 3 * 5
    mask16 = torch.zeros(M16, 2, dtype=torch.uint8, device=DEV)
    mask_short = mask16[:-1].contiguous()
    slab16 = torch.zeros(1, 2, 16, device=DEV)
    slab12 = torch.zeros(1, 2, 12, device=DEV)
    eu8 = empty_u8()
    nothing = torch.empty(0)
    idx16 = torch.zeros(2, 2, 3, 16, dtype=torch.uint8, device=DEV)
    idx12 = torch.zeros(2, 2, 3, 12, dtype=torch.uint8, device=DEV)
    dyp16 = sr.rand_bf16((2, 16, 2, 3), 54, device=DEV)   # pooled 3x5 (3,2,1)
    dyp12 = sr.rand_bf16((2, 12, 2, 3), 55, device=DEV)
    g16 = sr.rand_bf16((4, 16), 56, device=DEV)
    g12 = sr.rand_bf16((4, 12), 57, device=DEV)
    return [
        ("maxpool_fwd-C12", lambda: e.maxpool_fwd(x12, 3, 2, 1)),
        ("maxpool_bwd-C12", lambda: e.maxpool_bwd(dyp12, idx12, 3, 5, 3, 2, 1)),
        ("maxpool_bwd-idx", lambda: e.maxpool_bwd(dyp16, idx16[:1].contiguous(),
                                                  3, 5, 3, 2, 1)),
        ("maxpool_bwd-hw", lambda: e.maxpool_bwd(dyp16, idx16, 9, 9, 3, 2, 1)),
        ("gap_fwd-C12", lambda: e.gap_fwd(x12)),
        ("gap_bwd-C12", lambda: e.gap_bwd(g12, 3, 5)),
        ("add_relu_fwd-numel", lambda: e.add_relu_fwd(odd, odd)),
        ("add_relu_fwd-b-shape", lambda: e.add_relu_fwd(x16, other)),
        ("add_relu_fwd-b-small", lambda: e.add_relu_fwd(x16, small)),
        ("add_relu_fwd-b-dtype", lambda: e.add_relu_fwd(x16, f32)),
        ("add_relu_bwd-numel", lambda: e.add_relu_bwd(odd, odd)),
        ("add_relu_bwd-y-shape", lambda: e.add_relu_bwd(x16, small)),
        ("add_relu_bwd-y-dtype", lambda: e.add_relu_bwd(x16, f32)),
        ("add_relu_bwd_add-numel", lambda: e.add_relu_bwd_add(odd, odd, odd)),
        ("add_relu_bwd_add-y-shape", lambda: e.add_relu_bwd_add(x16, other, x16)),
        ("add_relu_bwd_add-dx0-shape", lambda: e.add_relu_bwd_add(x16, x16, small)),
        ("add_relu_bwd_add-dx0-dtype", lambda: e.add_relu_bwd_add(x16, x16, f32)),
        ("add_relu_bwd_add_mask-mask", lambda: e.add_relu_bwd_add_mask(
            x16, mask_short, x16)),
        ("add_relu_bwd_add_mask-dx0", lambda: e.add_relu_bwd_add_mask(
            x16, mask16, small)),
        ("add_bf16-shape", lambda: e.add_bf16(x16, small)),
        ("bn_fwd_train-C12", lambda: e.bn_fwd_train(
            x12, v12(), v12(), EPS, True, v12(), v12(), MOM, nothing)),
        ("bn_fwd_train-res", lambda: e.bn_fwd_train(
            x16, v16(), v16(), EPS, True, v16(), v16(), MOM, small)),
        ("bn_fwd_train-gamma", lambda: e.bn_fwd_train(
            x16, v12(), v16(), EPS, True, v16(), v16(), MOM, nothing)),
        ("bn_fwd_train-running", lambda: e.bn_fwd_train(
            x16, v16(), v16(), EPS, True, v12(), v12(), MOM, nothing)),
        ("bn_fwd_eval-C12", lambda: e.bn_fwd_eval(x12, v12(), v12(), True)),
        ("bn_fwd_eval-scale", lambda: e.bn_fwd_eval(x16, v12(), v16(), True)),
        ("bn_bwd-C12", lambda: e.bn_bwd(
            x12, x12, x12, v12(), v12(), v12(), True, eu8)),
        ("bn_bwd-dy", lambda: e.bn_bwd(
            small, x16, x16, v16(), v16(), v16(), True, eu8)),
        ("bn_bwd-y", lambda: e.bn_bwd(
            x16, x16, small, v16(), v16(), v16(), True, eu8)),
        ("bn_bwd-mask", lambda: e.bn_bwd(
            x16, x16, x16, v16(), v16(), v16(), True, mask_short)),
        ("bn_bwd-mean", lambda: e.bn_bwd(
            x16, x16, x16, v16(), v12(), v16(), True, mask16)),
        ("bn_bwd_pre-C12", lambda: e.bn_bwd_pre(
            x12, slab12, x12, x12, v12(), v12(), v12(), True, eu8)),
        ("bn_bwd_pre-dy", lambda: e.bn_bwd_pre(
            small, slab16, x16, x16, v16(), v16(), v16(), True, eu8)),
        ("bn_bwd_pre-mask", lambda: e.bn_bwd_pre(
            x16, slab16, x16, x16, v16(), v16(), v16(), True, mask_short)),
        ("bn_bwd_pre-slab", lambda: e.bn_bwd_pre(
            x16, slab12, x16, x16, v16(), v16(), v16(), True, mask16)),
    ]


def test_bindings_reject_bad_arguments():
    accepted = []
    for name, call in _bad_calls():
        try:
            call()
        except RuntimeError:
            continue
        accepted.append(name)
    assert not accepted, f"accepted without an error: {accepted}"
