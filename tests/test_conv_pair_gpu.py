"""The paired conv backward (conv2d_dgrad_wgrad, conv2d_dgrad_bn_wgrad): a
stride-1 conv's dgrad and wgrad GEMMs launched as one grid must return, bit
for bit, what conv2d_dgrad / conv2d_dgrad_bn and conv2d_wgrad return on the
same inputs: every workgroup of the pair runs the tile, split and K range it
runs in the separate launch. So every comparison here is torch.equal, under
each workgroup order, each epilogue (set_epilogue_vec) and with the pair
switched off (set_pair_bwd(False): the bindings then issue the two launches).

Shapes are the smallest that reach each path of the pair launcher:
  1x1  N=2 9x9 72->136     M=162 ragged against the 128-row tile, neither
                           channel count a multiple of 128, dgrad unsplit
  1x1  N=1 8x8 128->128    one tile per problem, one k-tile for the dgrad
  1x1  N=1 64x64 64->1024  conv_splits 2 and conv_wgrad_splits 8 (none of the
                           split-K cases of conv_refs.CASES is 1x1; its two,
                           "splitk" and "wgrad-8way", run below as 3x3)
  3x3  N=2 7x7 64->64      padding on every border, wgrad K = 98 < 2 k-tiles
  3x3  N=1 14x14 256->256  dgrad splits 4: the BN-stats reduce and its slab

The conv bindings refuse channel counts that are no multiple of 8 and allocate
every output themselves, so through them both problems of a grid always take
the same epilogue. The launcher decides each problem's epilogue on its own,
though, so test_pair_mixed_epilogues drives it through the extension's test
hook pipe8_gemm_pair: the two GEMM kinds of a 1x1 pair on plain matrices,
written into the caller's buffers, with one problem's N no multiple of the
16-byte group (or its output base off a 16-byte boundary) and the other's
whole; the one grid against the two separate 8-wave launches, torch.equal.

test_pair_decode needs no GPU: it pins the workgroup -> (problem, tile, split)
map of the pair grid to the two separate dim3(nwg, splits) grids.
"""
import functools

import pytest
import torch

import conv_refs as cr

gpu = pytest.mark.gpu
DEV = "cuda"
EPS, MOM = 1e-5, 0.1

# id -> (N, C, H, W, Kout, R, pad), stride 1
GEOMS = {
    "1x1-ragged": (2, 72, 9, 9, 136, 1, 0),
    "1x1-one-tile": (1, 128, 8, 8, 128, 1, 0),
    "1x1-splitk": (1, 64, 64, 64, 1024, 1, 0),
    "3x3-pad": (2, 64, 7, 7, 64, 3, 1),
    "3x3-splitk-bn": (1, 256, 14, 14, 256, 3, 1),
    "3x3-refs-splitk": cr.CASES["splitk"][:6] + (1,),
    "3x3-refs-wgrad-8way": cr.CASES["wgrad-8way"][:6] + (1,),
}

# (on, dgrad_first) of set_pair_bwd
MODES = {"wgrad-first": (True, False), "dgrad-first": (True, True),
         "off": (False, False)}


@functools.lru_cache(maxsize=None)
def ext():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def restore_pair_bwd(prev):
    """prev: the mode (0, 1 or 2) a set_pair_bwd call returned."""
    ext().set_pair_bwd(prev != 0, prev == 2)


class knobs:
    """set_pair_bwd / set_epilogue_vec for a block; puts back what each call
    reported as the setting it replaced."""

    def __init__(self, mode, vec=True):
        self.mode, self.vec = MODES[mode], vec

    def __enter__(self):
        self.prev_mode = ext().set_pair_bwd(*self.mode)
        self.prev_vec = ext().set_epilogue_vec(self.vec)

    def __exit__(self, *exc):
        restore_pair_bwd(self.prev_mode)
        ext().set_epilogue_vec(self.prev_vec)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of one geometry and the separate bindings' results, made once.
    Those bindings launch each GEMM on its own under every setting."""
    N, C, H, W, K, R, pad = GEOMS[name]
    HO, WO = H + 2 * pad - R + 1, W + 2 * pad - R + 1
    x = cr.rand_bf16((N, C, H, W), 50, device=DEV)
    w = cr.rand_bf16((K, C, R, R), 51, scale=0.5, device=DEV)
    dy = cr.rand_bf16((N, K, HO, WO), 52, device=DEV)
    # the BN(+ReLU) layer that produced x and consumes dx as its dy
    a = cr.rand_bf16((N, C, H, W), 53, scale=3.0, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(54)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    by, mean, invstd, mask = ext().bn_fwd_train(
        a, gamma, beta, EPS, True, torch.zeros(C, device=DEV),
        torch.ones(C, device=DEV), MOM, torch.empty(0))
    dx = ext().conv2d_dgrad(dy, w, H, W, 1, pad)
    dw = ext().conv2d_wgrad(x, dy, R, R, 1, pad)
    dxb, slab = ext().conv2d_dgrad_bn(dy, w, H, W, 1, pad, a, by, mean,
                                      invstd, True, mask)
    torch.cuda.synchronize()
    return dict(x=x, w=w, dy=dy, a=a, by=by, mean=mean, invstd=invstd,
                mask=mask, dx=dx, dw=dw, dxb=dxb, slab=slab)


def check_pair(name):
    N, C, H, W, K, R, pad = GEOMS[name]
    c = case(name)

    def poison_outputs():  # dx, dw and the slab are allocated by the binding
        cr.poison((N, C, H, W), c["x"])
        cr.poison((K, C, R, R), c["w"])
        if c["slab"].numel():
            cr.poison(tuple(c["slab"].shape), c["slab"])

    poison_outputs()
    dx, dw = ext().conv2d_dgrad_wgrad(c["dy"], c["w"], c["x"], H, W, R, R, pad)
    assert torch.equal(dx, c["dx"]), f"dx[{name}]"
    assert torch.equal(dw, c["dw"]), f"dw[{name}]"
    assert dw.is_contiguous(memory_format=torch.channels_last)
    poison_outputs()
    dxb, slab, dwb = ext().conv2d_dgrad_bn_wgrad(
        c["dy"], c["w"], c["x"], H, W, R, R, pad, c["a"], c["by"], c["mean"],
        c["invstd"], True, c["mask"])
    assert torch.equal(dxb, c["dxb"]), f"dx(bn)[{name}]"
    assert torch.equal(dwb, c["dw"]), f"dw(bn)[{name}]"
    assert slab.shape == c["slab"].shape and torch.equal(slab, c["slab"]), \
        f"slab[{name}]"


@gpu
def test_shapes_reach_their_paths():
    """The split counts the docstring claims (heuristics at their defaults)."""
    e = ext()
    info = e.route_info()
    if info["conv_splits_force"] >= 1 or info["wgrad_budget"] != 512:
        # the comparisons of this file hold at any split count; which paths
        # they reach is then not what the docstring says, and is not asserted
        pytest.skip("split counts forced by MPIAMD_* knobs: path coverage "
                    "of the shape list not asserted")
    N, C, H, W, K, R, pad = GEOMS["1x1-splitk"]
    assert e.conv_splits(N * H * W, C, K) == 2
    assert e.conv_wgrad_splits(K, C, N * H * W) == 8
    N, C, H, W, K, R, pad = GEOMS["1x1-ragged"]
    assert e.conv_splits(N * H * W, C, K) == 1
    N, C, H, W, K, R, pad = GEOMS["3x3-splitk-bn"]
    assert e.conv_splits(N * H * W, C, 9 * K) == 4
    assert case("3x3-splitk-bn")["slab"].numel() > 0
    assert case("1x1-ragged")["slab"].numel() == 0


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(GEOMS))
def test_pair_equals_separate(name, mode):
    with knobs(mode):
        check_pair(name)


@gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_pair_scalar_epilogue(name):
    """set_epilogue_vec(False): both problems on the one-element-per-lane
    epilogue; the reference stays the vector-epilogue result."""
    with knobs("wgrad-first", vec=False):
        check_pair(name)


# ------------------------------------------------------- mixed epilogues
# Problem 1 is the wgrad kind (c1 [2][M1][n1] fp32 = a1^T b1, two k-tiles, one
# per split), problem 2 the dgrad kind (c2 = a2 b2: [M2][n2] bf16 unsplit, or
# [2][M2][n2] fp32 slabs). Two row tiles each, problem 2 two column tiles.
PM1, PK1, PLDB1 = 136, 100, 80
PM2, PK2, PLDB2 = 130, 136, 144
# whole: a multiple of 8 (the 16-byte group of bf16, two of fp32), the vector
# epilogue's condition on N; ragged: no multiple of 4, scalar for either type
PN1 = {"whole": 72, "ragged": 70}
PN2 = {"whole": 136, "ragged": 134}
GUARD = 16  # NaN elements kept on either side of an output


@functools.lru_cache(maxsize=None)
def plain_inputs():
    return (cr.rand_bf16((PK1, PM1), 80, device=DEV),
            cr.rand_bf16((PK1, PLDB1), 81, device=DEV),
            cr.rand_bf16((PM2, PK2), 82, device=DEV),
            cr.rand_bf16((PK2, PLDB2), 83, device=DEV))


@functools.lru_cache(maxsize=None)
def plain_refs(n1, n2):
    """fp64 products and the fp32-accumulation bounds of both problems."""
    a1, b1, a2, b2 = (t.double() for t in plain_inputs())
    b1, b2 = b1[:, :n1], b2[:, :n2]
    return (a1.T @ b1, PK1 * 2.0 ** -23 * (a1.abs().T @ b1.abs()),
            a2 @ b2, PK2 * 2.0 ** -23 * (a2.abs() @ b2.abs()))


def guarded(shape, dtype, shift):
    """A NaN-filled buffer and a contiguous view of `shape` in it that starts
    `shift` elements past a 16-byte boundary."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + shift:GUARD + shift + n].view(shape)


def run_plain_pair(n1, n2, c2_f32, shift1, shift2, paired, second_first):
    a1, b1, a2, b2 = plain_inputs()
    buf1, c1 = guarded((2, PM1, n1), torch.float32, shift1)
    if c2_f32:
        buf2, c2 = guarded((2, PM2, n2), torch.float32, shift2)
    else:
        buf2, c2 = guarded((PM2, n2), torch.bfloat16, shift2)
    ext().pipe8_gemm_pair(a1, b1, c1, n1, a2, b2, c2, n2, paired, second_first)
    torch.cuda.synchronize()
    for buf, c, sh in ((buf1, c1, shift1), (buf2, c2, shift2)):
        assert not torch.isnan(c).any(), "an output element was not written"
        assert torch.isnan(buf[:GUARD + sh]).all(), "write ahead of the output"
        assert torch.isnan(buf[GUARD + sh + c.numel():]).all(), \
            "write past the output"
    return c1, c2


# id -> (N of problem 1, N of problem 2, element shift of c1, of c2): which
# problem loses the 16-byte-store epilogue, and why
MIXES = {
    "p1-vec/p2-ragged-n": ("whole", "ragged", 0, 0),
    "p1-ragged-n/p2-vec": ("ragged", "whole", 0, 0),
    "p1-vec/p2-unaligned": ("whole", "whole", 0, 2),
    "p1-unaligned/p2-vec": ("whole", "whole", 1, 0),
}


@gpu
@pytest.mark.parametrize("vec", [True, False])
@pytest.mark.parametrize("second_first", [False, True])
@pytest.mark.parametrize("c2_f32", [False, True])
@pytest.mark.parametrize("mix", list(MIXES))
def test_pair_mixed_epilogues(mix, c2_f32, second_first, vec):
    """One problem on the scalar epilogue and the other on the 16-byte-store
    epilogue in the same grid (every such mix the launcher instantiates), and
    with set_epilogue_vec(False) both scalar: equal, bit for bit, to the two
    separate launches, which choose their epilogues by the same rule. The
    separate launches' result is also held to fp64: fp32 accumulation of K
    exact products errs by at most K * 2^-24 * sum|a||b| (2^-23 allowed, the
    MFMA's internal order is its own), plus one bf16 rounding, 2^-8 relative,
    for the bf16 output."""
    k1, k2, shift1, shift2 = MIXES[mix]
    n1, n2 = PN1[k1], PN2[k2]
    prev = ext().set_epilogue_vec(vec)
    try:
        want1, want2 = run_plain_pair(n1, n2, c2_f32, shift1, shift2, False,
                                      False)
        got1, got2 = run_plain_pair(n1, n2, c2_f32, shift1, shift2, True,
                                    second_first)
    finally:
        ext().set_epilogue_vec(prev)
    assert torch.equal(got1, want1), "problem 1"
    assert torch.equal(got2, want2), "problem 2"

    ref1, bound1, ref2, bound2 = plain_refs(n1, n2)
    assert ((want1.double().sum(0) - ref1).abs() <= bound1).all()
    if c2_f32:
        out2 = want2.double().sum(0)
    else:
        out2, bound2 = want2.double(), bound2 + 2.0 ** -8 * ref2.abs()
    assert ((out2 - ref2).abs() <= bound2).all()


@gpu
def test_set_pair_bwd_returns_previous():
    e = ext()
    prev = e.set_pair_bwd(False)
    try:
        assert prev in (0, 1, 2)
        assert e.set_pair_bwd(True) == 0
        assert e.set_pair_bwd(True, True) == 1
        assert e.set_pair_bwd(False, True) == 2  # off: the order is dropped
        assert e.set_pair_bwd(False) == 0
    finally:
        restore_pair_bwd(prev)
    assert e.set_pair_bwd(prev != 0, prev == 2) == prev


@gpu
def test_pair_rejects_mismatched_geometry():
    c = case("3x3-pad")
    N, C, H, W, K, R, pad = GEOMS["3x3-pad"]
    with pytest.raises(RuntimeError):  # x is not H x W
        ext().conv2d_dgrad_wgrad(c["dy"], c["w"], c["x"], H + 1, W, R, R, pad)
    with pytest.raises(RuntimeError):  # dy is not the pad-0 output
        ext().conv2d_dgrad_wgrad(c["dy"], c["w"], c["x"], H, W, R, R, 0)


# ---------------------------------------------------------------- model level
def make_block(stride, down):
    import torch.nn as nn

    from mpi_operator_amd.models.resnet import Bottleneck
    from mpi_operator_amd.ops import BatchNormReLU, Conv2d

    torch.manual_seed(0)
    ds = None
    if down:
        ds = nn.Sequential(Conv2d(64, 128, 1, stride=stride),
                           BatchNormReLU(128, relu=False))
    net = Bottleneck(64 if down else 128, 32, stride, ds).to(DEV)
    for m in net.modules():
        if isinstance(m, Conv2d):
            m.to(torch.bfloat16)
    net = net.to(memory_format=torch.channels_last)
    net.train()
    return net


def block_step(net, xv, state):
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    x = xv.detach().clone().requires_grad_(True)
    out = net(x)
    out.float().pow(2).mean().backward()
    res = [out.detach().clone(), x.grad.detach().clone()]
    res += [p.grad.detach().clone() for p in net.parameters()]
    res += [b.detach().clone() for b in net.buffers()]
    return res


def assert_all_equal(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"tensor {i}"


@gpu
@pytest.mark.parametrize("stride,down", [(1, False), (1, True), (2, True)])
def test_bottleneck_pair_on_off(stride, down):
    """Forward and backward of one bottleneck: identity skip, stride-1
    downsample (its conv pairs too) and stride 2 (conv2 and the downsample
    keep their separate launches)."""
    net = make_block(stride, down)
    xv = cr.rand_bf16((2, 64 if down else 128, 12, 12), 60, device=DEV)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    with knobs("off"):
        ref = block_step(net, xv, state)
    for mode in ("wgrad-first", "dgrad-first"):
        with knobs(mode):
            assert_all_equal(block_step(net, xv, state), ref)


@gpu
def test_bottleneck_graph_replays_equal_eager():
    """One capture, three replays of a bottleneck step with the pair on; each
    replay equals the eager step on the same input."""
    net = make_block(1, False)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    inputs = [cr.rand_bf16((2, 128, 12, 12), s, device=DEV)
              for s in (70, 71, 72, 73)]
    with knobs("wgrad-first"):
        want = [block_step(net, xv, state) for xv in inputs[1:]]
        net.load_state_dict(state)
        xs = inputs[0].detach().clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up off the capture stream
            net(xs).float().pow(2).mean().backward()
        torch.cuda.current_stream().wait_stream(side)
        net.zero_grad(set_to_none=True)
        xs.grad = None
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = net(xs)
            out.float().pow(2).mean().backward()
        for xv, ref in zip(inputs[1:], want):
            net.load_state_dict(state)
            with torch.no_grad():
                xs.copy_(xv)
            g.replay()
            torch.cuda.synchronize()
            got = [out.detach().clone(), xs.grad.detach().clone()]
            got += [p.grad.detach().clone() for p in net.parameters()]
            got += [b.detach().clone() for b in net.buffers()]
            assert_all_equal(got, ref)


# ------------------------------------------------------------- no GPU needed
@pytest.mark.parametrize("second_first", [False, True])
@pytest.mark.parametrize("p1,p2", [
    ((1, 1, 0), (1, 1, 0)),       # one workgroup each
    ((4, 8, 0), (6, 1, 0)),       # split wgrad, unsplit dgrad, no fold
    ((32, 2, 4), (64, 1, 8)),     # both folded (nwg % 8 == 0, nwg >= 32)
    ((9, 16, 0), (40, 4, 5)),     # nblk1 no multiple of 8 ahead of a fold
    ((256, 2, 32), (3, 7, 0)),
])
def test_pair_decode(p1, p2, second_first):
    """Workgroup b of the pair grid is workgroup (x, y) of problem p's own
    dim3(nwg, splits) grid, x fastest, with that grid's XCD fold; every
    workgroup of both grids appears exactly once."""
    (nwg1, sp1, cpx1), (nwg2, sp2, cpx2) = p1, p2
    n1, n2 = nwg1 * sp1, nwg2 * sp2

    def own_grid(nwg, splits, cpx):  # pipe_mix8_k's decode of blockIdx
        out = []
        for y in range(splits):
            for x in range(nwg):
                out.append(((x & 7) * cpx + (x >> 3) if cpx else x, y))
        return out

    want = [(0, t, s) for t, s in own_grid(nwg1, sp1, cpx1)]
    want2 = [(1, t, s) for t, s in own_grid(nwg2, sp2, cpx2)]
    want = want2 + want if second_first else want + want2
    got = [tuple(ext().pair_decode(b, n1, nwg1, cpx1, n2, nwg2, cpx2,
                                   second_first)) for b in range(n1 + n2)]
    assert got == want
    assert len(set(got)) == n1 + n2
