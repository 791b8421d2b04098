"""The software-pipelined BN statistics producers (set_bn_pipelined) and the
line-coalesced BN finalize (set_bn_finalize_coalesced) against the kernels
they replace. Both change only how bytes move: every comparison here is
torch.equal between the two settings of a setter in one process — no
tolerance anywhere in this file.

Shapes follow the pipeline depth D = 1 (MPIAMD_BN_PIPE_DEPTH in
batchnorm.hip): a thread runs one pair-iteration per 2·grid·rows_per_block
rows, the grid is capped at 512 blocks, and the cases below make threads run
0, 1, D, D + 1 and >= 2D + 1 pair-iterations with an odd last row. The
launchers take the pipelined kernels only where a thread runs more than two
pair-iterations and only for the bitmask-gated forms; for the other cases the
switch must change nothing, which is the same assertion."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.3
D = 1


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def rand_cl(*shape, seed=0, scale=1.0):
    torch.manual_seed(seed)
    t = ((torch.rand(*shape, device="cuda") * 2 - 1) * scale).to(torch.bfloat16)
    return cl(t)


def ext_():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def both(setter_name, fn):
    """fn() under setter(False) and setter(True); the previous value is put
    back whatever happens. Returns (old, new)."""
    setter = getattr(ext_(), setter_name)
    prev = setter(False)
    try:
        old = fn()
        assert setter(True) is False
        new = fn()
    finally:
        setter(prev)
    return old, new


def assert_all_equal(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, i
        assert torch.equal(g, w), i


def test_setters_return_previous_value():
    ext = ext_()
    for name in ("set_bn_pipelined", "set_bn_finalize_coalesced"):
        setter = getattr(ext, name)
        prev = setter(False)
        try:
            assert setter(True) is False
            assert setter(True) is True
        finally:
            setter(prev)


# ------------------------------------------------------------------ producers
# (M, C): rows_per_block = 2048 / C, grid = min(512, ceil(M / rows_per_block)),
# one pair-iteration covers 2 · grid · rows_per_block rows.
PRODUCER_SHAPES = [
    (5, 64),                            # a single block; rows 5.. run 0 times
    (300, 2048),                        # 1 pair-iteration, no second row
    (512 * 2 * D + 37, 2048),           # D and D + 1, second row missing
    (512 * 4, 2048),                    # 2 each: the last size not pipelined
    (512 * 4 + 1, 2048),                # 2 and 3: the first pipelined size
    (512 * 2 * (2 * D + 1) + 37, 2048),  # 2D + 1 and 2D + 2, grid capped
    (16384 * 2 * (2 * D + 1) + 5, 64),  # 32 rows/block, 2D + 1 (+1 for 5 rows)
    (1001, 192),                        # C8 = 24: 16 idle threads, odd M
    (5120 * 2 * (D + 1) + 7, 192),      # ... and D + 1, D + 2 pair-iterations
]


@functools.lru_cache(maxsize=None)
def producer_case(M, C):
    """Inputs of one shape, computed once and shared; nothing here is
    modified by the tests."""
    ext = ext_()
    a = rand_cl(1, C, M, 1, seed=1)
    b = rand_cl(1, C, M, 1, seed=2)
    torch.manual_seed(3)
    jmask = torch.randint(0, 256, (M, C // 8), device="cuda", dtype=torch.uint8)
    cons = []
    for seed in (4, 5):
        x = rand_cl(1, C, M, 1, seed=seed, scale=3.0)
        torch.manual_seed(seed + 10)
        gamma = torch.rand(C, device="cuda") + 0.5
        beta = torch.randn(C, device="cuda") * 0.2
        cons.append((x, gamma, beta))
    return ext, a, b, jmask, cons


def fresh_running(C):
    return torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("M,C", PRODUCER_SHAPES)
def test_bn_fwd_bwd_pipelined_equals_plain(M, C, relu):
    ext, a, _, _, cons = producer_case(M, C)
    x, gamma, beta = cons[0]
    e = torch.empty(0)

    def run():
        out = []
        for res in (e, a):
            rm, rv = fresh_running(C)
            y, mean, invstd, mask = ext.bn_fwd_train(x, gamma, beta, EPS, relu,
                                                     rm, rv, MOM, res)
            out += [y, mean, invstd, mask, rm, rv]
        # backward with the bitmask and, under relu, with the y > 0 gate
        masks = [mask, torch.empty(0, dtype=torch.uint8, device="cuda")]
        for mk in masks if relu else masks[:1]:
            out += ext.bn_bwd(a, x, y, gamma, mean, invstd, relu, mk)
        return out

    old, new = both("set_bn_pipelined", run)
    assert_all_equal(new, old)


@pytest.mark.parametrize("nstat", [1, 2])
@pytest.mark.parametrize("join", [1, 0])
@pytest.mark.parametrize("M,C", PRODUCER_SHAPES)
def test_join_stats_pipelined_equals_plain(M, C, join, nstat):
    ext, a, b, jmask, cons = producer_case(M, C)
    e = torch.empty(0)
    stats = []
    for x, gamma, beta in cons:
        rm, rv = fresh_running(C)
        _, mean, invstd, mask = ext.bn_fwd_train(x, gamma, beta, EPS, True, rm,
                                                 rv, MOM, e)
        stats.append((x, mean, invstd, mask))
    x0, mean0, invstd0, cmask = stats[0]
    x1, mean1, invstd1, _ = stats[1]

    def run():
        return ext.join_bwd_stats(a, jmask if join else e, b, x0, mean0,
                                  invstd0, cmask, x1 if nstat == 2 else e,
                                  mean1 if nstat == 2 else e,
                                  invstd1 if nstat == 2 else e)

    old, new = both("set_bn_pipelined", run)
    assert len(new) == 1 + nstat
    assert_all_equal(new, old)


# conv shapes whose split-K reduce carries the statistics. The reduce+stats
# kernels have no pipelined form (a conv that splits has M·C < 2^22, so no
# thread runs more than two pair-iterations, and a pipelined form measured no
# faster): what is held here is that the switch leaves these routes alone.
# (N, C, H, W, Kout, R, stride, pad), splits
FWD_SPLIT = [
    ((2, 1024, 7, 7, 256, 1, 1, 0), 2),
    ((2, 1536, 7, 7, 256, 1, 1, 0), 3),
    ((2, 2048, 7, 7, 128, 1, 1, 0), 4),
    ((16, 1024, 7, 7, 256, 1, 1, 0), 2),  # M = 784: a second pair-iteration
]
DGRAD_SPLIT = [
    ((2, 256, 7, 7, 1024, 1, 1, 0), 2),
    ((2, 128, 7, 7, 2048, 1, 1, 0), 4),
    ((16, 256, 7, 7, 1024, 1, 1, 0), 2),
]


def conv_fwd_outputs(ext, geom):
    N, C, H, W, K, R, st, pad = geom
    x = rand_cl(N, C, H, W, seed=10)
    w = rand_cl(K, C, R, R, seed=11, scale=0.5)

    def run():
        y, slab = ext.conv2d_fwd_bn(x, w, st, pad, True, False)
        assert slab.numel() > 0  # the reduce+stats route was really taken
        return [y, slab]
    return run


def conv_dgrad_outputs(ext, geom, relu):
    N, C, H, W, K, R, st, pad = geom
    w = rand_cl(K, C, R, R, seed=11, scale=0.5)
    dyo = rand_cl(N, K, H, W, seed=12)
    a = rand_cl(N, C, H, W, seed=13, scale=3.0)
    torch.manual_seed(7)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda") * 0.2
    rm, rv = fresh_running(C)
    by, mean, invstd, mask = ext.bn_fwd_train(a, gamma, beta, EPS, relu, rm,
                                              rv, MOM, torch.empty(0))
    masks = [mask]
    if relu:
        masks.append(torch.empty(0, dtype=torch.uint8, device="cuda"))

    def run():
        out = []
        for mk in masks:
            dy, slab = ext.conv2d_dgrad_bn(dyo, w, H, W, st, pad, a, by, mean,
                                           invstd, relu, mk)
            assert slab.numel() > 0
            out += [dy, slab]
        return out
    return run


@pytest.mark.parametrize("geom,splits", FWD_SPLIT)
def test_conv_fwd_reduce_stats_pipelined_equals_plain(geom, splits):
    ext = ext_()
    N, C, H, W, K, R, st, pad = geom
    assert ext.conv_splits(N * H * W, K, R * R * C) == splits
    old, new = both("set_bn_pipelined", conv_fwd_outputs(ext, geom))
    assert_all_equal(new, old)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("geom,splits", DGRAD_SPLIT)
def test_conv_dgrad_reduce_stats_pipelined_equals_plain(geom, splits, relu):
    ext = ext_()
    N, C, H, W, K, R, st, pad = geom
    assert ext.conv_splits(N * H * W, C, R * R * K) == splits
    old, new = both("set_bn_pipelined", conv_dgrad_outputs(ext, geom, relu))
    assert_all_equal(new, old)


# ------------------------------------------------------------- finalize alone
FIN_ROWS = [1, 2, 255, 256, 257, 512, 513, 3136]
FIN_C = [8, 24, 64, 72, 1024, 2048]  # 24 and 72 leave a partial channel slice


@functools.lru_cache(maxsize=None)
def finalize_case(C):
    ext = ext_()
    x = rand_cl(1, C, 64, 1, seed=20, scale=3.0)  # M = 64
    dy = rand_cl(1, C, 64, 1, seed=21)
    torch.manual_seed(22)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda") * 0.2
    rm, rv = fresh_running(C)
    y, mean, invstd, mask = ext.bn_fwd_train(x, gamma, beta, EPS, True, rm, rv,
                                             MOM, torch.empty(0))
    # hand-made slabs: [rows][2][C]; sum in row 0, a positive sum of squares
    torch.manual_seed(23)
    slab = torch.randn(max(FIN_ROWS), 2, C, device="cuda")
    slab[:, 1] = slab[:, 1].abs() + 1.0
    return ext, x, dy, gamma, beta, y, mean, invstd, mask, slab


@pytest.mark.parametrize("rows", FIN_ROWS)
@pytest.mark.parametrize("C", FIN_C)
def test_finalize_coalesced_equals_bands(C, rows):
    """The bands kernels (switch off) against the coalesced kernels at the
    width the launcher picks for this (C, rows) and at each width forced
    through the tuning override: below 256 channels the launcher keeps the
    bands kernel, and the override is what reaches the new kernels there."""
    ext, x, dy, gamma, beta, y, mean, invstd, mask, slab_all = finalize_case(C)
    slab = slab_all[:rows].contiguous()

    def run():
        rm, rv = fresh_running(C)
        out = ext.bn_fwd_train_pre(x, slab, gamma, beta, EPS, True, rm, rv, MOM,
                                   torch.empty(0))
        out += [rm, rv]
        out += ext.bn_bwd_pre(dy, slab, x, y, gamma, mean, invstd, True, mask)
        return out

    prev_ch = ext.set_bn_finalize_ch(0)
    try:
        for width in (0, 8, 16):
            ext.set_bn_finalize_ch(width)
            old, new = both("set_bn_finalize_coalesced", run)
            # y mean invstd mask, rm rv, dx dgamma dbeta
            assert len(new) == 4 + 2 + 3
            assert_all_equal(new, old)
    finally:
        ext.set_bn_finalize_ch(prev_ch)


def test_finalize_width_override_rejects_other_values():
    ext = ext_()
    prev = ext.set_bn_finalize_ch(8)
    try:
        assert ext.set_bn_finalize_ch(-1) == 8
        with pytest.raises(RuntimeError):
            ext.set_bn_finalize_ch(32)
        assert ext.set_bn_finalize_ch(0) == -1  # the rejected value left it
    finally:
        ext.set_bn_finalize_ch(prev)


# ---------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def block():
    """A downsample bottleneck, 64 -> 256 channels."""
    import torch.nn as nn

    from mpi_operator_amd.models.resnet import Bottleneck
    from mpi_operator_amd.ops import BatchNormReLU, Conv2d

    torch.manual_seed(0)
    ds = nn.Sequential(Conv2d(64, 256, 1), BatchNormReLU(256, relu=False))
    net = Bottleneck(64, 64, 1, ds).to("cuda")
    for m in net.modules():
        if isinstance(m, Conv2d):
            m.to(torch.bfloat16)
    net = net.to(memory_format=torch.channels_last)
    net.train()
    return net


def block_step(net, xv, state):
    """One forward + backward from the saved buffers; returns the output, the
    input gradient, every parameter gradient and every buffer afterwards."""
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    x = xv.detach().clone().requires_grad_(True)
    out = net(x)
    out.float().pow(2).mean().backward()
    res = [out.detach().clone(), x.grad.detach().clone()]
    res += [p.grad.detach().clone() for p in net.parameters()]
    res += [b.detach().clone() for b in net.buffers()]
    return res


def test_bottleneck_all_gate_combinations(block):
    ext = ext_()
    xv = rand_cl(2, 64, 16, 16, seed=30)
    state = {k: v.detach().clone() for k, v in block.state_dict().items()}
    prev_p = ext.set_bn_pipelined(False)
    prev_f = ext.set_bn_finalize_coalesced(False)
    try:
        ref = block_step(block, xv, state)
        for pipe, fin in ((True, False), (False, True), (True, True)):
            ext.set_bn_pipelined(pipe)
            ext.set_bn_finalize_coalesced(fin)
            assert_all_equal(block_step(block, xv, state), ref)
    finally:
        ext.set_bn_pipelined(prev_p)
        ext.set_bn_finalize_coalesced(prev_f)
        block.load_state_dict(state)


def test_bottleneck_graph_replay_equals_eager(block):
    """Capture and replay at the defaults (both gates on): the second replay
    equals eager."""
    ext = ext_()
    prev_p = ext.set_bn_pipelined(True)
    prev_f = ext.set_bn_finalize_coalesced(True)
    state = {k: v.detach().clone() for k, v in block.state_dict().items()}
    try:
        inputs = [rand_cl(2, 64, 16, 16, seed=s) for s in (40, 41, 42)]
        want = block_step(block, inputs[2], state)

        block.load_state_dict(state)
        xs = inputs[0].detach().clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up off the capture stream
            block(xs).float().pow(2).mean().backward()
        torch.cuda.current_stream().wait_stream(side)
        block.zero_grad(set_to_none=True)
        xs.grad = None
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = block(xs)
            out.float().pow(2).mean().backward()
        for xv in inputs[1:]:
            block.load_state_dict(state)
            with torch.no_grad():
                xs.copy_(xv)
            g.replay()
            torch.cuda.synchronize()
        got = [out.detach().clone(), xs.grad.detach().clone()]
        got += [p.grad.detach().clone() for p in block.parameters()]
        got += [b.detach().clone() for b in block.buffers()]
        assert_all_equal(got, want)
    finally:
        ext.set_bn_pipelined(prev_p)
        ext.set_bn_finalize_coalesced(prev_f)
        block.load_state_dict(state)
