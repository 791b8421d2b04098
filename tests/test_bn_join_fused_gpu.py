"""BN-backward statistics fused into the residual-join gradient kernel
(join_bwd_stats, MPIAMD_FUSEBN_JOIN) against the kernels it replaces:
add_relu_bwd_add_mask / add_bf16 for the gradient sum, bn_bwd's partials pass
for the statistics. The fused kernel keeps the sum's roundings and
bn_partials' row assignment and accumulation order, so every comparison here
is torch.equal — no tolerance anywhere in this file."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.3


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def rand_cl(*shape, seed=0, scale=1.0):
    torch.manual_seed(seed)
    t = ((torch.rand(*shape, device="cuda") * 2 - 1) * scale).to(torch.bfloat16)
    return cl(t)


# ---------------------------------------------------------------- kernel level
# rows_per_block = 256 / C8; the partials grid is capped at 512 blocks.
# (N, C, H, W)
SHAPES = [
    (4, 64, 96, 96),    # M=36864, 32 rows/block: every block loops > once
    (1, 64, 5, 1),      # M=5: a single block, no second row
    (7, 192, 11, 13),   # M=1001 (odd), C8=24: 10 rows/block, 16 idle threads
    (2, 2048, 23, 23),  # M=1058, C8=256: 1 row/block, grid capped, odd tail
]


@functools.lru_cache(maxsize=None)
def kernel_case(shape):
    """Inputs of one shape and the unfused references, computed once and
    shared by the four (JOIN, NSTAT) variants; nothing here is modified."""
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    N, C, H, W = shape
    M = N * H * W
    a = rand_cl(N, C, H, W, seed=1)
    b = rand_cl(N, C, H, W, seed=2)
    torch.manual_seed(3)
    jmask = torch.randint(0, 256, (M, C // 8), device="cuda", dtype=torch.uint8)
    cmask = torch.randint(0, 256, (M, C // 8), device="cuda", dtype=torch.uint8)
    cons = []  # the consumer BN layers: bn3, then the downsample BN
    for seed in (4, 5):
        x = rand_cl(N, C, H, W, seed=seed, scale=3.0)
        torch.manual_seed(seed + 10)
        gamma = torch.rand(C, device="cuda") + 0.5
        beta = torch.randn(C, device="cuda") * 0.2
        y, mean, invstd, _ = ext.bn_fwd_train(
            x, gamma, beta, EPS, True, torch.zeros(C, device="cuda"),
            torch.ones(C, device="cuda"), MOM, torch.empty(0))
        cons.append((x, y, gamma, mean, invstd))
    dxt_ref = {1: ext.add_relu_bwd_add_mask(a, jmask, b),
               0: ext.add_bf16(a, b)}
    bwd_ref = {}
    for join, dxt in dxt_ref.items():
        for k, (x, y, gamma, mean, invstd) in enumerate(cons):
            bwd_ref[join, k] = ext.bn_bwd(dxt, x, y, gamma, mean, invstd,
                                          True, cmask)
    return ext, a, b, jmask, cmask, cons, dxt_ref, bwd_ref


@pytest.mark.parametrize("nstat", [1, 2])
@pytest.mark.parametrize("join", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_join_stats_kernel(shape, join, nstat):
    ext, a, b, jmask, cmask, cons, dxt_ref, bwd_ref = kernel_case(shape)
    e = torch.empty(0)
    x0, _, _, mean0, invstd0 = cons[0]
    x1, _, _, mean1, invstd1 = cons[1]
    res = ext.join_bwd_stats(a, jmask if join else e, b, x0, mean0, invstd0,
                             cmask, x1 if nstat == 2 else e,
                             mean1 if nstat == 2 else e,
                             invstd1 if nstat == 2 else e)
    assert len(res) == 1 + nstat
    dxt = res[0]
    assert torch.equal(dxt, dxt_ref[join])
    for k in range(nstat):
        x, y, gamma, mean, invstd = cons[k]
        slab = res[1 + k]
        assert slab.dim() == 3 and slab.shape[1] == 2 and slab.shape[2] == shape[1]
        dx, dg, db = ext.bn_bwd_pre(dxt, slab, x, y, gamma, mean, invstd,
                                    True, cmask)
        dx_r, dg_r, db_r = bwd_ref[join, k]
        assert torch.equal(dg, dg_r), k
        assert torch.equal(db, db_r), k
        assert torch.equal(dx, dx_r), k


def test_join_stats_rejects_bad_arguments():
    ext, a, b, jmask, cmask, cons, _, _ = kernel_case(SHAPES[1])
    e = torch.empty(0)
    x0, _, _, mean0, invstd0 = cons[0]
    with pytest.raises(RuntimeError):  # the consumer mask is required
        ext.join_bwd_stats(a, jmask, b, x0, mean0, invstd0, e, e, e, e)
    with pytest.raises(RuntimeError):  # shape mismatch
        ext.join_bwd_stats(a, jmask, b, rand_cl(1, 64, 4, 1), mean0, invstd0,
                           cmask, e, e, e)
    with pytest.raises(RuntimeError):  # statistics of another width
        ext.join_bwd_stats(a, jmask, b, x0, mean0[:32], invstd0, cmask,
                           e, e, e)


# ----------------------------------------------------------------- block level
class CountingExt:
    """The extension module with the entry points of this path wrapped, so a
    silent fallback to the unfused kernels cannot pass for the fused route."""

    def __init__(self, ext):
        self._ext = ext
        self.joins = []        # number of slabs of each join_bwd_stats call
        self.join_slabs = []   # the slabs those calls returned
        self.pre_from_join = 0  # bn_bwd_pre calls fed by one of them
        self.add_bf16_calls = 0
        self.add_mask_calls = 0

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def join_bwd_stats(self, *args):
        res = self._ext.join_bwd_stats(*args)
        self.joins.append(len(res) - 1)
        self.join_slabs += list(res[1:])
        return res

    def bn_bwd_pre(self, dy, slab, *args):
        if any(slab is s for s in self.join_slabs):
            self.pre_from_join += 1
        return self._ext.bn_bwd_pre(dy, slab, *args)

    def add_bf16(self, *args):
        self.add_bf16_calls += 1
        return self._ext.add_bf16(*args)

    def add_relu_bwd_add_mask(self, *args):
        self.add_mask_calls += 1
        return self._ext.add_relu_bwd_add_mask(*args)


@pytest.fixture(scope="module")
def blocks():
    """A downsample bottleneck followed by two plain ones, 32→8→32 channels."""
    import torch.nn as nn

    from mpi_operator_amd.models.resnet import Bottleneck
    from mpi_operator_amd.ops import BatchNormReLU, Conv2d

    torch.manual_seed(0)
    ds = nn.Sequential(Conv2d(32, 32, 1), BatchNormReLU(32, relu=False))
    net = nn.Sequential(Bottleneck(32, 8, 1, ds), Bottleneck(32, 8),
                        Bottleneck(32, 8)).to("cuda")
    for m in net.modules():
        if isinstance(m, Conv2d):
            m.to(torch.bfloat16)
    net = net.to(memory_format=torch.channels_last)
    net.train()
    return net


def block_input(seed=20):
    return rand_cl(2, 32, 16, 16, seed=seed)


def chain_loss(net, x):
    return net(x).float().pow(2).mean()


def branch_loss(net, x):
    """The middle block's output also feeds a second consumer, so the dout it
    receives is a sum and not the next block's dxt."""
    h = net[1](net[0](x))
    return net[2](h).float().pow(2).mean() + h.float().pow(2).mean()


def grads_of(net, x):
    out = [x.grad.detach().clone()]
    out += [p.grad.detach().clone() for p in net.parameters()]
    return out


def run(net, xv, monkeypatch, gate, loss_fn=chain_loss, backwards=1):
    """Forward + backward with the join gate set; returns (gradients of the
    LAST backward, the call counts)."""
    from mpi_operator_amd.ops import fused_block, hip_ext

    monkeypatch.setattr(fused_block, "_FUSEBN", True)
    monkeypatch.setattr(fused_block, "_FUSEBN_JOIN", gate)
    counting = CountingExt(hip_ext())
    monkeypatch.setattr(fused_block, "hip_ext", lambda: counting)
    x = xv.detach().clone().requires_grad_(True)
    loss = loss_fn(net, x)
    for i in range(backwards):
        net.zero_grad(set_to_none=True)
        x.grad = None
        loss.backward(retain_graph=i + 1 < backwards)
    return grads_of(net, x), counting


def assert_all_equal(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), i


def test_three_blocks_gate_on_equals_off(blocks, monkeypatch):
    xv = block_input()
    ref, c_off = run(blocks, xv, monkeypatch, False)
    assert c_off.joins == [] and c_off.pre_from_join == 0
    assert c_off.add_bf16_calls == 1 and c_off.add_mask_calls == 2
    got, c_on = run(blocks, xv, monkeypatch, True)
    # block 2 → block 1's bn3 (one slab); block 1 → block 0's bn3 and
    # downsample BN (two slabs); block 0 has no producer: plain add_bf16
    assert c_on.joins == [1, 2]
    assert c_on.pre_from_join == 3
    assert c_on.add_bf16_calls == 1 and c_on.add_mask_calls == 0
    assert_all_equal(got, ref)


def test_second_consumer_falls_back(blocks, monkeypatch):
    xv = block_input(seed=21)
    ref, _ = run(blocks, xv, monkeypatch, False, loss_fn=branch_loss)
    got, c_on = run(blocks, xv, monkeypatch, True, loss_fn=branch_loss)
    # block 1's dout is not block 2's dxt: its bn3 runs the partials pass;
    # block 0's two BNs still take block 1's slabs
    assert c_on.joins == [1, 2] and c_on.pre_from_join == 2
    assert_all_equal(got, ref)


def test_second_backward_retain_graph(blocks, monkeypatch):
    xv = block_input(seed=22)
    ref, _ = run(blocks, xv, monkeypatch, False)
    got, _ = run(blocks, xv, monkeypatch, True, backwards=2)
    assert_all_equal(got, ref)


def test_graph_capture_replays(blocks, monkeypatch):
    from mpi_operator_amd.ops import fused_block, hip_ext

    inputs = [block_input(seed=s) for s in (30, 31, 32)]
    refs = [run(blocks, xv, monkeypatch, False)[0] for xv in inputs[1:]]

    monkeypatch.setattr(fused_block, "_FUSEBN_JOIN", True)
    monkeypatch.setattr(fused_block, "hip_ext", hip_ext)
    xs = inputs[0].detach().clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture stream
        chain_loss(blocks, xs).backward()
    torch.cuda.current_stream().wait_stream(side)
    blocks.zero_grad(set_to_none=True)
    xs.grad = None
    counting = CountingExt(hip_ext())
    monkeypatch.setattr(fused_block, "hip_ext", lambda: counting)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain_loss(blocks, xs).backward()
    assert counting.joins == [1, 2] and counting.pre_from_join == 3
    for xv, ref in zip(inputs[1:], refs):
        with torch.no_grad():
            xs.copy_(xv)
        g.replay()
        torch.cuda.synchronize()
        assert_all_equal(grads_of(blocks, xs), ref)
