"""BatchNorm statistics fused into the conv GEMM epilogue (unsplit routes),
the forward split-K reduce and the dgrad split-K reduce, against the unfused
conv2d_fwd / bn_fwd_train / conv2d_dgrad / bn_bwd kernels on the same inputs.

The fused convs must return the bit-identical tensor (same GEMM kernel, same
split-K summation order); the statistics may differ only in fp32 summation
order on the epilogue routes and must be bit-identical on the split-K routes
(the reduce keeps bn_partials' row assignment and accumulation order)."""
import copy

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


def relerr(a, b):  # the metric of tests/test_ops_gpu.py
    d = (a.float() - b.float()).abs().max().item()
    s = b.float().abs().max().item() + 1e-6
    return d / s


def conv_splits(M, ncols, K):
    """The bindings' split-K choice (bindings.cpp conv_splits)."""
    tiles = ((M + 127) // 128) * ((ncols + 127) // 128)
    nk = (K + 63) // 64
    if tiles >= 256 or nk < 16:
        return 1
    return max(1, min(512 // tiles, nk // 8, 16))


def out_hw(H, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1


def check_slab_sums(y, slab):
    """Per channel: slab rows summed in fp64 vs Σy, Σy² of the returned bf16 y
    in fp64; bounds 1e-5·Σ|y| and 1e-5·Σy² (≈170 fp32 eps — a dropped or
    doubled row moves a sum by ≥ 1/M ≈ 1e-4 at these sizes)."""
    C = y.shape[1]
    assert slab.dim() == 3 and slab.shape[1] == 2 and slab.shape[2] == C
    y2d = y.permute(0, 2, 3, 1).reshape(-1, C).double()
    s = slab.double().sum(0)
    d0 = (s[0] - y2d.sum(0)).abs()
    d1 = (s[1] - (y2d * y2d).sum(0)).abs()
    b0 = 1e-5 * y2d.abs().sum(0)
    b1 = 1e-5 * (y2d * y2d).sum(0)
    print("slab sum err/bound:", (d0 / b0.clamp_min(1e-30)).max().item(),
          (d1 / b1.clamp_min(1e-30)).max().item())
    assert bool((d0 <= b0).all()), (d0 / b0.clamp_min(1e-30)).max().item()
    assert bool((d1 <= b1).all()), (d1 / b1.clamp_min(1e-30)).max().item()


def check_bn_pre(ext, y, slab, exact):
    """bn_fwd_train_pre(slab) vs bn_fwd_train on the same y, with and
    without a residual."""
    C = y.shape[1]
    torch.manual_seed(5)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda") * 0.2
    for res in (torch.empty(0), rand_cl(*y.shape, seed=6)):
        rm_u, rv_u = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        rm_f, rv_f = rm_u.clone(), rv_u.clone()
        o_u, m_u, i_u, k_u = ext.bn_fwd_train(y, gamma, beta, EPS, True, rm_u,
                                              rv_u, MOM, res)
        o_f, m_f, i_f, k_f = ext.bn_fwd_train_pre(y, slab, gamma, beta, EPS,
                                                  True, rm_f, rv_f, MOM, res)
        print("mean/invstd/rm/rv/out relerr:", relerr(m_f, m_u),
              relerr(i_f, i_u), relerr(rm_f, rm_u), relerr(rv_f, rv_u),
              relerr(o_f, o_u))
        assert relerr(m_f, m_u) < 1e-3
        assert relerr(i_f, i_u) < 1e-3
        assert relerr(rm_f, rm_u) < 1e-3
        assert relerr(rv_f, rv_u) < 1e-3
        assert relerr(o_f, o_u) < 0.02
        if exact:
            assert torch.equal(m_f, m_u) and torch.equal(i_f, i_u)
            assert torch.equal(rm_f, rm_u) and torch.equal(rv_f, rv_u)
            assert torch.equal(o_f, o_u) and torch.equal(k_f, k_u)


def run_fwd_case(geom, want_splits):
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    N, C, H, W, K, R, st, pad = geom
    HO, WO = out_hw(H, R, st, pad), out_hw(W, R, st, pad)
    splits = conv_splits(N * HO * WO, K, R * R * C)
    assert splits == want_splits, splits  # the case exercises what it claims
    x = rand_cl(N, C, H, W, seed=10)
    w = rand_cl(K, C, R, R, seed=11, scale=0.5)
    y_ref = ext.conv2d_fwd(x, w, st, pad)
    y, slab = ext.conv2d_fwd_bn(x, w, st, pad, True, True)
    assert slab.numel() > 0  # the fused route was really taken
    assert torch.equal(y, y_ref)
    check_slab_sums(y, slab)
    check_bn_pre(ext, y, slab, exact=splits > 1)
    return ext, x, w, y_ref


# N, C, H, W, Kout, R, stride, pad
UNSPLIT = [
    (2, 64, 7, 7, 64, 1, 1, 0),       # M=98: 1 tile, 2nd band 34 rows, Kout<tile
    (2, 64, 14, 14, 256, 1, 1, 0),    # M=392: last M-tile 8 rows, 2 N-tiles
    (2, 64, 16, 16, 64, 3, 1, 1),     # 3x3 gather
    (2, 64, 15, 15, 64, 3, 2, 1),     # stride-2 gather, odd H/W
    (2, 8, 32, 32, 64, 7, 2, 3),      # stem-like, C=8
    (8, 64, 16, 16, 256, 1, 1, 0),    # 32 tiles: the XCD tile-fold path
    (32, 64, 16, 16, 1024, 1, 1, 0),  # 128 tiles of 256²: the 16-wave route
]

SPLIT = [
    ((2, 1024, 7, 7, 256, 1, 1, 0), 2),
    ((2, 2048, 7, 7, 128, 1, 1, 0), 4),
    ((64, 512, 7, 7, 512, 3, 1, 1), 5),   # the stage-4 3x3 shape itself
    ((2, 512, 7, 7, 128, 3, 1, 1), 9),    # runtime-count path
    ((2, 128, 15, 15, 64, 3, 2, 1), 2),   # stride-2 gather
]


@pytest.mark.parametrize("geom", UNSPLIT)
def test_epilogue_stats_unsplit(geom):
    ext, x, w, y_ref = run_fwd_case(geom, 1)
    # the epilogue flag off: unfused conv, empty slab
    y, slab = ext.conv2d_fwd_bn(x, w, geom[6], geom[7], True, False)
    assert slab.numel() == 0 and torch.equal(y, y_ref)


@pytest.mark.parametrize("geom,splits", SPLIT)
def test_splitk_reduce_stats_fwd(geom, splits):
    ext, x, w, y_ref = run_fwd_case(geom, splits)
    # the sub-gate off: unfused conv, empty slab
    y, slab = ext.conv2d_fwd_bn(x, w, geom[6], geom[7], False, True)
    assert slab.numel() == 0 and torch.equal(y, y_ref)


# dgrads of the stride-1 split geometries; as dgrads the first two do not
# split (K = R·S·Kout is short) and must take the unfused pair unchanged, so
# their channel-swapped twins (the conv3-dgrad role: many output channels
# reduced onto few) are added to cover dgrad splits 2 and 4 on 1x1.
DGRAD = [
    ((2, 1024, 7, 7, 256, 1, 1, 0), 1),
    ((2, 2048, 7, 7, 128, 1, 1, 0), 1),
    ((64, 512, 7, 7, 512, 3, 1, 1), 5),
    ((2, 512, 7, 7, 128, 3, 1, 1), 2),
    ((2, 256, 7, 7, 1024, 1, 1, 0), 2),
    ((2, 128, 7, 7, 2048, 1, 1, 0), 4),
]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("geom,splits", DGRAD)
def test_splitk_reduce_stats_bwd(geom, splits, relu):
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    N, C, H, W, K, R, st, pad = geom
    HO, WO = out_hw(H, R, st, pad), out_hw(W, R, st, pad)
    assert conv_splits(N * H * W, C, R * R * K) == splits
    w = rand_cl(K, C, R, R, seed=11, scale=0.5)
    dyo = rand_cl(N, K, HO, WO, seed=12)
    # the BN layer that consumes the dgrad result as its dy
    a = rand_cl(N, C, H, W, seed=13, scale=3.0)
    torch.manual_seed(7)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda") * 0.2
    by, mean, invstd, mask = ext.bn_fwd_train(
        a, gamma, beta, EPS, relu, torch.zeros(C, device="cuda"),
        torch.ones(C, device="cuda"), MOM, torch.empty(0))

    dy_ref = ext.conv2d_dgrad(dyo, w, H, W, st, pad)
    dx_ref, dg_ref, db_ref = ext.bn_bwd(dy_ref, a, by, gamma, mean, invstd,
                                        relu, mask)
    masks = [mask]
    if relu:  # the mask-less (y > 0) gating path as well
        masks.append(torch.empty(0, dtype=torch.uint8, device="cuda"))
    for mk in masks:
        dy, slab = ext.conv2d_dgrad_bn(dyo, w, H, W, st, pad, a, by, mean,
                                       invstd, relu, mk)
        assert torch.equal(dy, dy_ref)
        if splits == 1:
            assert slab.numel() == 0
            continue
        assert slab.numel() > 0
        dx, dg, db = ext.bn_bwd_pre(dy, slab, a, by, gamma, mean, invstd,
                                    relu, mk)
        print("dgamma/dbeta/dx relerr:", relerr(dg, dg_ref),
              relerr(db, db_ref), relerr(dx, dx_ref))
        assert relerr(dg, dg_ref) < 5e-3
        assert relerr(db, db_ref) < 5e-3
        assert relerr(dx, dx_ref) < 0.05
        # row assignment and accumulation order of bn_partials are kept
        assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
        assert torch.equal(dx, dx_ref)


def block_relerr(a, b):  # the metric of tests/test_fused_block_gpu.py
    a, b = a.float(), b.float()
    return (a - b).norm().item() / (b.norm().item() + 1e-12)


def run_block(block, x, fused):  # as tests/test_fused_block_gpu.py
    from mpi_operator_amd.ops import add_relu
    block.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    if fused:
        out = block(x)  # training + cuda → fused path
    else:
        h = block.bn1(block.conv1(x))
        h = block.bn2(block.conv2(h))
        h = block.bn3(block.conv3(h))
        out = add_relu(h, x)
    out.float().pow(2).mean().backward()
    grads = {n: p.grad.detach().clone() for n, p in block.named_parameters()}
    return out.detach(), x.grad.detach().clone(), grads


def test_bottleneck_that_splits(monkeypatch):
    """Bottleneck(1024, 256, stride 1) on [2,1024,7,7]: conv1 splits 2 and
    conv2 splits 4 forward; the conv3 and conv2 dgrads split backward."""
    from mpi_operator_amd.models.resnet import Bottleneck
    from mpi_operator_amd.ops import Conv2d, fused_block

    for gate in ("_FUSEBN", "_FUSEBN_EPI", "_FUSEBN_SPLITK", "_FUSEBN_BWD"):
        monkeypatch.setattr(fused_block, gate, True)
    assert conv_splits(98, 256, 1024) == 2 and conv_splits(98, 256, 9 * 256) == 4

    torch.manual_seed(0)
    blk = Bottleneck(1024, 256, 1, None).to("cuda")
    for m in blk.modules():
        if isinstance(m, Conv2d):
            m.to(torch.bfloat16)
    blk = blk.to(memory_format=torch.channels_last)
    blk.train()
    x = cl((torch.rand(2, 1024, 7, 7, device="cuda") * 2 - 1).to(torch.bfloat16))

    blk_ref = copy.deepcopy(blk)
    out_f, dx_f, g_f = run_block(blk, x, fused=True)
    out_u, dx_u, g_u = run_block(blk_ref, x, fused=False)
    assert block_relerr(out_f, out_u) < 0.02, block_relerr(out_f, out_u)
    assert block_relerr(dx_f, dx_u) < 0.03, block_relerr(dx_f, dx_u)
    for n in g_u:
        assert block_relerr(g_f[n], g_u[n]) < 0.03, (n, block_relerr(g_f[n], g_u[n]))
    for (n, b_f), (_, b_u) in zip(blk.named_buffers(), blk_ref.named_buffers()):
        assert block_relerr(b_f, b_u) < 1e-3, n
