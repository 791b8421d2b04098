"""GPU numerics for every hand-written kernel vs the fp32 PyTorch reference
(mpi_operator_amd.ops.reference), on identical bf16-rounded inputs."""
import pytest
import torch

from mpi_operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def rand_cl(*shape, seed=0, scale=1.0):
    torch.manual_seed(seed)
    t = ((torch.rand(*shape, device="cuda") * 2 - 1) * scale).to(torch.bfloat16)
    return cl(t)


def relerr(a, b):
    d = (a.float() - b.float()).abs().max().item()
    s = b.float().abs().max().item() + 1e-6
    return d / s


# ---------------- conv ----------------
@pytest.mark.parametrize("geom", [
    # N, C, H, W, Kout, R, stride, pad
    (2, 64, 16, 16, 128, 1, 1, 0),    # 1x1
    (2, 64, 16, 16, 64, 3, 1, 1),     # 3x3 s1
    (2, 128, 15, 15, 64, 3, 2, 1),    # 3x3 s2, odd HW
    (2, 8, 32, 32, 64, 7, 2, 3),      # stem-like 7x7 s2 C=8
    (2, 256, 14, 14, 512, 1, 2, 0),   # downsample 1x1 s2
])
def test_conv_fwd_dgrad_wgrad(geom):
    from mpi_operator_amd.ops import hip_ext
    N, C, H, W, K, R, st, pad = geom
    x = rand_cl(N, C, H, W, seed=10)
    w = rand_cl(K, C, R, R, seed=11, scale=0.5)
    ext = hip_ext()
    y = ext.conv2d_fwd(x, w, st, pad)
    yr = torch.nn.functional.conv2d(x.float(), w.float(), stride=st, padding=pad)
    assert relerr(y, yr) < 0.02, relerr(y, yr)

    dy = rand_cl(*y.shape, seed=12)
    dx = ext.conv2d_dgrad(dy, w, H, W, st, pad)
    dxr = torch.nn.grad.conv2d_input((N, C, H, W), w.float(), dy.float(),
                                     stride=st, padding=pad)
    assert relerr(dx, dxr) < 0.02, relerr(dx, dxr)

    dw = ext.conv2d_wgrad(x, dy, R, R, st, pad)
    dwr = torch.nn.grad.conv2d_weight(x.float(), (K, C, R, R), dy.float(),
                                      stride=st, padding=pad)
    assert relerr(dw, dwr) < 0.02, relerr(dw, dwr)


# ---------------- batchnorm ----------------
@pytest.mark.parametrize("C", [8, 64, 2048])
@pytest.mark.parametrize("relu", [True, False])
def test_bn_fwd_bwd(C, relu):
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    N, H, W = 4, 7, 7
    x = rand_cl(N, C, H, W, seed=20, scale=3.0)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda") * 0.2
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")
    y, mean, invstd, mask = ext.bn_fwd_train(x, gamma, beta, 1e-5, relu, rm,
                                             rv, 0.3, torch.empty(0))
    yr, mr, ir = ref.bn_relu_fwd_train(x.float().cpu(), gamma.cpu(), beta.cpu(), 1e-5, relu)
    assert relerr(mean.cpu(), mr) < 1e-3
    assert relerr(invstd.cpu(), ir) < 1e-3
    assert relerr(y.cpu(), yr) < 0.02
    # fused running-stats update
    n = N * H * W
    var_b = ir.pow(-2) - 1e-5
    assert relerr(rm.cpu(), 0.3 * mr) < 1e-3
    assert relerr(rv.cpu(), 0.7 + 0.3 * var_b * n / (n - 1)) < 1e-3

    dy = rand_cl(N, C, H, W, seed=21)
    dx, dgamma, dbeta = ext.bn_bwd(dy, x, y, gamma, mean, invstd, relu, mask)
    dxr, dgr, dbr = ref.bn_relu_bwd(dy.float().cpu(), x.float().cpu(), yr,
                                    gamma.cpu(), mr, ir, relu)
    assert relerr(dbeta.cpu(), dbr) < 5e-3
    assert relerr(dgamma.cpu(), dgr) < 5e-3
    assert relerr(dx.cpu(), dxr) < 0.05
    # mask-less backward (legacy y>0 path) must agree exactly
    dx2, dg2, db2 = ext.bn_bwd(dy, x, y, gamma, mean, invstd, relu,
                               torch.empty(0, dtype=torch.uint8))
    assert torch.equal(dx, dx2) and torch.equal(dg2, dgamma)


def test_bn_eval():
    from mpi_operator_amd.ops import functional as Fx
    C = 64
    x = rand_cl(2, C, 8, 8, seed=22)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    rm = torch.randn(C, device="cuda") * 0.1
    rv = torch.rand(C, device="cuda") + 0.5
    y = Fx.bn_relu_eval(x, gamma, beta, rm, rv)
    yr = ref.bn_relu_fwd_eval(x.float().cpu(), gamma.cpu(), beta.cpu(),
                              rm.cpu(), rv.cpu(), 1e-5, True)
    assert relerr(y.cpu(), yr) < 0.02


# ---------------- pooling / gap / add-relu ----------------
def test_maxpool_fwd_bwd():
    """y vs torch reference; idx checked by self-consistency (ties in bf16
    make torch's argmax choice non-unique, so bwd is validated against a
    python scatter using OUR indices)."""
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    N, C, H, W = 2, 64, 15, 15
    x = rand_cl(N, C, H, W, seed=30)
    y, idx = ext.maxpool_fwd(x, 3, 2, 1)
    yr, _ = ref.max_pool2d_fwd(x.float().cpu(), 3, 2, 1)
    assert relerr(y.cpu(), yr) < 0.01
    HO = WO = (H + 2 - 3) // 2 + 1
    # consistency: x at the recorded argmax equals y, and bwd scatters there
    xp = torch.nn.functional.pad(x.float().cpu(), (1, 1, 1, 1), value=float("-inf"))
    idx_c = idx.cpu().long()  # [N,HO,WO,C], values 0..8
    dy = rand_cl(N, C, HO, WO, seed=31)
    dxr = torch.zeros(N, C, H, W)
    for n in range(N):
        for ho in range(HO):
            for wo in range(WO):
                pos = idx_c[n, ho, wo]  # [C]
                r, s = pos // 3, pos % 3
                h = ho * 2 + r - 1
                w = wo * 2 + s - 1
                cvals = xp[n, torch.arange(C), h + 1, w + 1]
                assert torch.allclose(cvals.to(torch.bfloat16).float(),
                                      y.cpu()[n, :, ho, wo].float(), atol=1e-3)
                valid = (h >= 0) & (h < H) & (w >= 0) & (w < W)
                hs = h.clamp(0, H - 1)
                ws = w.clamp(0, W - 1)
                dxr[n, torch.arange(C)[valid], hs[valid], ws[valid]] += \
                    dy.float().cpu()[n, torch.arange(C)[valid], ho, wo]
    dx = ext.maxpool_bwd(dy, idx, H, W, 3, 2, 1)
    assert relerr(dx.cpu(), dxr) < 0.02


def test_gap():
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    x = rand_cl(4, 2048, 7, 7, seed=32)
    y = ext.gap_fwd(x)
    yr = ref.global_avg_pool_fwd(x.float().cpu())
    assert relerr(y.cpu(), yr) < 0.01
    dy = (torch.rand(4, 2048, device="cuda") * 2 - 1).to(torch.bfloat16)
    dx = ext.gap_bwd(dy, 7, 7)
    dxr = ref.global_avg_pool_bwd(dy.float().cpu(), x.shape)
    assert relerr(dx.cpu(), dxr) < 0.01


def test_add_relu():
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    a = rand_cl(2, 64, 9, 9, seed=33)
    b = rand_cl(2, 64, 9, 9, seed=34)
    y = ext.add_relu_fwd(a, b)
    yr = torch.relu(a.float() + b.float())
    assert relerr(y, yr) < 0.01
    dy = rand_cl(2, 64, 9, 9, seed=35)
    dx = ext.add_relu_bwd(dy, y)
    dxr = dy.float() * (yr > 0)
    assert relerr(dx, dxr) < 0.01


# ---------------- linear / softmax-xent ----------------
def test_linear_fwd_bwd():
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    torch.manual_seed(40)
    x = ((torch.rand(64, 2048, device="cuda") * 2 - 1)).to(torch.bfloat16)
    w = ((torch.rand(1000, 2048, device="cuda") * 2 - 1) * 0.05).to(torch.bfloat16)
    b = torch.randn(1000, device="cuda")
    y = ext.linear_fwd(x, w, b)
    yr = x.float() @ w.float().t() + b
    assert relerr(y, yr) < 0.02
    dy = ((torch.rand(64, 1000, device="cuda") * 2 - 1)).to(torch.bfloat16)
    dx, dw, db = ext.linear_bwd(dy, x, w)
    assert relerr(dx, dy.float() @ w.float()) < 0.02
    assert relerr(dw, dy.float().t() @ x.float()) < 0.02
    assert relerr(db, dy.float().sum(0)) < 0.01


@pytest.mark.parametrize("V", [10, 1000])
def test_softmax_xent(V):
    """V=10 is the SimpleCNN head: most of a block's 256 threads own no
    column. Two rows pin their target to the first and the last column."""
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    torch.manual_seed(41)
    logits = ((torch.rand(64, V, device="cuda") * 2 - 1) * 4).to(torch.bfloat16)
    tgt = torch.randint(0, V, (64,), device="cuda")
    tgt[0], tgt[1] = 0, V - 1
    loss, probs = ext.softmax_xent_fwd(logits, tgt)
    lr_, pr = ref.softmax_cross_entropy_fwd(logits.float().cpu(), tgt.cpu())
    assert abs(loss.item() - lr_.item()) < 2e-3 * abs(lr_.item()) + 1e-3
    assert relerr(probs.cpu(), pr) < 0.01
    d = ext.softmax_xent_bwd(probs, tgt, torch.ones(1, device="cuda"))
    dr = ref.softmax_cross_entropy_bwd(pr, tgt.cpu(), 1.0)
    assert relerr(d.cpu(), dr) < 0.02


# ---------------- sgd ----------------
def test_sgd_step():
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(42)
    shapes = [(64, 32, 3, 3), (2048,), (1000, 2048), (7,)]  # incl. non-%8 tail
    masters = [torch.randn(*s, device="cuda") for s in shapes]
    grads = [torch.randn(*s, device="cuda").to(torch.bfloat16) for s in shapes]
    moms = [torch.randn(*s, device="cuda").abs() for s in shapes]
    outs = [torch.empty(*s, device="cuda", dtype=torch.bfloat16) for s in shapes]
    m2 = [m.cpu().clone() for m in masters]
    g2 = [g.cpu() for g in grads]
    mo2 = [m.cpu().clone() for m in moms]
    o2 = [torch.empty(*s, dtype=torch.bfloat16) for s in shapes]
    Fx.sgd_momentum_step(masters, grads, moms, outs, 0.1, 0.9, 1e-4)
    ref.sgd_momentum_step(m2, g2, mo2, o2, 0.1, 0.9, 1e-4)
    for a, b in zip(masters, m2):
        assert relerr(a.cpu(), b) < 1e-5
    for a, b in zip(moms, mo2):
        assert relerr(a.cpu(), b) < 1e-5
    for a, b in zip(outs, o2):
        assert relerr(a.cpu(), b) < 1e-2


# ---------------- end-to-end ----------------
def test_resnet50_train_step_gpu():
    from mpi_operator_amd import models
    from mpi_operator_amd.optim import FusedSGD
    torch.manual_seed(50)
    m = models.to_mi355x(models.resnet50(num_classes=100), "cuda")
    m.train()
    x = cl(torch.randn(4, 3, 64, 64, device="cuda", dtype=torch.bfloat16))
    y = torch.randint(0, 100, (4,), device="cuda")
    opt = FusedSGD(m.parameters(), lr=0.02, momentum=0.9)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = m.loss(m(x), y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(l == l for l in losses), losses  # no NaN
    assert losses[-1] < losses[0], losses  # memorizing a fixed batch


def test_simple_cnn_train_step_gpu():
    """The mnist example model on the GPU contract (bf16 channels-last):
    one fwd+bwd+step, loss finite."""
    from mpi_operator_amd import models
    from mpi_operator_amd.optim import FusedSGD
    torch.manual_seed(5)
    m = models.to_mi355x(models.SimpleCNN(in_ch=1, num_classes=10), "cuda")
    m.train()
    opt = FusedSGD(m.parameters(), lr=0.01)
    x = torch.randn(8, 1, 28, 28, device="cuda").to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), device="cuda")
    loss = m.loss(m(x), y)
    loss.backward()
    opt.step()
    assert float(loss) == float(loss)


@pytest.mark.parametrize("wd,nesterov", [(0.01, False), (0.01, True), (0.0, True)])
def test_fused_sgd_kernel_wd_nesterov_matches_torch(wd, nesterov):
    """The sgd_step_k wd/nesterov algebra vs torch.optim.SGD on fp32 CUDA
    params (the loss-descent tests only exercise the defaults)."""
    from mpi_operator_amd.optim import FusedSGD
    torch.manual_seed(44)
    a = torch.nn.Linear(64, 32).to("cuda")
    b = torch.nn.Linear(64, 32).to("cuda")
    b.load_state_dict(a.state_dict())
    oa = FusedSGD(a.parameters(), lr=0.1, momentum=0.9, weight_decay=wd,
                  nesterov=nesterov)
    ob = torch.optim.SGD(b.parameters(), lr=0.1, momentum=0.9,
                         weight_decay=wd, nesterov=nesterov)
    x = torch.randn(16, 64, device="cuda")
    for _ in range(5):
        oa.zero_grad(); ob.zero_grad()
        a(x).pow(2).mean().backward()
        b(x).pow(2).mean().backward()
        oa.step(); ob.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-5), (pa - pb).abs().max()
