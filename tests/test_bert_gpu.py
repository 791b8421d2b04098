"""BERT on MI355X: HIP NT-GEMM linear path numerics vs fp32 torch reference,
odd/ragged GEMM shapes through the mixed-staging kernels, and a full
BERT-base train step (loss finite & decreasing)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = a.float(), b.float()
    return (a - b).norm().item() / (b.norm().item() + 1e-12)


def test_bert_linear_gpu_matches_fp32():
    from mpi_operator_amd.models.bert import BertLinear
    torch.manual_seed(0)
    lin = BertLinear(1024, 4096).to("cuda", torch.bfloat16)
    x = (torch.rand(4, 128, 1024, device="cuda") * 2 - 1).to(torch.bfloat16)
    y = lin(x)
    yr = torch.nn.functional.linear(x.float(), lin.weight.float(), lin.bias.float())
    assert relerr(y, yr) < 0.02


@pytest.mark.parametrize("M,N,K", [(512, 1000, 2048), (96, 24, 40), (256, 3072, 768),
                                   (8192, 256, 512),  # split-K dw (16 slabs)
                                   (4096, 1024, 1024),  # attn-out shape (8 slabs)
                                   # out_features not %8 (zero-padded dy in
                                   # linear_bwd, ragged TN column granules):
                                   (32, 2, 768),    # NSP head
                                   (64, 10, 64),    # SimpleCNN classifier
                                   (96, 30, 40)])   # the vocab-30522 class
def test_linear_bwd_ragged_shapes(M, N, K):
    """dx/dw via the TN-staged kernels on shapes incl. non-%128, non-%8,
    and linear_fwd at the same shapes."""
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    torch.manual_seed(1)
    x = ((torch.rand(M, K, device="cuda") * 2 - 1)).to(torch.bfloat16)
    w = ((torch.rand(N, K, device="cuda") * 2 - 1) * 0.05).to(torch.bfloat16)
    dy = ((torch.rand(M, N, device="cuda") * 2 - 1)).to(torch.bfloat16)
    b = torch.randn(N, device="cuda")
    y = ext.linear_fwd(x, w, b)
    assert relerr(y, x.float() @ w.float().t() + b) < 0.02
    dx, dw, db = ext.linear_bwd(dy, x, w)
    assert relerr(dx, dy.float() @ w.float()) < 0.02
    assert relerr(dw, dy.float().t() @ x.float()) < 0.02
    assert relerr(db, dy.float().sum(0)) < 0.01


def test_bert_base_train_step_gpu():
    from mpi_operator_amd.models.bert import bert_base, to_mi355x_bert
    from mpi_operator_amd.optim import FusedSGD
    torch.manual_seed(2)
    m = to_mi355x_bert(bert_base(), "cuda")
    m.train()
    opt = FusedSGD(m.parameters(), lr=5e-3, momentum=0.9)
    ids = torch.randint(0, m.cfg.vocab_size, (2, 64), device="cuda")
    mlm_labels = ids.clone()
    nsp = torch.randint(0, 2, (2,), device="cuda")
    losses = []
    for _ in range(8):
        opt.zero_grad()
        mlm_logits, nsp_logits = m(ids)
        loss = m.loss(mlm_logits, nsp_logits, mlm_labels, nsp)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(l == l for l in losses), losses  # no NaN
    assert losses[-1] < losses[0], losses


def test_mlm_head_loss_matches_composed_path():
    """Fused decoder+CE head (padded-vocab buffer) vs the logits+loss
    composition: same loss and same input/weight/bias grads."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(7)
    M, K, V = 256, 768, 30522  # ragged vocab exercises the pad contract
    h = ((torch.rand(M, K, device="cuda") * 2 - 1) * 0.5).to(torch.bfloat16)
    w = ((torch.rand(V, K, device="cuda") * 2 - 1) * 0.05).to(torch.bfloat16)
    b = torch.randn(V, device="cuda") * 0.01
    tgt = torch.randint(0, V, (M,), device="cuda")
    tgt[::3] = -100  # masked-out rows

    h1 = h.clone().requires_grad_()
    w1 = w.clone().requires_grad_()
    b1 = b.clone().requires_grad_()
    loss1 = Fx.mlm_head_loss(h1, w1, b1, tgt)
    loss1.backward()

    h2 = h.clone().requires_grad_()
    w2 = w.clone().requires_grad_()
    b2 = b.clone().requires_grad_()
    logits = Fx.linear(h2, w2, b2)
    loss2 = Fx.masked_softmax_cross_entropy(logits, tgt)
    loss2.backward()

    assert abs(loss1.item() - loss2.item()) < 2e-3 * abs(loss2.item()) + 1e-4
    for a, c in ((h1.grad, h2.grad), (w1.grad, w2.grad), (b1.grad, b2.grad)):
        num = (a.float() - c.float()).norm().item()
        den = c.float().norm().item() + 1e-30
        assert num / den < 0.02, (num / den, a.shape)


@pytest.mark.parametrize("M,N", [(4096, 1024), (100, 768), (7, 2048),
                                 # odd M at N <= 1024: the last row pair of the
                                 # 2-row dx kernel (MPIAMD_LN2) has no partner
                                 (5, 1024)])
def test_layernorm_fwd_bwd_matches_fp32(M, N):
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(3)
    x = ((torch.rand(M, N, device="cuda") * 2 - 1) * 3).to(torch.bfloat16)
    g = torch.rand(N, device="cuda") + 0.5
    b = torch.randn(N, device="cuda") * 0.2
    x1 = x.clone().requires_grad_(True)
    y = Fx.layer_norm(x1, g.clone().requires_grad_(False), b, 1e-12)
    xr = x.float().clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (N,), gr, br, 1e-12)
    assert relerr(y, yr) < 0.02
    dy = ((torch.rand(M, N, device="cuda") * 2 - 1)).to(torch.bfloat16)
    # grads through our Fn (need g/b as leaf tensors for grad check)
    g2 = g.clone().requires_grad_(True)
    b2 = b.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    y2 = Fx.layer_norm(x2, g2, b2, 1e-12)
    y2.backward(dy)
    yr.backward(dy.float())
    assert relerr(x2.grad, xr.grad) < 0.03
    assert relerr(g2.grad, gr.grad) < 0.02
    assert relerr(b2.grad, br.grad) < 0.02


def test_masked_xent_matches_fp32_reference():
    """Fused MLM CE (ignore_index, mean over valid) vs the fp32 oracle,
    forward loss and backward dlogits, at a vocab-scale ragged V."""
    from mpi_operator_amd.ops import functional as Fx
    from mpi_operator_amd.ops import reference as ref
    torch.manual_seed(3)
    B, V = 96, 30522
    logits = (torch.randn(B, V, device="cuda") * 2).to(torch.bfloat16)
    target = torch.randint(0, V, (B,), device="cuda")
    target[::3] = -100  # a third ignored
    lg = logits.clone().requires_grad_(True)
    loss = Fx.masked_softmax_cross_entropy(lg, target)
    loss.backward()
    lf = logits.float().clone().requires_grad_(True)
    ref_loss = torch.nn.functional.cross_entropy(lf, target, ignore_index=-100)
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item()) + 1e-3
    err = (lg.grad.float() - lf.grad).abs().max().item()
    scale = lf.grad.abs().max().item()
    assert err < 0.05 * scale + 1e-6, (err, scale)


@pytest.mark.parametrize("V", [1001, 1002])
def test_masked_xent_small_ragged_vocab(V):
    """Rows 0-3 start at four different 16-byte phases (row pitch 2002 or
    2004 bytes), so the scalar head takes both even and odd lengths, and
    most of the 256 threads own no vector octet. Targets hit the first
    column (in the head or the first octet) and the last (in the tail).
    Bounds of test_masked_xent_matches_fp32_reference."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(4)
    B = 8
    logits = (torch.randn(B, V, device="cuda") * 2).to(torch.bfloat16)
    target = torch.randint(0, V, (B,), device="cuda")
    target[0], target[1], target[2] = 0, V - 1, -100
    lg = logits.clone().requires_grad_(True)
    loss = Fx.masked_softmax_cross_entropy(lg, target)
    loss.backward()
    lf = logits.float().clone().requires_grad_(True)
    ref_loss = torch.nn.functional.cross_entropy(lf, target, ignore_index=-100)
    ref_loss.backward()
    print("loss", loss.item(), "ref", ref_loss.item())
    assert abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item()) + 1e-3
    err = (lg.grad.float() - lf.grad).abs().max().item()
    scale = lf.grad.abs().max().item()
    print("dlogits err", err, "scale", scale)
    assert err < 0.05 * scale + 1e-6, (err, scale)
    assert lg.grad[2].abs().max().item() == 0.0  # the ignored row


def test_masked_xent_all_ignored_rows():
    from mpi_operator_amd.ops import functional as Fx
    B, V = 8, 512
    logits = torch.randn(B, V, device="cuda").to(torch.bfloat16).requires_grad_(True)
    target = torch.full((B,), -100, device="cuda", dtype=torch.long)
    loss = Fx.masked_softmax_cross_entropy(logits, target)
    assert loss.item() == 0.0
    loss.backward()
    assert logits.grad.abs().max().item() == 0.0


def test_bert_mlm_head_on_hip_path_matches_torch():
    """The rerouted MLM decoder (Fx.linear + fused CE) against the plain
    torch head computation, fwd loss + grads into h and tok weights."""
    from mpi_operator_amd.models.bert import bert_base, to_mi355x_bert
    torch.manual_seed(5)
    m = to_mi355x_bert(bert_base(), "cuda")
    ids = torch.randint(0, m.cfg.vocab_size, (2, 32), device="cuda")
    labels = ids.clone()
    labels[:, ::2] = -100
    nsp = torch.randint(0, 2, (2,), device="cuda")
    mlm_logits, nsp_logits = m(ids)
    loss = m.loss(mlm_logits, nsp_logits, labels, nsp)
    loss.backward()
    g_hip = m.bert.embeddings.tok.weight.grad.clone()
    m.zero_grad(set_to_none=True)

    # plain-torch head on the same trunk output
    x = m.bert(ids)
    h = torch.nn.functional.gelu(m.mlm_transform(x), approximate="tanh")
    h = m.mlm_ln(h)
    logits_t = torch.matmul(h, m.bert.embeddings.tok.weight.t()) + m.mlm_bias
    l_t = torch.nn.functional.cross_entropy(
        logits_t.float().view(-1, m.cfg.vocab_size), labels.view(-1),
        ignore_index=-100)
    l_nsp = torch.nn.functional.cross_entropy(m.nsp(x[:, 0]).float(), nsp)
    (l_t + l_nsp).backward()
    g_t = m.bert.embeddings.tok.weight.grad
    assert abs(loss.item() - (l_t + l_nsp).item()) < 0.05 * abs((l_t + l_nsp).item()) + 5e-2
    num = (g_hip.float() - g_t.float()).abs().max().item()
    den = g_t.float().abs().max().item() + 1e-6
    assert num < 0.1 * den + 1e-4, (num, den)


def test_ffn_fused_gelu_matches_fp32():
    """Fused FFN (GELU in GEMM epilogues) vs a plain fp32 torch FFN:
    forward output and all five gradients."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(7)
    M, H, I = 512, 256, 1024
    x = (torch.randn(M, H, device="cuda") * 0.5).to(torch.bfloat16)
    w1 = (torch.randn(I, H, device="cuda") * 0.05).to(torch.bfloat16)
    b1 = torch.randn(I, device="cuda").to(torch.bfloat16) * 0.1
    w2 = (torch.randn(H, I, device="cuda") * 0.05).to(torch.bfloat16)
    b2 = torch.randn(H, device="cuda").to(torch.bfloat16) * 0.1
    args = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = Fx.ffn(*args)
    y.float().square().mean().backward()

    ref = [t.float().clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    h = torch.nn.functional.linear(ref[0], ref[1], ref[2])
    g = torch.nn.functional.gelu(h, approximate="tanh")
    yr = torch.nn.functional.linear(g, ref[3], ref[4])
    yr.square().mean().backward()

    assert torch.allclose(y.float(), yr, rtol=0.05, atol=0.05), \
        (y.float() - yr).abs().max()
    for a, r, name in zip(args, ref, "x w1 b1 w2 b2".split()):
        num = (a.grad.float() - r.grad).abs().max().item()
        den = r.grad.abs().max().item() + 1e-6
        assert num < 0.08 * den + 1e-4, (name, num, den)


def test_fused_attention_matches_torch():
    """Fused MHA fwd + hybrid bwd vs the plain torch chain (fp32 math)."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(11)
    B, S, H, D = 4, 128, 8, 64
    qkv = (torch.randn(B, S, 3, H, D, device="cuda") * 0.5).to(torch.bfloat16)
    a = qkv.clone().requires_grad_(True)
    out = Fx.attention(a, H, 1.0 / D ** 0.5)
    out.float().square().mean().backward()

    r = qkv.float().clone().requires_grad_(True)
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    scores = torch.matmul(q, k.transpose(-1, -2)) / D ** 0.5
    p = torch.softmax(scores, dim=-1)
    ctx_t = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D)
    ctx_t.square().mean().backward()

    fwd_err = (out.float() - ctx_t).abs().max().item()
    assert fwd_err < 0.02, fwd_err
    g_err = (a.grad.float() - r.grad).abs().max().item()
    g_scale = r.grad.abs().max().item() + 1e-6
    assert g_err < 0.08 * g_scale + 1e-4, (g_err, g_scale)


@pytest.mark.parametrize("S", [160, 256])
def test_fused_attention_seq_over_128(S):
    """S in (128, 256]: the 256-capacity template runs TWO 128-row
    q-chunks per (b, h) — the first cut left rows 128+ uninitialized
    (NaN at seq 256, caught by an end-to-end edge sweep)."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(19)
    B, H, D = 2, 4, 64
    qkv = (torch.randn(B, S, 3, H, D, device="cuda") * 0.5).to(torch.bfloat16)
    a = qkv.clone().requires_grad_(True)
    out = Fx.attention(a, H, 1.0 / D ** 0.5)
    out.float().square().mean().backward()
    r = qkv.float().clone().requires_grad_(True)
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / D ** 0.5, dim=-1)
    ref = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D)
    ref.square().mean().backward()
    assert (out.float() - ref).abs().max().item() < 0.02
    g_err = (a.grad.float() - r.grad).abs().max().item()
    g_scale = r.grad.abs().max().item() + 1e-6
    assert g_err < 0.08 * g_scale + 1e-4, (g_err, g_scale)


def test_fused_attention_ragged_seq():
    """S not a multiple of 32: padded key columns must not leak."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(13)
    B, S, H, D = 2, 72, 4, 64
    qkv = (torch.randn(B, S, 3, H, D, device="cuda") * 0.5).to(torch.bfloat16)
    out = Fx.attention(qkv, H, 0.125)
    r = qkv.float()
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * 0.125, dim=-1)
    ref = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D)
    assert (out.float() - ref).abs().max().item() < 0.02


def test_layer_norm_add_matches_fp32():
    """Fused residual+LN vs torch fp32, fwd + grads to both addends."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(17)
    M, N = 384, 1024
    a = (torch.randn(M, N, device="cuda") * 0.7).to(torch.bfloat16)
    b = (torch.randn(M, N, device="cuda") * 0.7).to(torch.bfloat16)
    w = torch.rand(N, device="cuda") + 0.5
    bb = torch.randn(N, device="cuda") * 0.1
    aa, ab = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    wa, wb = w.clone().requires_grad_(True), bb.clone().requires_grad_(True)
    y = Fx.layer_norm_add(aa, ab, wa, wb, 1e-12)
    y.float().square().mean().backward()

    # reference computes on the bf16-rounded sum (what the kernel stats see)
    ra = (a.float() + b.float()).to(torch.bfloat16).float().requires_grad_(True)
    rw = w.clone().requires_grad_(True)
    rb = bb.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(ra, (N,), rw, rb, 1e-12)
    yr.square().mean().backward()

    assert (y.float() - yr).abs().max().item() < 0.02
    for g, r, name in ((aa.grad, ra.grad, "da"), (ab.grad, ra.grad, "db"),
                       (wa.grad, rw.grad, "dw"), (wb.grad, rb.grad, "dbias")):
        num = (g.float() - r).abs().max().item()
        den = r.abs().max().item() + 1e-6
        assert num < 0.08 * den + 1e-4, (name, num, den)


def test_ffn_fused_gelu_pipe256_route():
    """Shape that routes fc1 through the 256²-tile writer kernel
    (M%256==0, I%256==0, nwg>=128): numerics vs fp32 torch."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(19)
    M, H, I = 4096, 256, 4096
    x = (torch.randn(M, H, device="cuda") * 0.5).to(torch.bfloat16)
    w1 = (torch.randn(I, H, device="cuda") * 0.05).to(torch.bfloat16)
    b1 = torch.randn(I, device="cuda").to(torch.bfloat16) * 0.1
    w2 = (torch.randn(H, I, device="cuda") * 0.05).to(torch.bfloat16)
    b2 = torch.randn(H, device="cuda").to(torch.bfloat16) * 0.1
    y = Fx.ffn(x, w1, b1, w2, b2)
    h = torch.nn.functional.linear(x.float(), w1.float(), b1.float())
    g = torch.nn.functional.gelu(h, approximate="tanh")
    yr = torch.nn.functional.linear(g, w2.float(), b2.float())
    assert torch.allclose(y.float(), yr, rtol=0.05, atol=0.05), \
        (y.float() - yr).abs().max()


def test_ffn_fused_gelu_pipe256_route_bwd():
    """Backward at the 256²-route FFN shape: the fc2-dx GEMM with the gelu'
    epilogue runs at M=4096, N=4096, K=256 — the TN pipe by default, the
    transpose-plus-pipe256 route under MPIAMD_GELUBWD_WT=1, and the
    recompute-tanh writers under MPIAMD_GELU_DERIV=0.

    First the GEMM alone: linear_gelu_dgrad against fp32 (dy·w2) ⊙ gelu'(h),
    max error over max |reference| with NO absolute floor. Budget: the bf16
    store of dh is 2^-8 relative (bf16 unit roundoff); the saved operand is
    bf16 too — gelu'(h) itself (another 2^-8 relative) or, under
    GELU_DERIV=0, h with |δh| <= 2^-8·|h| and |gelu''| <= 1.13, i.e.
    |δgelu'| <= 0.005 where |h| <= 1 and less beyond, where gelu'' decays;
    the fp32 accumulation over K=256 is negligible. Together under
    2·2^-8 + 0.001 = 0.009 of the scale; the bound is 0.02.
    One output tile left unwritten, a dropped k-tile or a transposed w2
    moves the error to the order of the scale itself.

    Then all five FFN gradients against the fp32 torch FFN under a
    sum-of-squares loss, so that they are O(1) and the bound is purely
    relative (0.08 of the max, as in test_ffn_fused_gelu_matches_fp32)."""
    from mpi_operator_amd.ops import functional as Fx
    from mpi_operator_amd.ops import hip_ext
    from mpi_operator_amd.ops import reference as ref_ops
    ext = hip_ext()
    torch.manual_seed(19)
    M, H, I = 4096, 256, 4096
    x = (torch.randn(M, H, device="cuda") * 0.5).to(torch.bfloat16)
    w1 = (torch.randn(I, H, device="cuda") * 0.05).to(torch.bfloat16)
    b1 = torch.randn(I, device="cuda").to(torch.bfloat16) * 0.1
    w2 = (torch.randn(H, I, device="cuda") * 0.05).to(torch.bfloat16)
    b2 = torch.randn(H, device="cuda").to(torch.bfloat16) * 0.1
    dy = (torch.rand(M, H, device="cuda") * 2 - 1).to(torch.bfloat16)

    _, aux = ext.linear_gelu_fwd(x, w1, b1)
    dh = ext.linear_gelu_dgrad(dy, w2, aux)
    h_ref = x.float() @ w1.float().t() + b1.float()
    dh_ref = (dy.float() @ w2.float()) * ref_ops.dgelu(h_ref)
    err = (dh.float() - dh_ref).abs().max().item()
    scale = dh_ref.abs().max().item()
    print("fc2-dx err", err, "scale", scale)
    assert err < 0.02 * scale, (err, scale)

    args = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = Fx.ffn(*args)
    y.float().square().sum().backward()

    ref = [t.float().clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    h = torch.nn.functional.linear(ref[0], ref[1], ref[2])
    g = torch.nn.functional.gelu(h, approximate="tanh")
    yr = torch.nn.functional.linear(g, ref[3], ref[4])
    yr.square().sum().backward()

    assert torch.allclose(y.float(), yr, rtol=0.05, atol=0.05), \
        (y.float() - yr).abs().max()
    for a, r, name in zip(args, ref, "x w1 b1 w2 b2".split()):
        num = (a.grad.float() - r.grad).abs().max().item()
        den = r.grad.abs().max().item()
        print(name, "grad err", num, "scale", den)
        assert num < 0.08 * den, (name, num, den)


def test_fused_attention_backward_matches_torch():
    """The fused S=128 attention backward vs the fp32 torch chain."""
    from mpi_operator_amd.ops import functional as Fx
    torch.manual_seed(23)
    B, S, H, D = 3, 128, 4, 64
    qkv = (torch.randn(B, S, 3, H, D, device="cuda") * 0.5).to(torch.bfloat16)
    a = qkv.clone().requires_grad_(True)
    out = Fx.attention(a, H, 1.0 / D ** 0.5)
    gout = torch.randn_like(out)
    out.backward(gout)

    r = qkv.float().clone().requires_grad_(True)
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / D ** 0.5, dim=-1)
    ctx_t = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D)
    ctx_t.backward(gout.float())

    err = (a.grad.float() - r.grad).abs().max().item()
    scale = r.grad.abs().max().item() + 1e-6
    assert err < 0.08 * scale + 2e-3, (err, scale)


def test_composite_layer_matches_decomposed():
    """BertLayerFn (whole-layer composite with accumulate-dgrad joins) vs
    the per-op Fn path: same output and same grads for every param."""
    import os
    from mpi_operator_amd.models.bert import BertConfig, BertLayer, LayerNorm, BertLinear
    torch.manual_seed(11)
    cfg = BertConfig(hidden=512, layers=1, heads=8, intermediate=2048)
    layer = BertLayer(cfg).to(device="cuda", dtype=torch.bfloat16)
    for mod in layer.modules():
        if isinstance(mod, LayerNorm):
            mod.weight.data = mod.weight.data.float()
            mod.bias.data = mod.bias.data.float()
        elif isinstance(mod, BertLinear):
            mod.bias.data = mod.bias.data.float()
    x = ((torch.rand(2, 128, 512, device="cuda") * 2 - 1) * 0.5).to(torch.bfloat16)

    def run(fused):
        os.environ["MPIAMD_LAYER_FUSED"] = "1" if fused else "0"
        for p in layer.parameters():
            p.grad = None
        xc = x.clone().requires_grad_()
        y = layer(xc)
        y.float().square().mean().backward()
        grads = {n: p.grad.detach().float().clone()
                 for n, p in layer.named_parameters()}
        return y.detach().float(), xc.grad.detach().float().clone(), grads

    y1, dx1, g1 = run(True)
    y0, dx0, g0 = run(False)
    os.environ.pop("MPIAMD_LAYER_FUSED", None)
    assert (y1 - y0).abs().max().item() < 1e-5, "composite fwd differs"
    rel = (dx1 - dx0).norm().item() / (dx0.norm().item() + 1e-30)
    assert rel < 0.02, f"dx mismatch {rel}"
    for n in g0:
        num = (g1[n] - g0[n]).norm().item()
        den = g0[n].norm().item() + 1e-30
        assert num / den < 0.02, (n, num / den)


def test_bert_forward_with_attention_mask():
    """attn_mask falls back to the eager attention path — guard the shape
    plumbing end-to-end (the fused kernel path requires mask is None)."""
    from mpi_operator_amd.models.bert import bert_base, to_mi355x_bert
    torch.manual_seed(23)
    m = to_mi355x_bert(bert_base(), "cuda")
    ids = torch.randint(0, m.cfg.vocab_size, (2, 48), device="cuda")
    mask = torch.ones(2, 48, device="cuda")
    mask[:, 40:] = 0  # padded tail
    mlm_logits, nsp_logits = m(ids, attn_mask=mask)
    assert torch.isfinite(mlm_logits.float()).all()
    assert torch.isfinite(nsp_logits.float()).all()
