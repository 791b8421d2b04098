"""Flash attention on MI355X (ops/csrc/flash_attention.hip): tiled
online-softmax forward + recompute-from-lse backward vs the fp32 torch chain
on the bf16-rounded input, for seq up to 512 and padded (key-masked) batches;
lse accuracy, determinism, saved-state size and the BertLayer routing."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, D = 2, 3, 64
SCALE = 0.125
FMIN = torch.finfo(torch.float32).min


def _key_mask(S, valid):
    mask = torch.zeros(len(valid), S, device="cuda")
    for b, n in enumerate(valid):
        mask[b, n:] = FMIN
    return mask


@functools.lru_cache(maxsize=None)
def _case(S, masked):
    """Inputs and the fp32 reference (out, dqkv, lse) for one shape; computed
    once and shared — callers must not modify the tensors."""
    g = torch.Generator(device="cuda").manual_seed(1000 + S)
    qkv = (torch.randn(B, S, 3, H, D, device="cuda", generator=g) * 0.5
           ).to(torch.bfloat16)
    gout = torch.randn(B, S, H * D, device="cuda", generator=g
                       ).to(torch.bfloat16)
    mask = _key_mask(S, [S, S - 37]) if masked else None
    r = qkv.float().requires_grad_()
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if mask is not None:
        s = s + mask[:, None, None, :]
    p = torch.softmax(s, dim=-1)
    out = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D)
    out.backward(gout.float())
    lse = torch.logsumexp(s.detach(), dim=-1)
    return qkv, gout, mask, out.detach(), r.grad.detach(), lse


def _run(S, masked):
    from mpi_operator_amd.ops import functional as Fx
    qkv, gout, mask, out_r, grad_r, _ = _case(S, masked)
    a = qkv.clone().requires_grad_()
    out = Fx.flash_attention(a, H, SCALE, mask)
    out.backward(gout)
    torch.cuda.synchronize()
    assert out.shape == (B, S, H * D) and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    assert torch.isfinite(a.grad.float()).all()
    ferr = (out.float() - out_r).abs().max().item()
    gerr = (a.grad.float() - grad_r).abs().max().item()
    gmax = grad_r.abs().max().item()
    print(f"S={S} masked={masked}: fwd err {ferr:.3e}, grad err {gerr:.3e} "
          f"(max |ref grad| {gmax:.3e})")
    assert ferr < 0.02, ferr
    assert gerr < 0.08 * gmax + 2e-3, (gerr, gmax)
    return a.grad


@pytest.mark.parametrize("S", [129, 296, 512])
def test_flash_attention_unmasked(S):
    """129: second q-chunk / key tile hold one row; 296 = 2·128 + 40 (tail
    not a multiple of 32 or 16); 512: four full tiles (max_seq)."""
    _run(S, False)


@pytest.mark.parametrize("S", [72, 320])
def test_flash_attention_key_mask(S):
    """Valid lengths [S, S−37]; masked keys take finfo.min. Their dK and dV
    rows must be exactly zero (P is exactly 0 there)."""
    grad = _run(S, True)
    assert (grad[1, S - 37:, 1:] == 0).all()
    assert (grad[0, :, 1:] != 0).any()


def test_flash_lse_matches_logsumexp():
    """lse from the kernel vs fp32 torch.logsumexp at S=296, masked.
    Measured max abs error on MI355X: 9.537e-07 (2 ulp at lse ≈ 5.7);
    asserted 10× that, which is below the 1e-3 ceiling (a score of ~0.5
    rounded to bf16 is off by ~1e-3 — the bug this guards against; fp32
    accumulation over 64 products ~1e-5)."""
    from mpi_operator_amd.ops import hip_ext
    qkv, _, mask, _, _, lse_r = _case(296, True)
    ctx, lse = hip_ext().flash_attn_fwd(qkv, H, SCALE, mask)
    assert lse.shape == (B, H, 296) and lse.dtype == torch.float32
    err = (lse - lse_r).abs().max().item()
    print(f"lse max abs err {err:.3e}")
    assert err < min(10 * LSE_MEASURED, 1e-3), err


LSE_MEASURED = 9.537e-07


def test_flash_backward_deterministic():
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    qkv, gout, mask, _, _, _ = _case(296, True)
    ctx, lse = ext.flash_attn_fwd(qkv, H, SCALE, mask)
    d1 = ext.flash_attn_bwd(qkv, ctx, gout, lse, SCALE, mask)
    d2 = ext.flash_attn_bwd(qkv, ctx, gout, lse, SCALE, mask)
    assert torch.equal(d1, d2)


def test_flash_saved_state_is_linear_in_seq():
    """Autograd keeps out + lse (+ qkv, which already exists): no
    [B,H,S,S] tensor. A [2,2,512,512] bf16 probs alone would be 2 MiB."""
    from mpi_operator_amd.ops import functional as Fx
    Bs, Hs, S = 2, 2, 512
    qkv = (torch.randn(Bs, S, 3, Hs, D, device="cuda") * 0.5
           ).to(torch.bfloat16).requires_grad_()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = Fx.flash_attention(qkv, Hs, SCALE)
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated() - before
    out_bytes = out.numel() * out.element_size()
    lse_bytes = Bs * Hs * S * 4
    print(f"saved-state bytes {used} (out {out_bytes}, lse {lse_bytes})")
    assert used < out_bytes + lse_bytes + 64 * 1024, used


def _small_layer():
    from mpi_operator_amd.models.bert import (BertConfig, BertLayer,
                                              BertLinear, LayerNorm)
    torch.manual_seed(11)
    cfg = BertConfig(hidden=128, layers=1, heads=2, intermediate=256)
    layer = BertLayer(cfg).to(device="cuda", dtype=torch.bfloat16)
    for mod in layer.modules():
        if isinstance(mod, LayerNorm):
            mod.weight.data = mod.weight.data.float()
            mod.bias.data = mod.bias.data.float()
        elif isinstance(mod, BertLinear):
            mod.bias.data = mod.bias.data.float()
    return layer


@pytest.mark.parametrize("shape,pad", [((2, 80, 128), 16), ((1, 320, 128), 0)])
def test_bert_layer_routes_to_flash_attention(shape, pad, monkeypatch):
    """MPIAMD_FLASH_ATTN=1 sends the (b,1,1,s) key-masked / s > 256 layer
    through Fx.flash_attention exactly once; =0 keeps the eager chain; both
    agree on the output and every gradient."""
    from mpi_operator_amd.ops import functional as Fx
    layer = _small_layer()
    b, s, _ = shape
    x = ((torch.rand(*shape, device="cuda") * 2 - 1) * 0.5).to(torch.bfloat16)
    cot = torch.randn(*shape, device="cuda")
    mask = None
    if pad:
        keep = torch.ones(b, s, device="cuda")
        keep[1, s - pad:] = 0
        mask = (1.0 - keep[:, None, None, :].float()) * FMIN

    calls = []
    real = Fx.flash_attention

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(Fx, "flash_attention", counting)

    def run(flag):
        monkeypatch.setenv("MPIAMD_FLASH_ATTN", flag)
        del calls[:]
        for p in layer.parameters():
            p.grad = None
        xc = x.clone().requires_grad_()
        y = layer(xc, mask)
        # a fixed random cotangent: y ends in a unit-gain LayerNorm, so
        # mean(y²) is constant and its gradient is pure rounding noise
        (y.float() * cot).sum().backward()
        grads = {n: p.grad.detach().float().clone()
                 for n, p in layer.named_parameters()}
        return (y.detach().float(), xc.grad.detach().float().clone(), grads,
                len(calls))

    # monkeypatch restores the variable (and Fx.flash_attention) on teardown
    y1, dx1, g1, n1 = run("1")
    y0, dx0, g0, n0 = run("0")
    assert n1 == 1 and n0 == 0, (n1, n0)

    def rel(a, r):
        return (a - r).norm().item() / (r.norm().item() + 1e-30)

    assert rel(y1, y0) < 0.02, rel(y1, y0)
    assert rel(dx1, dx0) < 0.02, rel(dx1, dx0)
    for n in g0:
        assert rel(g1[n], g0[n]) < 0.02, (n, rel(g1[n], g0[n]))
