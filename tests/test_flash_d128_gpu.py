"""Flash attention at head_dim 128 on MI355X (ops/csrc/flash_attention_d128.hip)
against an fp64 torch chain on the bf16-rounded input: dense, causal, key
mask, packed, and the BERT route."""
import pytest
import torch

import attn_dropout_refs as ar
from mpi_operator_amd.models.bert import (BertConfig, BertForPreTraining,
                                          to_mi355x_bert)
from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import hip_ext
from test_flash_attention_gpu import LSE_MEASURED

pytestmark = pytest.mark.gpu

B, H, D, SCALE, DEV = 2, 3, 128, 128 ** -0.5, "cuda"


def _inputs(b, S):
    """attn_dropout_refs.inputs (same seeds and scaling) with D = 128."""
    g = torch.Generator().manual_seed(1000 + S)
    qkv = (torch.randn(b, S, 3, H, D, generator=g) * 0.5).to(torch.bfloat16)
    gout = torch.randn(b, S, H * D, generator=g).to(torch.bfloat16)
    return qkv.to(DEV), gout.to(DEV)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("S,masked", [(128, 0), (129, 0), (296, 0), (296, 1)])
def test_against_fp64(S, masked, causal):
    """128: one tile (causal: a diagonal alone); 129: a second tile / chunk
    with one live row and the 64-key dK/dV chunk edge 128 -> 192; 296 =
    2·128 + 40: past tiles and a ragged diagonal. Measured fwd / grad error,
    dense (max |ref grad| 0.25-0.43) then causal (3.9-4.1): S=128 6.5e-4 /
    1.4e-3, 3.0e-3 / 1.1e-2; S=129 6.4e-4 / 1.3e-3, 2.6e-3 / 1.0e-2; S=296
    3.7e-4 / 8.5e-4, 4.4e-3 / 1.2e-2; S=296 masked 3.7e-4 / 1.1e-3, 4.4e-3 /
    1.1e-2; lse 8.5e-7 to 8.8e-7. S = 296 also checks lse and that the
    backward repeats."""
    qkv, gout = _inputs(B, S)
    mask = ar.key_mask(S, [S, S - 37], DEV) if masked else None
    r = qkv.double().requires_grad_()
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if masked:
        s = s + mask[:, None, None, :].double()
    if causal:
        s = s.masked_fill(
            torch.ones(S, S, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    out_r = torch.matmul(torch.softmax(s, dim=-1), v)
    out_r = out_r.transpose(1, 2).reshape(B, S, H * D)
    out_r.backward(gout.double())
    a = qkv.clone().requires_grad_()
    out = Fx.flash_attention(a, H, SCALE, mask, causal=bool(causal))
    out.backward(gout)
    ferr = (out.double() - out_r).abs().max().item()
    gerr = (a.grad.double() - r.grad).abs().max().item()
    gmax = r.grad.abs().max().item()
    print(f"S={S} masked={masked} causal={causal}: fwd err {ferr:.3e}, grad "
          f"err {gerr:.3e} (max |ref grad| {gmax:.3e})")
    assert ferr < 0.02, ferr
    assert gerr < 0.08 * gmax + 2e-3, (gerr, gmax)
    if S == 296:
        ctx, lse = hip_ext().flash_attn_fwd(qkv, H, SCALE, mask, bool(causal))
        err = (lse.double() - torch.logsumexp(s, -1)).abs().max().item()
        print(f"lse (masked={masked} causal={causal}) max abs err {err:.3e}")
        assert err < min(10 * LSE_MEASURED, 1e-3), err
        bwd = hip_ext().flash_attn_bwd
        d1 = bwd(qkv, ctx, gout, lse, SCALE, mask, bool(causal))
        d2 = bwd(qkv, ctx, gout, lse, SCALE, mask, bool(causal))
        assert torch.equal(d1, d2) and torch.equal(d1, a.grad)


@pytest.mark.parametrize("j", [1, 64, 128, 200])
def test_no_look_ahead_bit_for_bit(j):
    """j = 64 is the dK/dV key-chunk boundary, 128 the tile boundary."""
    qkv = _inputs(B, 296)[0]
    other = torch.cat([qkv[:, :j], _inputs(B, 297)[0][:, j:296]], 1)
    c0, l0 = hip_ext().flash_attn_fwd(qkv, H, SCALE, None, True)
    c1, l1 = hip_ext().flash_attn_fwd(other, H, SCALE, None, True)
    assert torch.equal(c0[:, :j], c1[:, :j]) and torch.equal(l0[..., :j], l1[..., :j])


@pytest.mark.parametrize("causal", [False, True])
def test_packed_equals_dense(causal):
    """Lengths [129, 0, 40, 200] in T = 400 against the dense call on each
    sequence alone; the rows past 369 are zero."""
    ext = hip_ext()
    qkv, gout = (t[0] for t in _inputs(1, 400))
    cul, ms = [0, 129, 129, 169, 369], 200
    cu = torch.tensor(cul, dtype=torch.int32, device=DEV)
    x = qkv.clone().requires_grad_()
    ctx = Fx.flash_attention_varlen(x, cu, ms, H, SCALE, causal=causal)
    ctx.backward(gout)
    lse = ext.flash_attn_varlen_fwd(qkv, cu, ms, H, SCALE, causal)[1]
    for n, (a, e) in enumerate(zip(cul, cul[1:])):
        if e == a:
            continue
        q1 = qkv[a:e][None].clone().requires_grad_()
        c1 = Fx.flash_attention(q1, H, SCALE, None, causal=causal)
        c1.backward(gout[a:e][None])
        l1 = ext.flash_attn_fwd(q1.detach(), H, SCALE, None, causal)[1]
        assert torch.equal(ctx[a:e], c1[0]), n
        assert torch.equal(lse[:, a:e], l1[0]), n
        assert torch.equal(x.grad[a:e], q1.grad[0]), n
    assert not (ctx[369:].any() or lse[:, 369:].any() or x.grad[369:].any())


@pytest.mark.parametrize("causal", [False, True])
def test_bert_head_dim_128_routes_to_flash(monkeypatch, causal):
    """Not Fx.attention and not the eager chain (a zero [B,1,S,S] mask selects
    that): within 2 % of it, not equal to it; causal: no look-ahead."""
    torch.manual_seed(5)
    cfg = BertConfig(hidden=256, heads=2, layers=2, intermediate=256,
                     max_seq=128, causal=causal)
    model = to_mi355x_bert(BertForPreTraining(cfg), DEV).bert.eval()
    monkeypatch.setattr(Fx, "attention", None)
    ids = torch.randint(0, 512, (2, 128), device=DEV)
    ids2 = torch.cat([ids[:, :70], (ids[:, 70:] + 1) % 512], 1)
    with torch.no_grad():
        y, y2 = model(ids).float(), model(ids2).float()
        ye = model(ids, attn_mask=torch.zeros(2, 1, 128, 128, device=DEV)).float()
    rel = (y - ye).norm().item() / ye.norm().item()
    print(f"head_dim 128 model (causal={causal}) vs eager chain: rel {rel:.3e}")
    assert 0 < rel < 0.02, rel
    if causal:
        assert torch.equal(y[:, :70], y2[:, :70])


def test_contract():
    qkv = _inputs(B, 128)[0]
    with pytest.raises(ValueError):
        Fx.flash_attention(qkv, H, SCALE, None, 0.1, Fx.DropoutRng(1, DEV))
    with pytest.raises(RuntimeError):
        hip_ext().flash_attn_fwd(qkv[..., :96].contiguous(), H, SCALE, None, False)
