"""Causal flash attention on MI355X (CAUSAL in ops/csrc/flash_attention.hip)
against an fp64 torch chain on the bf16-rounded input."""
import pytest
import torch

import attn_dropout_refs as ar
from mpi_operator_amd.models.bert import (BertConfig, BertForPreTraining,
                                          to_mi355x_bert)
from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import hip_ext
from mpi_operator_amd.ops import reference as ref
from test_flash_attention_gpu import LSE_MEASURED

pytestmark = pytest.mark.gpu

B, H, D, SCALE, DEV = 2, 3, 64, ar.SCALE, "cuda"
SEED, OFFSET, SITE, P = 0x1234_5678_9abc_def1, (3 << 32) + 7, 3, 0.1


def _rng():
    rng = Fx.DropoutRng(SEED, DEV)
    rng.set_state(SEED, OFFSET)
    return rng


@pytest.mark.parametrize("S,masked,p", [(128, 0, 0.0), (129, 0, 0.0),
                                        (296, 0, 0.0), (296, 1, 0.0), (296, 0, P)])
def test_causal_against_fp64(S, masked, p):
    """128: the diagonal tile alone; 129: a diagonal tile with one live row;
    296 = 2·128 + 40: past tiles and a diagonal. Measured fwd / grad error
    (max |ref grad| 3.9-4.3): 2.7e-3 / 1.5e-2, 3.7e-3 / 9.2e-3, 3.2e-3 /
    9.1e-3, masked 3.2e-3 / 8.3e-3, p=0.1 3.5e-3 / 9.4e-3; lse 8.2e-7.
    S = 296 without dropout also checks lse and that the backward repeats."""
    qkv, gout = ar.inputs(B, H, S, DEV)
    mask = ar.key_mask(S, [S, S - 37], DEV) if masked else None
    r = qkv.double().requires_grad_()
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if masked:
        s = s + mask[:, None, None, :].double()
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=DEV).triu(1),
                      float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if p:
        keep = ref.attn_dropout_keep(SEED, OFFSET, SITE, B, H, S, p).to(DEV)
        pr = pr * keep.double() * ref.dropout_threshold(p)[2]
    out_r = torch.matmul(pr, v).transpose(1, 2).reshape(B, S, H * D)
    out_r.backward(gout.double())
    a = qkv.clone().requires_grad_()
    out = Fx.flash_attention(a, H, SCALE, mask, p, _rng(), SITE, causal=True)
    out.backward(gout)
    ferr = (out.double() - out_r).abs().max().item()
    gerr = (a.grad.double() - r.grad).abs().max().item()
    gmax = r.grad.abs().max().item()
    print(f"S={S} masked={masked} p={p}: fwd err {ferr:.3e}, grad err "
          f"{gerr:.3e} (max |ref grad| {gmax:.3e})")
    assert ferr < 0.02, ferr
    assert gerr < 0.08 * gmax + 2e-3, (gerr, gmax)
    if S == 296 and not p:
        ctx, lse = hip_ext().flash_attn_fwd(qkv, H, SCALE, mask, True)
        err = (lse.double() - torch.logsumexp(s, -1)).abs().max().item()
        print(f"causal lse (masked={masked}) max abs err {err:.3e}")
        assert err < min(10 * LSE_MEASURED, 1e-3), err
        d1 = hip_ext().flash_attn_bwd(qkv, ctx, gout, lse, SCALE, mask, True)
        d2 = hip_ext().flash_attn_bwd(qkv, ctx, gout, lse, SCALE, mask, True)
        assert torch.equal(d1, d2) and torch.equal(d1, a.grad)


@pytest.mark.parametrize("j", [1, 100, 128, 200])
def test_no_look_ahead_bit_for_bit(j):
    qkv = ar.inputs(B, H, 296, DEV)[0]
    other = torch.cat([qkv[:, :j], ar.inputs(B, H, 297, DEV)[0][:, j:296]], 1)
    c0, l0 = hip_ext().flash_attn_fwd(qkv, H, SCALE, None, True)
    c1, l1 = hip_ext().flash_attn_fwd(other, H, SCALE, None, True)
    assert torch.equal(c0[:, :j], c1[:, :j]) and torch.equal(l0[..., :j], l1[..., :j])


@pytest.mark.parametrize("p", [0.0, P])
def test_packed_equals_dense_causal(p):
    """Lengths [129, 0, 40, 200] in T = 400 against the dense call on each
    sequence alone (p = 0) or row n of the key-masked [4, 200] batch (p > 0)."""
    ext = hip_ext()
    qkv, gout = (t[0] for t in ar.inputs(1, H, 400, DEV))
    cul, ms = [0, 129, 129, 169, 369], 200
    cu = torch.tensor(cul, dtype=torch.int32, device=DEV)
    drop = (_rng().state, p, SITE) if p else ()
    x = qkv.clone().requires_grad_()
    ctx = Fx.flash_attention_varlen(x, cu, ms, H, SCALE, p, _rng(), SITE, True)
    ctx.backward(gout)
    vfwd = ext.flash_attn_varlen_drop_fwd if p else ext.flash_attn_varlen_fwd
    lse = vfwd(qkv, cu, ms, H, SCALE, *drop, True)[1]

    def dense(q, cot, mask):
        q = q.clone().requires_grad_()
        c = Fx.flash_attention(q, H, SCALE, mask, p, _rng(), SITE, causal=True)
        c.backward(cot)
        fwd = ext.flash_attn_drop_fwd if p else ext.flash_attn_fwd
        return c, fwd(q.detach(), H, SCALE, mask, *drop, True)[1], q.grad

    if p:  # the padded batch, once
        qd = torch.zeros(4, ms, 3, H, D, dtype=torch.bfloat16, device=DEV)
        gd = torch.zeros(4, ms, H * D, dtype=torch.bfloat16, device=DEV)
        mask = torch.full((4, ms), ar.FMIN, device=DEV)
        for n, (a, e) in enumerate(zip(cul, cul[1:])):
            qd[n, :e - a], gd[n, :e - a], mask[n, :e - a] = qkv[a:e], gout[a:e], 0
        batch = dense(qd, gd, mask)
    for n, (a, e) in enumerate(zip(cul, cul[1:])):
        if e == a:
            continue
        c1, l1, d1 = batch if p else dense(qkv[a:e][None], gout[a:e][None], None)
        m = n if p else 0
        assert torch.equal(ctx[a:e], c1[m, :e - a]), n
        assert torch.equal(lse[:, a:e], l1[m, :, :e - a]), n
        assert torch.equal(x.grad[a:e], d1[m, :e - a]), n
    assert not (ctx[369:].any() or lse[:, 369:].any() or x.grad[369:].any())


def test_causal_bert_routes_to_flash(monkeypatch):
    """Not Fx.attention and not the eager chain (a zero [B,1,S,S] mask selects
    that): within the BertLayer routing test's 2 % of it; no look-ahead."""
    torch.manual_seed(5)
    cfg = BertConfig(vocab_size=512, hidden=128, layers=2, heads=2,
                     intermediate=256, max_seq=128, causal=True)
    model = to_mi355x_bert(BertForPreTraining(cfg), DEV).bert.eval()
    monkeypatch.setattr(Fx, "attention", None)
    ids = torch.randint(0, 512, (2, 128), device=DEV)
    ids2 = torch.cat([ids[:, :70], (ids[:, 70:] + 1) % 512], 1)
    with torch.no_grad():
        y, y2 = model(ids).float(), model(ids2).float()
        ye = model(ids, attn_mask=torch.zeros(2, 1, 128, 128, device=DEV)).float()
    assert torch.equal(y[:, :70], y2[:, :70])
    rel = (y - ye).norm().item() / ye.norm().item()
    print(f"causal model vs eager chain: rel {rel:.3e}")
    assert 0 < rel < 0.02, rel
