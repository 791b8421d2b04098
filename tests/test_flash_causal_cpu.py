"""Causal attention off the GPU: reference.py and Fx on CPU fp32 against an
fp64 explicit-mask chain, and BertConfig(causal=True)."""
import pytest
import torch

from mpi_operator_amd.models.bert import BertConfig, BertModel
from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import reference as ref

H, D, SCALE = 2, 16, 0.25
CU = [0, 129, 129, 169, 369]  # lengths [129, 0, 40, 200]


def _check(qkv, gout, out, dqkv, lse):
    """One [S,3,H,D] sequence against the fp64 chain with an additive mask."""
    S = qkv.shape[0]
    r = qkv.double().requires_grad_()
    q, k, v = (r[:, i].transpose(0, 1) for i in range(3))
    mask = torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1)
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE + mask
    o = torch.matmul(torch.softmax(s, -1), v).transpose(0, 1).reshape(S, H * D)
    o.backward(gout.double())
    for got, want in ((out, o.detach()), (dqkv, r.grad),
                      (lse, torch.logsumexp(s.detach(), -1))):
        assert torch.allclose(got.double(), want, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("cul,T", [([0, 5], 5), ([0, 129], 129),
                                   ([0, 296], 296), (CU, 400)])
def test_causal_references_cpu(cul, T):
    """Packed Fx against fp64 per sequence; dense Fx on each alone equals it."""
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(T, 3, H, D, generator=g)
    gout = torch.randn(T, H * D, generator=g)
    cu = torch.tensor(cul, dtype=torch.int32)
    x = qkv.clone().requires_grad_()
    y = Fx.flash_attention_varlen(x, cu, 296, H, SCALE, causal=True)
    y.backward(gout)
    lse = ref.flash_attention_varlen_fwd(qkv, cu, 296, H, SCALE, causal=True)[1]
    for a, e in zip(cul, cul[1:]):
        if e == a:
            continue
        _check(qkv[a:e], gout[a:e], y[a:e], x.grad[a:e], lse[:, a:e])
        xd = qkv[a:e][None].clone().requires_grad_()
        yd = Fx.flash_attention(xd, H, SCALE, causal=True)
        yd.backward(gout[a:e][None])
        assert torch.equal(yd[0], y[a:e]) and torch.equal(xd.grad[0], x.grad[a:e])
    assert not (y[cul[-1]:].any() or x.grad[cul[-1]:].any())


def test_bert_causal_cpu():
    """No look-ahead; equal to the non-causal eager path given the explicit
    [B,1,S,S] lower-triangular mask."""
    torch.manual_seed(3)
    model = BertModel(BertConfig(vocab_size=64, hidden=32, layers=2, heads=2,
                                 intermediate=64, max_seq=16, causal=True)).eval()
    ids = torch.randint(0, 64, (2, 12))
    ids2 = torch.cat([ids[:, :7], (ids[:, 7:] + 1) % 64], 1)
    tri = torch.full((12, 12), torch.finfo(torch.float32).min).triu(1)
    with torch.no_grad():
        y, y2 = model(ids), model(ids2)
        for layer in model.layers:
            layer.attn.causal = False
        ym = model(ids, attn_mask=tri.expand(2, 1, 12, 12))
    assert torch.equal(y[:, :7], y2[:, :7]) and not torch.equal(y, model(ids))
    assert torch.allclose(y, ym, atol=1e-5)
