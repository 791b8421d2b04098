"""Flash attention, CPU tier: the fp32 reference functions (the kernels'
specification — P recomputed from the row log-sum-exp, delta from dctx·ctx)
against the plain autograd chain softmax(QKᵀ·scale + mask)·V."""
import pytest
import torch

from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import reference as ref

B, S, H, D = 2, 37, 3, 64
SCALE = 0.125


def _inputs(masked):
    torch.manual_seed(5)
    qkv = torch.randn(B, S, 3, H, D) * 0.5
    gout = torch.randn(B, S, H * D)
    mask = None
    if masked:
        mask = torch.zeros(B, S)
        mask[1, S - 9:] = torch.finfo(torch.float32).min
    return qkv, gout, mask


def _chain(qkv, mask):
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if mask is not None:
        s = s + mask[:, None, None, :]
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D), s


@pytest.mark.parametrize("masked", [False, True])
def test_flash_attention_cpu_matches_autograd_chain(masked):
    qkv, gout, mask = _inputs(masked)
    a = qkv.clone().requires_grad_()
    out = Fx.flash_attention(a, H, SCALE, mask)
    out.backward(gout)
    r = qkv.clone().requires_grad_()
    out_r, _ = _chain(r, mask)
    out_r.backward(gout)
    assert out.shape == (B, S, H * D)
    err = (out - out_r).abs().max().item()
    assert err < 1e-5 * out_r.abs().max().item(), err
    gerr = (a.grad - r.grad).abs().max().item()
    assert gerr < 1e-5 * r.grad.abs().max().item(), gerr


@pytest.mark.parametrize("masked", [False, True])
def test_reference_lse_is_logsumexp(masked):
    qkv, _, mask = _inputs(masked)
    _, lse = ref.flash_attention_fwd(qkv, H, SCALE, mask)
    _, s = _chain(qkv, mask)
    assert lse.shape == (B, H, S) and lse.dtype == torch.float32
    assert (lse - torch.logsumexp(s, dim=-1)).abs().max().item() < 1e-5
