"""Packed (varlen) flash attention on the CPU: Fx.flash_attention_varlen in
fp32 runs ops/reference.py flash_attention_varlen_{fwd,bwd}, the
specification of the VARLEN kernels, and must equal plain per-sequence
softmax attention through autograd; and the per-sequence dropout masks must
be the dense [N, max_seqlen] ones cut to each length."""
import pytest
import torch

from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import reference as ref

H, D = 3, 64
SCALE = 0.125
# 1: a single key; 129: second chunk / tile hold one row; 0: an empty slot
# in the middle; 40: one partial tile starting at row 130 (no multiple of 16
# or 32); 128: exactly one tile; 296 = 2·128 + 40
LENS = [1, 129, 0, 40, 128, 296]
T = 616  # 594 used + 22 tail rows
MAX_SEQLEN = 296


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32)


def _torch_chain(qkv, lens):
    """Per-sequence softmax attention, plain torch, zeros at the tail."""
    parts, a = [], 0
    for n in lens:
        if n:
            q, k, v = (qkv[a:a + n, i].transpose(0, 1) for i in range(3))
            p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * SCALE,
                              dim=-1)
            parts.append(torch.matmul(p, v).transpose(0, 1).reshape(n, H * D))
        a += n
    parts.append(qkv.new_zeros(qkv.shape[0] - a, H * D))
    return torch.cat(parts)


def test_varlen_matches_per_sequence_attention():
    """Forward and dqkv to rtol 1e-4 / atol 1e-5 (fp32 rounding of sums of
    at most 296 terms); tail rows exactly zero in both."""
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(T, 3, H, D, generator=g) * 0.5
    gout = torch.randn(T, H * D, generator=g)
    cu = _cu(LENS)
    used = int(cu[-1])
    assert used == 594

    a = qkv.clone().requires_grad_()
    out = Fx.flash_attention_varlen(a, cu, MAX_SEQLEN, H, SCALE)
    out.backward(gout)
    r = qkv.clone().requires_grad_()
    out_r = _torch_chain(r, LENS)
    out_r.backward(gout)

    assert out.shape == (T, H * D)
    torch.testing.assert_close(out, out_r, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(a.grad, r.grad, rtol=1e-4, atol=1e-5)
    assert (out[used:] == 0).all()
    assert (a.grad[used:] == 0).all()
    assert (out[:used] != 0).any() and (a.grad[:used] != 0).any()


def test_varlen_reference_lse_layout():
    """lse is [H, T]: sequence n's rows at columns cu[n]..cu[n+1]−1."""
    g = torch.Generator().manual_seed(6)
    qkv = torch.randn(T, 3, H, D, generator=g) * 0.5
    cu = _cu(LENS)
    _, lse = ref.flash_attention_varlen_fwd(qkv, cu, MAX_SEQLEN, H, SCALE)
    assert lse.shape == (H, T) and lse.dtype == torch.float32
    a = int(cu[3])
    q, k = (qkv[a:a + 40, i].transpose(0, 1) for i in range(2))
    want = torch.logsumexp(torch.matmul(q, k.transpose(-1, -2)) * SCALE, -1)
    torch.testing.assert_close(lse[:, a:a + 40], want, rtol=1e-5, atol=1e-5)
    assert (lse[:, int(cu[-1]):] == 0).all()


def test_varlen_reference_rejects_bad_cu_seqlens():
    qkv = torch.zeros(8, 3, H, D)
    for cu in ([1, 4], [0, 5, 3], [0, 9]):
        with pytest.raises(ValueError):
            ref.flash_attention_varlen_fwd(
                qkv, torch.tensor(cu, dtype=torch.int32), 8, H, SCALE)
    with pytest.raises(ValueError):  # a sequence longer than max_seqlen
        ref.flash_attention_varlen_fwd(
            qkv, torch.tensor([0, 8], dtype=torch.int32), 4, H, SCALE)


def test_varlen_dropout_masks_are_the_dense_ones_cut_to_length():
    """Sequence n draws what batch row n of a dense [N, max_seqlen] batch
    draws: the mask does not depend on the other lengths."""
    seed, off, site, p = 1234, 7, 53, 0.1
    keeps = ref.varlen_attn_dropout_keep(seed, off, site, _cu(LENS), H,
                                         MAX_SEQLEN, p)
    dense = ref.attn_dropout_keep(seed, off, site, len(LENS), H, MAX_SEQLEN, p)
    assert len(keeps) == len(LENS)
    for n, L in enumerate(LENS):
        if L == 0:
            assert keeps[n] is None
            continue
        assert keeps[n].shape == (H, L, L) and keeps[n].dtype == torch.bool
        assert torch.equal(keeps[n], dense[n, :, :L, :L])
    assert not torch.equal(keeps[3], keeps[4][:, :40, :40])


def test_varlen_reference_applies_the_keep_list():
    """The reference with a keep list equals the dense reference with each
    sequence's own mask, forward and backward."""
    p = 0.1
    lens = [5, 0, 19]
    cu = _cu(lens)
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(26, 3, H, D, generator=g) * 0.5
    gout = torch.randn(26, H * D, generator=g)
    keeps = ref.varlen_attn_dropout_keep(3, 1, 2, cu, H, 19, p)
    rs = ref.dropout_threshold(p)[2]
    ctx, lse = ref.flash_attention_varlen_fwd(qkv, cu, 19, H, SCALE, keeps, rs)
    dqkv = ref.flash_attention_varlen_bwd(qkv, ctx, gout, lse, cu, 19, SCALE,
                                          keeps, rs)
    for n, (a, e) in enumerate(zip(cu.tolist(), cu.tolist()[1:])):
        if e == a:
            continue
        c1, l1 = ref.flash_attention_fwd(qkv[a:e][None], H, SCALE, None,
                                         keeps[n][None], rs)
        d1 = ref.flash_attention_bwd(qkv[a:e][None], c1, gout[a:e][None], l1,
                                     SCALE, None, keeps[n][None], rs)
        assert torch.equal(ctx[a:e], c1[0]) and torch.equal(dqkv[a:e], d1[0])
    assert (ctx[24:] == 0).all() and (dqkv[24:] == 0).all()


def test_varlen_dropout_needs_gpu_bf16():
    qkv = torch.zeros(8, 3, H, D)
    with pytest.raises(ValueError):
        Fx.flash_attention_varlen(qkv, _cu([8]), 8, H, SCALE, p=0.1)
