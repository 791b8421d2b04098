"""Attention-probability dropout on the CPU: the mask scheme of
csrc/philox.h as ops/reference.py attn_dropout_keep mirrors it, the reference
forward/backward with a mask against fp64 autograd, the read-outs that
test_attn_dropout_gpu.py uses to extract the kernels' masks, and BertModel
with BertConfig.attn_dropout."""
import math

import numpy as np
import pytest
import torch

import attn_dropout_refs as ar
from mpi_operator_amd.models import bert as bert_mod
from mpi_operator_amd.models.bert import BertConfig, BertForPreTraining
from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import reference as ref

SEED, OFFSET, SITE = 0x1234_5678_9abc_def1, (3 << 32) + 7, 3
B, H = 2, 3


# ------------------------------------------------------------ mask scheme
@pytest.mark.parametrize("S", [40, 129])
def test_call_ids_unique_and_slots_are_the_stated_rows(S):
    """(call, slot) is unique per element; every call serves at most 8
    elements, all in one column j of one (b, h), and slot s of the call of
    (band, half) is row 16·band + 4·half + (s & 3) + 8·(s >> 2) — the rows one
    lane holds of a 32×32 MFMA result, (r&3) + 8·(r>>2) + 4·(lane>>5), for
    registers r = 8·(band & 1) + s."""
    call, slot = ref.attn_dropout_call_slot(B, H, S)
    assert call.shape == slot.shape == (B * H, S, S)
    nb = (S + 15) // 16
    assert call.min() == 0 and call.max() < B * H * nb * 2 * S
    flat = call.reshape(-1) * 8 + slot.reshape(-1)
    assert np.unique(flat).size == B * H * S * S
    # rebuild every element's (call, slot) from the statement above
    want_call = np.full((B * H, S, S), -1, dtype=np.int64)
    want_slot = np.full((B * H, S, S), -1, dtype=np.int64)
    j = np.arange(S)
    for bh in range(B * H):
        for band in range(nb):
            for half in range(2):
                c = ((bh * nb + band) * 2 + half) * S + j
                for s in range(8):
                    i = 16 * band + 4 * half + (s & 3) + 8 * (s >> 2)
                    if i < S:
                        assert (want_call[bh, i] == -1).all()
                        want_call[bh, i] = c
                        want_slot[bh, i] = s
    assert (want_call == call).all() and (want_slot == slot).all()
    # the MFMA C-layout: lane half `half`, register r -> row within 32
    for r in range(16):
        for half in range(2):
            row = (r & 3) + 8 * (r >> 2) + 4 * half
            assert slot[0, row % S, 0] == r % 8 or row >= S
            assert row >> 4 == r >> 3
    counts = np.unique(call, return_counts=True)[1]
    assert counts.max() == 8
    if S % 16 == 0:
        assert counts.min() == 8


def test_mask_bits_equal_philox_by_hand():
    S, p = 40, 0.3
    thr = ref.dropout_threshold(p)[0]
    keep = ref.attn_dropout_keep(SEED, OFFSET, SITE, B, H, S, p)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (B, H, S, S)
    nb = (S + 15) // 16
    key = (SEED & 0xffffffff, SEED >> 32)
    for b, h, i, j in [(0, 0, 0, 0), (0, 0, 5, 1), (0, 1, 12, 39), (1, 2, 39, 7),
                       (1, 0, 20, 20), (0, 2, 31, 0), (1, 1, 35, 38)]:
        u = i & 15
        band, half, slot = i >> 4, (u >> 2) & 1, (u & 3) + 4 * (u >> 3)
        call = (((b * H + h) * nb + band) * 2 + half) * S + j
        w = ref.philox4x32_10(
            (call, SITE, OFFSET & 0xffffffff, OFFSET >> 32), key)
        r = (int(w[slot >> 1]) >> (16 * (slot & 1))) & 0xffff
        assert bool(keep[b, h, i, j]) == (r >= thr), (b, h, i, j)


def test_mask_differs_across_site_offset_b_h():
    S = 48
    n = S * S
    base = ref.attn_dropout_keep(SEED, OFFSET, SITE, B, H, S, 0.5)
    site = ref.attn_dropout_keep(SEED, OFFSET, SITE + 1, B, H, S, 0.5)
    step = ref.attn_dropout_keep(SEED, OFFSET + 1, SITE, B, H, S, 0.5)
    pairs = [("site", base[0, 0], site[0, 0]), ("offset", base[0, 0], step[0, 0]),
             ("b", base[0, 0], base[1, 0]), ("h", base[0, 0], base[0, 1])]
    for name, x, y in pairs:
        # independent fair masks agree on half their bits: 5 sigma of n/2
        agree = int((x == y).sum())
        assert abs(agree - n / 2) < 5 * math.sqrt(n / 4), (name, agree, n)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_within_5_sigma(p):
    S = 128
    keep = ref.attn_dropout_keep(SEED, OFFSET, SITE, B, H, S, p)
    p_eff = ref.dropout_threshold(p)[1]
    n = B * H * S * S
    sigma = math.sqrt(p_eff * (1 - p_eff) / n)
    rate = keep.double().mean().item()
    print(f"p={p}: keep rate {rate:.6f}, want {1 - p_eff:.6f} ± {5 * sigma:.6f}")
    assert abs(rate - (1 - p_eff)) < 5 * sigma, (rate, p_eff, sigma)


def test_keep_rejects_bad_arguments():
    with pytest.raises(ValueError):
        ref.attn_dropout_keep(1, 0, 0, 1, 1, 16, 1.0)
    with pytest.raises(ValueError):
        ref.attn_dropout_keep(1, 0, 1 << 32, 1, 1, 16, 0.5)
    with pytest.raises(ValueError):  # 2^15 · 2^11 · 2 · 2^15 = 2^42 calls
        ref.attn_dropout_call_slot(1 << 10, 32, 1 << 15)
    qkv = torch.zeros(1, 16, 3, 1, 64)
    for fn in (Fx.attention, Fx.flash_attention):
        with pytest.raises(ValueError):  # p > 0 is GPU bf16 only
            fn(qkv, 1, 0.125, None, 0.1, None, 0)
        with pytest.raises(ValueError):
            fn(qkv, 1, 0.125, None, 1.0, None, 0)


# --------------------------------------------- reference forward / backward
@pytest.mark.parametrize("S,masked", [(40, False), (72, True)])
def test_reference_dropout_matches_fp64_autograd(S, masked):
    """ref.flash_attention_fwd / _bwd with keep and drop_scale against fp64
    autograd of O = rs·(softmax(S)∘keep)·V on the same mask. The reference
    works in fp32 on sums of at most S = 72 terms of magnitude <= ~4: bound
    1e-4 absolute, relative to the largest reference value."""
    p = 0.5
    rs = ref.dropout_threshold(p)[2]
    qkv, gout = ar.inputs(B, H, S, "cpu")
    mask = ar.key_mask(S, [S, S - 37], "cpu") if masked else None
    keep = ref.attn_dropout_keep(SEED, OFFSET, SITE, B, H, S, p)
    out64, grad64, lse64 = ar.chain(qkv, gout, mask, keep, rs, torch.float64)
    x = qkv.float()
    ctx, lse = ref.flash_attention_fwd(x, H, ar.SCALE, mask, keep, rs)
    dqkv = ref.flash_attention_bwd(x, ctx, gout.float(), lse, ar.SCALE, mask,
                                   keep, rs)
    for name, got, want in (("ctx", ctx, out64), ("lse", lse, lse64),
                            ("dqkv", dqkv, grad64)):
        err = (got.double() - want).abs().max().item()
        bound = 1e-4 * max(1.0, want.abs().max().item())
        print(f"S={S} {name}: err {err:.3e} bound {bound:.3e}")
        assert err < bound, (name, err, bound)
    # lse is that of the undropped softmax
    assert torch.equal(lse, ref.flash_attention_fwd(x, H, ar.SCALE, mask)[1])
    # and without keep the functions are what they were
    c0, l0 = ref.flash_attention_fwd(x, H, ar.SCALE, mask)
    c1, l1 = ref.flash_attention_fwd(x, H, ar.SCALE, mask, None, 1.0)
    assert torch.equal(c0, c1) and torch.equal(l0, l1)


@pytest.mark.parametrize("S,masked", [(129, False), (72, True)])
def test_readouts_recover_the_mask_from_the_reference(S, masked):
    """The three one-hot read-outs of attn_dropout_refs, driven by the CPU
    reference, return the mask that went in, and the dQ read-out leaves no
    element out."""
    p = 0.5
    rs = ref.dropout_threshold(p)[2]
    qkv, gout = ar.inputs(B, H, S, "cpu")
    mask = ar.key_mask(S, [S, S - 37], "cpu") if masked else None
    keep = ref.attn_dropout_keep(SEED, OFFSET, SITE, B, H, S, p)
    want = keep.clone()
    if masked:
        want &= (mask == 0)[:, None, None, :]

    def fwd(x):
        return ref.flash_attention_fwd(x, H, ar.SCALE, mask, keep, rs)[0]

    def bwd(x, ctx, dctx, lse):
        return ref.flash_attention_bwd(x, ctx, dctx, lse, ar.SCALE, mask,
                                       keep, rs)

    assert torch.equal(ar.read_fwd_mask(fwd, qkv, mask), want)
    ctx, lse = ref.flash_attention_fwd(qkv, H, ar.SCALE, mask, keep, rs)
    assert torch.equal(ar.read_dkv_mask(bwd, qkv, ctx, lse, mask), want)
    got, left = ar.read_dq_mask(bwd, qkv, gout, mask)
    assert int(left.sum()) == 0
    assert torch.equal(got, want)


# ------------------------------------------------------------------ model
def _cfg(dropout=0.0, attn_dropout=0.0):
    return BertConfig(vocab_size=128, hidden=64, layers=2, heads=4,
                      intermediate=128, max_seq=32, dropout=dropout,
                      attn_dropout=attn_dropout)


def _model(dropout, attn_dropout):
    torch.manual_seed(0)
    return BertForPreTraining(_cfg(dropout, attn_dropout))


def _ids():
    g = torch.Generator().manual_seed(3)
    return torch.randint(0, 128, (2, 24), generator=g)


def test_bert_config_and_constructors():
    assert BertConfig().attn_dropout == 0.0
    assert bert_mod.BertConfig(attn_dropout=0.1).dropout == 0.0
    import inspect
    for f in (bert_mod.bert_large, bert_mod.bert_base):
        assert inspect.signature(f).parameters["attn_dropout"].default == 0.0


def test_bert_cpu_attn_dropout_runs_and_differs_from_eval():
    m = _model(0.0, 0.3)
    ids = _ids()
    m.eval()
    with torch.no_grad():
        e = m(ids)[0]
    m0 = _model(0.0, 0.0).eval()
    with torch.no_grad():
        assert torch.equal(e, m0(ids)[0])  # eval ignores attn_dropout
    m.train()
    torch.manual_seed(7)
    t1 = m(ids)[0]
    t2 = m(ids)[0]
    assert torch.isfinite(t1).all()
    assert not torch.equal(t1.detach(), e)
    assert not torch.equal(t1.detach(), t2.detach())  # fresh masks per forward
    t1.float().square().mean().backward()
    g = m.bert.layers[0].attn.qkv.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0


def test_bert_cpu_attn_dropout_zero_is_the_old_forward(monkeypatch):
    """attn_dropout = 0 with hidden-state dropout on: bit-equal, for the same
    torch seed, to the model whose SelfAttention.forward is the eager chain
    as it stood before attn_dropout existed (no extra random draws, nothing
    reordered)."""
    ids = _ids()
    m = _model(0.1, 0.0).train()
    torch.manual_seed(11)
    new = m(ids)[0].detach()

    def old_forward(self, x, attn_mask=None, *_):
        b, s, h = x.shape
        qkv = self.qkv(x).view(b, s, 3, self.heads, self.head_dim)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        scores = torch.matmul(q, k.transpose(-1, -2)) * self.scale
        if attn_mask is not None:
            scores = scores + attn_mask
        probs = torch.softmax(scores.float(), dim=-1).to(v.dtype)
        ctx = torch.matmul(probs, v).transpose(1, 2).reshape(b, s, h)
        return self.out(ctx)

    monkeypatch.setattr(bert_mod.SelfAttention, "forward", old_forward)
    torch.manual_seed(11)
    old = m(ids)[0].detach()
    assert torch.equal(new, old)
