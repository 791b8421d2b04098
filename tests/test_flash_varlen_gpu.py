"""Packed (varlen) flash attention on MI355X: the VARLEN instantiations of
csrc/flash_attention.hip against the dense kernels bit for bit, against the
fp32 torch chain, with dropout against the dense padded batch, determinism,
graph replay on new lengths, and BertForPreTraining on a packed batch.

Lengths [1, 129, 0, 40, 128, 296] (sum 594) in T = 616 rows, max_seqlen 296:
1 = a single key; 129 = the second chunk / tile hold one row; 0 = an empty
slot in the middle; 40 = one partial tile, starting at row 130 (no multiple
of 16 or 32); 128 = exactly one tile; 296 = 2·128 + 40."""
import functools
import math

import pytest
import torch

import attn_dropout_refs as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, D = 3, 64
SCALE = 0.125
LENS = [1, 129, 0, 40, 128, 296]
LENS2 = [296, 0, 64, 33, 200, 1]  # the graph replay's other mix, same sum
T = 616
MAX_SEQLEN = 296
FMIN = torch.finfo(torch.float32).min
SEED, OFFSET, SITE = 0x1234_5678_9abc_def1, (3 << 32) + 7, 3
P = 0.1


def _ext():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def _fx():
    from mpi_operator_amd.ops import functional
    return functional


def _ref():
    from mpi_operator_amd.ops import reference
    return reference


def _cu_list(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def _cu(lens):
    return torch.tensor(_cu_list(lens), dtype=torch.int32, device=DEV)


def _spans(lens):
    cu = _cu_list(lens)
    return [(n, a, e) for n, (a, e) in enumerate(zip(cu, cu[1:])) if e > a]


@functools.lru_cache(maxsize=None)
def _inputs():
    """qkv [T,3,H,D], the output cotangent [T,H·D] (bf16) — read-only."""
    g = torch.Generator().manual_seed(1616)
    qkv = (torch.randn(T, 3, H, D, generator=g) * 0.5).to(torch.bfloat16)
    gout = torch.randn(T, H * D, generator=g).to(torch.bfloat16)
    return qkv.to(DEV), gout.to(DEV)


def _packed(lens, max_seqlen=MAX_SEQLEN, p=0.0, rng=None):
    """(ctx, dqkv) of Fx.flash_attention_varlen through autograd."""
    qkv, gout = _inputs()
    a = qkv.clone().requires_grad_()
    out = _fx().flash_attention_varlen(a, _cu(lens), max_seqlen, H, SCALE, p,
                                       rng, SITE)
    out.backward(gout)
    torch.cuda.synchronize()
    return out.detach(), a.grad


@functools.lru_cache(maxsize=None)
def _packed_p0():
    return _packed(tuple(LENS))


def _rng(offset=OFFSET):
    rng = _fx().DropoutRng(SEED, DEV)
    rng.set_state(SEED, offset)
    return rng


# ------------------------------------------------------ 1. bit-identity, p = 0
def test_packed_equals_dense_per_sequence_bit_for_bit():
    """Each non-empty sequence of the packed call equals the dense kernels
    on its slice as a [1, L] batch: ctx and dqkv through Fx.flash_attention,
    ctx, lse and dqkv through the extension entry points. No tolerance: same
    tiles, same order, same roundings."""
    fx, ext = _fx(), _ext()
    qkv, gout = _inputs()
    ctx, dqkv = _packed_p0()
    assert ctx.shape == (T, H * D) and ctx.dtype == torch.bfloat16
    assert dqkv.shape == qkv.shape
    ctx_e, lse = ext.flash_attn_varlen_fwd(qkv, _cu(LENS), MAX_SEQLEN, H,
                                           SCALE)
    assert lse.shape == (H, T) and lse.dtype == torch.float32
    assert torch.equal(ctx_e, ctx)
    for n, a, e in _spans(LENS):
        q1 = qkv[a:e][None].contiguous()
        g1 = gout[a:e][None].contiguous()
        c1, l1 = ext.flash_attn_fwd(q1, H, SCALE, None)
        d1 = ext.flash_attn_bwd(q1, c1, g1, l1, SCALE, None)
        assert torch.equal(ctx[a:e], c1[0]), n
        assert torch.equal(lse[:, a:e], l1[0]), n
        assert torch.equal(dqkv[a:e], d1[0]), n
        x = q1.clone().requires_grad_()
        o = fx.flash_attention(x, H, SCALE)
        o.backward(g1)
        assert torch.equal(ctx[a:e], o[0]) and torch.equal(dqkv[a:e], x.grad[0])
        assert (c1 != 0).any() and (d1 != 0).any()


def test_extra_grid_rows_change_nothing():
    """max_seqlen = 512 adds two grid rows of workgroups that only exit."""
    ctx, dqkv = _packed_p0()
    ctx5, dqkv5 = _packed(tuple(LENS), max_seqlen=512)
    assert torch.equal(ctx5, ctx) and torch.equal(dqkv5, dqkv)


def test_tail_rows_are_zero():
    qkv, _ = _inputs()
    ctx, dqkv = _packed_p0()
    _, lse = _ext().flash_attn_varlen_fwd(qkv, _cu(LENS), MAX_SEQLEN, H, SCALE)
    used = sum(LENS)
    assert T - used == 22
    assert (ctx[used:] == 0).all() and (dqkv[used:] == 0).all()
    assert (lse[:, used:] == 0).all()
    assert torch.isfinite(ctx.float()).all()
    assert torch.isfinite(dqkv.float()).all()


# ---------------------------------------------------------- 2. against fp32
def test_packed_against_fp32_chain():
    """Per-sequence fp32 torch chain on the bf16-rounded input; the bounds
    of test_flash_attention_gpu.py."""
    qkv, gout = _inputs()
    ctx, dqkv = _packed_p0()
    r = qkv.float().requires_grad_()
    parts = []
    for _, a, e in _spans(LENS):
        q, k, v = (r[a:e, i].transpose(0, 1) for i in range(3))
        p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * SCALE, -1)
        parts.append(torch.matmul(p, v).transpose(0, 1).reshape(e - a, H * D))
    parts.append(r.new_zeros(T - sum(LENS), H * D))
    out_r = torch.cat(parts)
    out_r.backward(gout.float())
    ferr = (ctx.float() - out_r).abs().max().item()
    gerr = (dqkv.float() - r.grad).abs().max().item()
    gmax = r.grad.abs().max().item()
    print(f"packed {LENS}: fwd err {ferr:.3e}, grad err {gerr:.3e} "
          f"(max |ref grad| {gmax:.3e})")
    assert ferr < 0.02, ferr
    assert gerr < 0.08 * gmax + 2e-3, (gerr, gmax)


# ------------------------------------------------------------- 3. dropout
def test_packed_dropout_equals_dense_padded_batch():
    """p = 0.1 at max_seqlen = 296 against Fx.flash_attention on the same
    sequences padded to [6, 296] with the key mask, the same (seed, offset,
    site), dctx zero at pad rows. The dense batch keeps all six rows, so
    n needs no adjusting; its row 2 (the empty slot, fully masked: outside
    the dense contract) is left out of the comparison."""
    fx = _fx()
    qkv, gout = _inputs()
    N = len(LENS)
    qd = torch.zeros(N, MAX_SEQLEN, 3, H, D, dtype=torch.bfloat16, device=DEV)
    gd = torch.zeros(N, MAX_SEQLEN, H * D, dtype=torch.bfloat16, device=DEV)
    mask = torch.full((N, MAX_SEQLEN), FMIN, device=DEV)
    for n, a, e in _spans(LENS):
        qd[n, :e - a], gd[n, :e - a] = qkv[a:e], gout[a:e]
        mask[n, :e - a] = 0
    x = qd.clone().requires_grad_()
    od = fx.flash_attention(x, H, SCALE, mask, P, _rng(), SITE)
    od.backward(gd)
    ctx, dqkv = _packed(tuple(LENS), p=P, rng=_rng())
    for n, a, e in _spans(LENS):
        assert torch.equal(ctx[a:e], od[n, :e - a]), n
        assert torch.equal(dqkv[a:e], x.grad[n, :e - a]), n
    ctx0, _ = _packed_p0()
    assert not torch.equal(ctx, ctx0)
    used = sum(LENS)
    assert (ctx[used:] == 0).all() and (dqkv[used:] == 0).all()


def test_packed_dropout_mask_and_kept_fraction():
    """The forward's keep bits, read out exactly with one-hot V (the scheme
    of attn_dropout_refs: ctx[i, h, d] != 0 <=> keep[h, i, 64w + d]), equal
    ref.varlen_attn_dropout_keep, and the kept fraction over all valid
    (h, i, j) is within 4 sigma of 1 - thr/65536, sigma the binomial
    standard deviation at that count."""
    ref, ext = _ref(), _ext()
    qkv, _ = _inputs()
    rng = _rng()
    cu = _cu(LENS)
    got = {n: torch.zeros(H, e - a, e - a, dtype=torch.bool, device=DEV)
           for n, a, e in _spans(LENS)}
    for w in ar.windows(MAX_SEQLEN):
        x = qkv.clone()
        for n, a, e in _spans(LENS):
            if 64 * w < e - a:
                x[a:e, 2] = ar._onehot_rows(e - a, w, DEV)[:, None, :]
        ctx, _ = ext.flash_attn_varlen_drop_fwd(x, cu, MAX_SEQLEN, H, SCALE,
                                                rng.state, P, SITE)
        ctx = ctx.view(T, H, D)
        for n, a, e in _spans(LENS):
            m = min(D, e - a - 64 * w)
            if m > 0:
                got[n][:, :, 64 * w:64 * w + m] = \
                    (ctx[a:e, :, :m] != 0).permute(1, 0, 2)
    want = ref.varlen_attn_dropout_keep(SEED, OFFSET, SITE, cu.cpu(), H,
                                        MAX_SEQLEN, P)
    kept = count = 0
    for n, a, e in _spans(LENS):
        assert torch.equal(got[n].cpu(), want[n]), n
        kept += int(got[n].sum())
        count += got[n].numel()
    assert count == H * sum(n * n for n in LENS)
    thr = ref.dropout_threshold(P)[0]
    q = 1 - thr / 65536
    sigma = math.sqrt(q * (1 - q) / count)
    frac = kept / count
    print(f"kept {kept}/{count} = {frac:.5f}, expected {q:.5f}, "
          f"sigma {sigma:.2e}")
    assert abs(frac - q) < 4 * sigma, (frac, q, sigma)


# --------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("p", [0.0, P])
def test_packed_backward_deterministic(p):
    ext = _ext()
    qkv, gout = _inputs()
    cu = _cu(LENS)
    if p:
        st = _rng().state
        ctx, lse = ext.flash_attn_varlen_drop_fwd(qkv, cu, MAX_SEQLEN, H,
                                                  SCALE, st, p, SITE)
        d1, d2 = (ext.flash_attn_varlen_drop_bwd(
            qkv, ctx, gout, lse, cu, MAX_SEQLEN, SCALE, st, p, SITE)
            for _ in range(2))
    else:
        ctx, lse = ext.flash_attn_varlen_fwd(qkv, cu, MAX_SEQLEN, H, SCALE)
        d1, d2 = (ext.flash_attn_varlen_bwd(qkv, ctx, gout, lse, cu,
                                            MAX_SEQLEN, SCALE)
                  for _ in range(2))
    assert torch.equal(d1, d2)
    assert (d1 != 0).any()


# -------------------------------------------------------- 5. graph replay
def test_graph_replays_on_new_lengths():
    """Forward + backward captured once on LENS; cu_seqlens overwritten in
    place with LENS2 (same sum, same T); the replay equals an eager call on
    LENS2."""
    fx = _fx()
    qkv, gout = _inputs()
    assert sum(LENS2) == sum(LENS) and max(LENS2) <= MAX_SEQLEN
    cu = _cu(LENS)
    x = qkv.clone().requires_grad_()

    def step():
        x.grad = None
        out = fx.flash_attention_varlen(x, cu, MAX_SEQLEN, H, SCALE)
        out.backward(gout)
        return out

    step()  # eager warm-up
    x.grad = None
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    g.replay()
    torch.cuda.synchronize()
    ctx1, dqkv1 = _packed_p0()
    assert torch.equal(out.detach(), ctx1) and torch.equal(x.grad, dqkv1)
    cu.copy_(_cu(LENS2))
    g.replay()
    torch.cuda.synchronize()
    ctx2, dqkv2 = _packed(tuple(LENS2))
    assert torch.equal(out.detach(), ctx2) and torch.equal(x.grad, dqkv2)
    assert not torch.equal(ctx2, ctx1)


# ------------------------------------------------------------ bindings
def test_bindings_reject_bad_arguments():
    ext = _ext()
    qkv, gout = _inputs()
    cu = _cu(LENS)
    with pytest.raises(RuntimeError):  # int64 cu_seqlens
        ext.flash_attn_varlen_fwd(qkv, cu.long(), MAX_SEQLEN, H, SCALE)
    with pytest.raises(RuntimeError):  # on the CPU
        ext.flash_attn_varlen_fwd(qkv, cu.cpu(), MAX_SEQLEN, H, SCALE)
    with pytest.raises(RuntimeError):  # fewer than 2 entries
        ext.flash_attn_varlen_fwd(qkv, cu[:1], MAX_SEQLEN, H, SCALE)
    with pytest.raises(RuntimeError):  # not contiguous
        ext.flash_attn_varlen_fwd(qkv, cu[::2], MAX_SEQLEN, H, SCALE)
    with pytest.raises(RuntimeError):  # max_seqlen < 1
        ext.flash_attn_varlen_fwd(qkv, cu, 0, H, SCALE)
    with pytest.raises(RuntimeError):  # wrong head count
        ext.flash_attn_varlen_fwd(qkv, cu, MAX_SEQLEN, H + 1, SCALE)
    with pytest.raises(RuntimeError):  # dense layout
        ext.flash_attn_varlen_fwd(qkv[None], cu, MAX_SEQLEN, H, SCALE)
    ctx, lse = ext.flash_attn_varlen_fwd(qkv, cu, MAX_SEQLEN, H, SCALE)
    with pytest.raises(RuntimeError):  # lse of another T
        ext.flash_attn_varlen_bwd(qkv, ctx, gout, lse[:, :-1].contiguous(), cu,
                                  MAX_SEQLEN, SCALE)
    with pytest.raises(RuntimeError):  # the dropout state on the CPU
        ext.flash_attn_varlen_drop_fwd(qkv, cu, MAX_SEQLEN, H, SCALE,
                                       torch.zeros(2, dtype=torch.int64), P,
                                       SITE)


# ------------------------------------------------------ 6. model routing
B_M, S_M = 3, 48
LENS_M = [48, 17, 5]
VOCAB = 1000


def _model(dropout=0.0, attn_dropout=0.0):
    from mpi_operator_amd.models import bert as Bm
    torch.manual_seed(3)
    cfg = Bm.BertConfig(vocab_size=VOCAB, hidden=128, layers=2, heads=2,
                        intermediate=256, max_seq=64, dropout=dropout,
                        attn_dropout=attn_dropout)
    m = Bm.to_mi355x_bert(Bm.BertForPreTraining(cfg), DEV)
    m.seed_dropout(SEED)
    return m.train()


def _model_batch():
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(1, VOCAB, (B_M, S_M), generator=g)
    typ = torch.randint(0, 2, (B_M, S_M), generator=g)
    mask = (torch.arange(S_M)[None] < torch.tensor(LENS_M)[:, None]).long()
    labels = torch.where(mask.bool(),
                         torch.randint(0, VOCAB, (B_M, S_M), generator=g),
                         torch.full((B_M, S_M), -100))
    nsp = torch.tensor([1, 0, 1])
    return tuple(t.to(DEV) for t in (ids, typ, mask, labels, nsp))


def _spy(monkeypatch):
    fx = _fx()
    calls = []
    for name in ("flash_attention_varlen", "flash_attention", "attention"):
        real = getattr(fx, name)

        def spy(*a, _real=real, _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)

        monkeypatch.setattr(fx, name, spy)
    return calls


def _packed_args(m):
    from mpi_operator_amd.models.bert import pack_padded_batch
    ids, typ, mask, labels, _ = _model_batch()
    pk = pack_padded_batch(ids, typ, mask, labels, token_budget=80,
                           max_sequences=5, max_seq=m.cfg.max_seq)
    nsp = torch.tensor([1, 0, 1, -100, -100], device=DEV)
    return (pk.ids, pk.type_ids, None, pk.mlm_labels, nsp), dict(
        cu_seqlens=pk.cu_seqlens, max_seqlen=pk.max_seqlen,
        position_ids=pk.position_ids)


def test_bert_packed_routes_to_varlen_kernels(monkeypatch):
    """Padded-and-masked against packed: the packed step calls
    Fx.flash_attention_varlen once per layer and never Fx.flash_attention;
    loss and every gradient within 0.02 relative (the bound of
    test_bert_layer_routes_to_flash_attention)."""
    calls = _spy(monkeypatch)
    m = _model()

    def run(*a, **kw):
        del calls[:]
        m.zero_grad()
        loss = m(*a, **kw)
        loss.backward()
        torch.cuda.synchronize()
        return (loss.item(), {n: p.grad.detach().float().clone()
                              for n, p in m.named_parameters()}, list(calls))

    l_p, g_p, c_p = run(*_model_batch())
    args, kw = _packed_args(m)
    l_k, g_k, c_k = run(*args, **kw)
    assert c_p == ["flash_attention"] * 2, c_p
    assert c_k == ["flash_attention_varlen"] * 2, c_k
    print(f"loss padded {l_p:.5f} packed {l_k:.5f}")
    assert abs(l_k - l_p) / abs(l_p) < 0.02, (l_k, l_p)

    def rel(a, r):
        return (a - r).norm().item() / (r.norm().item() + 1e-30)

    for n in g_p:
        assert rel(g_k[n], g_p[n]) < 0.02, (n, rel(g_k[n], g_p[n]))


def test_bert_packed_with_dropout(monkeypatch):
    """dropout = attn_dropout = 0.1 on the packed path: finite loss and
    gradients, and two consecutive steps differ."""
    calls = _spy(monkeypatch)
    m = _model(0.1, 0.1)
    args, kw = _packed_args(m)
    losses = []
    for _ in range(2):
        m.zero_grad()
        loss = m(*args, **kw)
        loss.backward()
        assert torch.isfinite(loss)
        for n, p in m.named_parameters():
            assert torch.isfinite(p.grad.float()).all(), n
        losses.append(loss.item())
    assert calls == ["flash_attention_varlen"] * 4, calls
    assert losses[0] != losses[1], losses
