"""Attention-probability dropout in the attention kernels on MI355X
(csrc/attention.hip attn_fwd_k / attn_bwd_k with DROP, csrc/flash_attention.hip
flash_attn_fwd_k / _bwd_dkv_k / _bwd_dq_k with DROP): every mask bit against
the CPU reference ref.attn_dropout_keep, values against the fp32 chain of
test_flash_attention_gpu._case with that mask inserted, graph replay, and
BertConfig.attn_dropout end to end.

Bounds: those of test_flash_attention_gpu (0.02 on ctx, 0.08·gmax + 2e-3 on
dqkv) times rs = 1/(1 - p_eff): every output term carries the factor rs and
nothing else changes. gmax is taken as the smaller of max|grad| of the
dropped and of the undropped chain.

Shapes. Saved-probs path: S = 40 (half-filled last 16-row band, rows past
S), 128 (attn_bwd_k<true>), 200 (S_MAX = 256, two q-chunks, torch fallback).
Flash path: S = 129 and 296 (a second / third tile holding 1 / 40 rows) and
S = 72 with a key mask of valid lengths [S, S - 37]."""
import functools

import pytest
import torch

import attn_dropout_refs as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, D = 2, 3, 64
SCALE = ar.SCALE
SEED, OFFSET, SITE = 0x1234_5678_9abc_def1, (3 << 32) + 7, 3
PS = [0.1, 0.5]


def _ext():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def _fx():
    from mpi_operator_amd.ops import functional
    return functional


def _ref():
    from mpi_operator_amd.ops import reference
    return reference


def _rng(offset=OFFSET):
    rng = _fx().DropoutRng(SEED, DEV)
    rng.set_state(SEED, offset)
    return rng


@functools.lru_cache(maxsize=None)
def _keep(S, p, offset=OFFSET, site=SITE):
    return _ref().attn_dropout_keep(SEED, offset, site, B, H, S, p).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(S, masked, p):
    """Inputs, the reference mask and the fp32 chain with it inserted (out,
    dqkv, gmax); computed once and shared — read-only."""
    qkv, gout = ar.inputs(B, H, S, DEV)
    mask = ar.key_mask(S, [S, S - 37], DEV) if masked else None
    keep = _keep(S, p)
    rs = _ref().dropout_threshold(p)[2]
    out_r, grad_r, _ = ar.chain(qkv, gout, mask, keep, rs)
    _, grad_0, _ = ar.chain(qkv, gout, mask, None, 1.0)
    gmax = min(grad_r.abs().max().item(), grad_0.abs().max().item())
    return dict(qkv=qkv, gout=gout, mask=mask, keep=keep, rs=rs, out=out_r,
                grad=grad_r, gmax=gmax)


def _check_values(tag, c, out, grad):
    rs, gmax = c["rs"], c["gmax"]
    assert out.dtype == torch.bfloat16 and grad.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all() and torch.isfinite(grad.float()).all()
    ferr = (out.float() - c["out"]).abs().max().item()
    gerr = (grad.float() - c["grad"]).abs().max().item()
    print(f"{tag}: fwd err {ferr:.3e} (bound {0.02 * rs:.3e}), grad err "
          f"{gerr:.3e} (bound {0.08 * rs * gmax + 2e-3 * rs:.3e}, gmax {gmax:.3e})")
    assert ferr < 0.02 * rs, ferr
    assert gerr < 0.08 * rs * gmax + 2e-3 * rs, (gerr, gmax)


# --------------------------------------------------- saved-probs path, S <= 256
def _saved_probs(S, masked, p):
    c = _case(S, masked, p)
    ext = _ext()
    ctx, sp = ext.attn_drop_fwd(c["qkv"], H, SCALE, c["mask"], _rng().state, p,
                                SITE)
    assert tuple(sp.shape) == (B, H, S, S) and sp.dtype == torch.bfloat16
    # the mask, bit for bit, from the sign bit itself
    assert torch.equal(~torch.signbit(sp), c["keep"])
    # |probs| is the dropout-free kernel's probs, bit for bit
    ctx0, p0 = ext.attn_fwd(c["qkv"], H, SCALE, c["mask"], True)
    assert torch.equal(sp.abs().view(torch.int16), p0.view(torch.int16))
    # the whole Function: S = 128 runs attn_bwd_k<true>, else the torch chain
    a = c["qkv"].clone().requires_grad_()
    out = _fx().attention(a, H, SCALE, c["mask"], p, _rng(), SITE)
    out.backward(c["gout"])
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), ctx)
    _check_values(f"saved-probs S={S} masked={masked} p={p}", c, out.detach(),
                  a.grad)
    return c, a.grad


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("S", [40, 128, 200])
def test_saved_probs_path(S, p):
    _saved_probs(S, False, p)


def test_saved_probs_path_key_mask():
    S = 72
    c, grad = _saved_probs(S, True, 0.1)
    assert (grad[1, S - 37:, 1:] == 0).all()  # masked keys: dK = dV = 0
    assert (grad[0, :, 1:] != 0).any()


# ------------------------------------------------------------------ flash path
FLASH = [(129, False), (296, False), (72, True)]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("S,masked", FLASH)
def test_flash_masks_read_out_exactly(S, masked, p):
    """Forward, dK/dV and dQ kernels each draw the reference mask: read from
    the nonzero patterns of ctx, dV and dQ under one-hot V, dO and K."""
    ext = _ext()
    c = _case(S, masked, p)
    qkv, gout, mask = c["qkv"], c["gout"], c["mask"]
    state = _rng().state
    want = c["keep"].clone()
    if masked:
        want &= (mask == 0)[:, None, None, :]

    def fwd(x):
        return ext.flash_attn_drop_fwd(x, H, SCALE, mask, state, p, SITE)[0]

    def bwd(x, ctx, dctx, lse):
        return ext.flash_attn_drop_bwd(x, ctx, dctx, lse, SCALE, mask, state,
                                       p, SITE)

    assert torch.equal(ar.read_fwd_mask(fwd, qkv, mask), want)
    ctx, lse = ext.flash_attn_drop_fwd(qkv, H, SCALE, mask, state, p, SITE)
    assert torch.equal(ar.read_dkv_mask(bwd, qkv, ctx, lse, mask), want)
    got, left = ar.read_dq_mask(bwd, qkv, gout, mask)
    share = left.float().mean().item()
    print(f"S={S} p={p}: dQ read-out leaves out {share:.3e} of the elements")
    assert share == 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("S,masked", FLASH)
def test_flash_values(S, masked, p):
    ext, fx = _ext(), _fx()
    c = _case(S, masked, p)
    qkv, gout, mask = c["qkv"], c["gout"], c["mask"]
    rng = _rng()
    a = qkv.clone().requires_grad_()
    out = fx.flash_attention(a, H, SCALE, mask, p, rng, SITE)
    rng.tick()  # the Function holds its own copy of the state
    out.backward(gout)
    torch.cuda.synchronize()
    _check_values(f"flash S={S} masked={masked} p={p}", c, out.detach(), a.grad)
    # lse is the dropout-free kernel's, bit for bit
    state = _rng().state
    ctx, lse = ext.flash_attn_drop_fwd(qkv, H, SCALE, mask, state, p, SITE)
    _, lse0 = ext.flash_attn_fwd(qkv, H, SCALE, mask)
    assert torch.equal(ctx, out.detach())
    assert torch.equal(lse.view(torch.int32), lse0.view(torch.int32))
    # two backward calls are bit-equal, and equal to autograd's
    d1 = ext.flash_attn_drop_bwd(qkv, ctx, gout, lse, SCALE, mask, state, p, SITE)
    d2 = ext.flash_attn_drop_bwd(qkv, ctx, gout, lse, SCALE, mask, state, p, SITE)
    assert torch.equal(d1, d2) and torch.equal(d1, a.grad)
    if masked:
        assert (d1[1, S - 37:, 1:] == 0).all()
        assert (d1[0, :, 1:] != 0).any()


def test_bindings_reject_bad_arguments():
    ext = _ext()
    qkv = torch.zeros(1, 16, 3, 1, 64, dtype=torch.bfloat16, device=DEV)
    st = _rng().state
    for f in (ext.attn_drop_fwd, ext.flash_attn_drop_fwd):
        with pytest.raises(RuntimeError):
            f(qkv, 1, SCALE, None, st, 1.0, 0)            # p
        with pytest.raises(RuntimeError):
            f(qkv, 1, SCALE, None, st, 0.1, -1)           # site
        with pytest.raises(RuntimeError):
            f(qkv, 1, SCALE, None, st.cpu(), 0.1, 0)      # state on the CPU
        with pytest.raises(RuntimeError):
            f(qkv.float(), 1, SCALE, None, st, 0.1, 0)    # dtype
        with pytest.raises(RuntimeError):
            f(qkv, 2, SCALE, None, st, 0.1, 0)            # heads
    with pytest.raises(RuntimeError):                     # S != 128
        ext.attn_drop_bwd(qkv, torch.zeros(1, 16, 64, dtype=torch.bfloat16,
                                           device=DEV),
                          torch.zeros(1, 1, 16, 16, dtype=torch.bfloat16,
                                      device=DEV), SCALE, 0.1)


# --------------------------------------------------------------- graph capture
@pytest.mark.parametrize("path", ["saved_probs", "flash"])
def test_graph_replays_draw_fresh_masks(path):
    """tick + forward + backward captured once, replayed twice: the masks
    differ between replays and equal the reference at offsets +1 and +2."""
    fx = _fx()
    S, p = (128, 0.5) if path == "saved_probs" else (129, 0.5)
    c = _case(S, False, p)
    rng = _rng()
    # one-hot V, window 0: ctx[b, i, h, d] != 0 <=> keep[b, h, i, d]
    x = c["qkv"].clone()
    x[:, :, 2] = ar._onehot_rows(S, 0, DEV)[None, :, None, :]
    x.requires_grad_()
    op = fx.attention if path == "saved_probs" else fx.flash_attention

    def step():
        x.grad = None
        rng.tick()
        out = op(x, H, SCALE, None, p, rng, SITE)
        out.backward(c["gout"])
        return out

    step()  # eager warm-up; its autograd graph dies with the dropped output
    rng.set_state(SEED, OFFSET)
    x.grad = None
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    seen = []
    for k in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        got = (out.detach().reshape(B, S, H, D) != 0).permute(0, 2, 1, 3)
        assert torch.equal(got, _keep(S, p, OFFSET + k)[..., :D]), k
        # dV[b, j, h, d] = rs·sum_i P[i, j]·keep[i, j]·dO[i, d] of this replay
        assert torch.isfinite(x.grad.float()).all()
        seen.append((got.clone(), x.grad.clone()))
    assert not torch.equal(seen[0][0], seen[1][0])
    assert not torch.equal(seen[0][1], seen[1][1])
    assert rng.get_state() == (SEED, OFFSET + 2)


# ----------------------------------------------------------------------- model
def _tiny_bert(attn_dropout):
    from mpi_operator_amd.models import bert as Bm
    torch.manual_seed(5)
    cfg = Bm.BertConfig(vocab_size=512, hidden=128, layers=2, heads=2,
                        intermediate=256, max_seq=192,
                        attn_dropout=attn_dropout)
    m = Bm.to_mi355x_bert(Bm.BertForPreTraining(cfg), DEV)
    m.seed_dropout(SEED)
    return m


@pytest.mark.parametrize("S,pad", [(128, 0), (160, 23)])
def test_bert_with_attn_dropout(S, pad, monkeypatch):
    """S = 128 unmasked: Fx.attention with attn_bwd_k<true>; S = 160 with a
    padding mask: the flash kernels. Sites 1 + 2·layers + i = 5, 6."""
    fx = _fx()
    sites = []
    for name in ("attention", "flash_attention"):
        real = getattr(fx, name)

        def spy(*a, _real=real, _name=name, **kw):
            sites.append((_name, a[4], a[6]))
            return _real(*a, **kw)

        monkeypatch.setattr(fx, name, spy)
    m = _tiny_bert(0.1)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, 512, (2, S), generator=g).to(DEV)
    labels = ids.clone()
    nsp = torch.tensor([0, 1], device=DEV)
    am = None
    if pad:
        am = torch.ones(2, S, device=DEV)
        am[1, S - pad:] = 0
    m.train()
    losses, grads = [], []
    for _ in range(2):
        m.zero_grad()
        loss = m(ids, attn_mask=am, mlm_labels=labels, nsp_labels=nsp)
        loss.backward()
        w = m.bert.layers[0].attn.qkv.weight.grad
        assert torch.isfinite(loss) and torch.isfinite(w.float()).all()
        losses.append(loss.item())
        grads.append(w.clone())
    want = "flash_attention" if pad else "attention"
    assert sites == [(want, 0.1, 5), (want, 0.1, 6)] * 2, sites
    assert losses[0] != losses[1] and not torch.equal(grads[0], grads[1])
    del sites[:]
    m.eval()
    m0 = _tiny_bert(0.0).eval()
    with torch.no_grad():
        y, y0 = m(ids, attn_mask=am), m0(ids, attn_mask=am)
    assert all(s[1] == 0 for s in sites), sites
    assert torch.equal(y[0], y0[0]) and torch.equal(y[1], y0[1])
