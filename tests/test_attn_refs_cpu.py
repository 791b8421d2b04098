"""The attention edge harness itself (attn_refs.py), without a GPU: an fp32
emulation of the flash kernels' roundings passes every bound, each of nine
deliberately wrong emulations misses at least one, the 0.97-scaled dQ that the
bounds catch passes the suite's previous criterion, and the input families
and masks do what they are for.

The emulation walks the keys in 128-wide tiles with an online softmax in fp32
(running max from the finite floor, alpha = exp(m_old - m_new)), parks the
unnormalized bf16(exp(s - m)) for P·V while l sums the fp32 values, rounds ctx
to bf16, and in the backward rounds P, dS and the three outputs to bf16.
Worst error / bound ratio of the correct emulation over the 32 pass-side
cases: ctx 0.82, dq 0.81, dk 0.86, dv 0.91, lse below 0.2."""
import pytest
import torch

import attn_refs as ar

B, H, S = 2, 3, 296
bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731


def _qkv32(qkv):
    return (qkv[:, :, i].transpose(1, 2).float() for i in range(3))


def _vis_add(qkv, mask, causal, off1=False, drop_key=None, let_in=False):
    B_, S_, _, H_, _ = qkv.shape
    vis = ar.visible(mask, B_, S_, causal).expand(B_, H_, S_, S_).clone()
    if off1:  # j <= i + 1
        vis = ar.visible(mask, B_, S_, False) & torch.ones(
            S_, S_, dtype=torch.bool).tril(1)
        vis = vis.expand(B_, H_, S_, S_).clone()
    add = torch.zeros(B_, S_)
    if mask is not None:
        add = torch.where(mask > ar.VISIBLE_ABOVE, mask, add)
    if drop_key is not None:
        vis[..., drop_key] = False
    if let_in:  # the first masked key of batch row 0, with its real score
        jm = int((mask[0] <= ar.VISIBLE_ABOVE).nonzero()[0])
        tri = torch.ones(S_, S_, dtype=torch.bool).tril()[:, jm] if causal \
            else torch.ones(S_, dtype=torch.bool)
        vis[0, :, :, jm] = tri
    return vis, add[:, None, None, :]


def emu_fwd(qkv, scale, mask, causal, bug=None):
    """(ctx bf16 [B,S,H·D], lse fp32 [B,H,S]) of the emulated forward."""
    B_, S_, _, H_, D = qkv.shape
    q, k, v = _qkv32(qkv)
    vis, add = _vis_add(qkv, mask, causal, off1=bug == "fwd_off1",
                        drop_key=128 if bug == "drop_key_128" else None,
                        let_in=bug == "masked_key_in")
    s = torch.matmul(q, k.transpose(-1, -2)) * scale + add
    floor = torch.tensor(ar.FLOOR)
    m = torch.full((B_, H_, S_), ar.FLOOR)
    l = torch.zeros(B_, H_, S_)
    o = torch.zeros(B_, H_, S_, D)
    for t, k0 in enumerate(range(0, S_, 128)):
        sl = slice(k0, min(k0 + 128, S_))
        st = torch.where(vis[..., sl], s[..., sl], floor)
        m_new = torch.maximum(m, st.amax(-1))
        alpha = (m - m_new).exp()
        e = torch.where(vis[..., sl], (st - m_new[..., None]).exp(),
                        torch.zeros(()))
        l = (l if bug == "l_norescale" and t == 1 else l * alpha) + e.sum(-1)
        o = (o if bug == "o_norescale" and t == 1 else o * alpha[..., None]) \
            + torch.matmul(bf(e), v[:, :, sl])
        m = m_new
    inv = torch.where(l > 0, 1 / l, torch.zeros(()))
    ctx = (o * inv[..., None]).transpose(1, 2).reshape(B_, S_, H_ * D)
    lse = torch.where(l > 0, m + l.log(), m)
    if bug == "lse_bf16":
        lse = torch.logsumexp(bf(s).masked_fill(~vis, float("-inf")), -1)
    return ctx.to(torch.bfloat16), lse


def emu_bwd(qkv, gout, ctx, lse, scale, mask, causal, bug=None):
    """dqkv bf16 [B,S,3,H,D] of the emulated backward on (ctx, lse)."""
    B_, S_, _, H_, D = qkv.shape
    q, k, v = _qkv32(qkv)
    vis, add = _vis_add(qkv, mask, causal, off1=bug == "bwd_off1")
    s = torch.matmul(q, k.transpose(-1, -2)) * scale + add
    p = torch.where(vis, (s - lse[..., None]).exp(), torch.zeros(()))
    do = gout.reshape(B_, S_, H_, D).transpose(1, 2).float()
    o = ctx.reshape(B_, S_, H_, D).transpose(1, 2).float()
    delta = (do * o).sum(-1, keepdim=True)
    ds = (torch.matmul(do, v.transpose(-1, -2)) - delta) * p * scale
    pb, dsb = bf(p), bf(ds)
    dv = torch.matmul(pb.transpose(-1, -2), do)
    dq = torch.matmul(dsb, k) * (0.97 if bug == "dq_097" else 1.0)
    dk = torch.matmul(dsb.transpose(-1, -2), q) * (0.97 if bug == "dk_097" else 1.0)
    return torch.stack([t.transpose(1, 2) for t in (dq, dk, dv)],
                       dim=2).to(torch.bfloat16)


def _run(family, D, causal, kind, bug=None, value=ar.FMIN):
    qkv, gout = ar.inputs(family, B, H, S, D)
    mask = ar.key_mask(kind, S, value) if kind else None
    sc = ar.scale_of(D)
    ctx, lse = emu_fwd(qkv, sc, mask, causal, bug)
    dqkv = emu_bwd(qkv, gout, ctx, lse, sc, mask, causal, bug)
    tag = f"emu[{family}-D{D}-c{int(causal)}-{kind}-{bug}]"
    res, f = ar.check_flash(tag, family, qkv, gout, sc, mask, causal, ctx, lse,
                            dqkv)
    return res, f, (ctx, lse, dqkv)


# ------------------------------------------------------------- pass side
_worst = {}


@pytest.mark.parametrize("kind", ["hole", "head"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("D", [64, 128])
def test_emulation_passes_every_bound(D, family, causal, kind):
    res, f, _ = _run(family, D, causal, kind)
    assert [n for n, *_ in res] == ["ctx", "lse", "dq", "dk", "dv"]
    for n, ok, worst, msg in res:
        _worst[n] = max(_worst.get(n, 0.0), worst)
        print(msg)
        assert ok and worst < 1, msg
    print("worst ratios so far:", {n: round(w, 3) for n, w in _worst.items()})
    assert f["small"]  # |s| <= 32: the lse bound is the capped one
    assert float(f["lse_abs"].max()) < ar.LSE_CAP + 1e-12


# ------------------------------------------------------------- fail side
# bug -> the case it is run on: (family, causal, mask kind)
BUGS = {
    "dq_097": ("sharp", False, None),
    "dk_097": ("sharp", False, None),
    "o_norescale": ("ramp_up", False, None),
    "l_norescale": ("ramp_up", False, None),
    "fwd_off1": ("sharp", True, None),
    "bwd_off1": ("sharp", True, None),
    "drop_key_128": ("sharp", False, None),
    "masked_key_in": ("sharp", False, "hole"),
    "lse_bf16": ("sharp", False, None),
}


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("bug", sorted(BUGS))
def test_wrong_emulation_misses_a_bound(bug, D):
    family, causal, kind = BUGS[bug]
    good, _, _ = _run(family, D, causal, kind)
    assert all(ok for _, ok, _, _ in good), good
    res, _, _ = _run(family, D, causal, kind, bug)
    missed = [n for n, ok, _, _ in res if not ok]
    print(bug, D, "misses", missed, [round(w, 2) for _, _, w, _ in res])
    assert missed, f"{bug} at D={D} passes every bound"
    if bug in ("dq_097", "dk_097"):
        assert missed == [bug[:2]]
    if bug == "lse_bf16":
        assert missed == ["lse"]


def _autograd64(qkv, gout, scale, causal):
    B_, S_, _, H_, D = qkv.shape
    r = qkv.double().requires_grad_()
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(torch.ones(S_, S_, dtype=torch.bool).triu(1),
                          float("-inf"))
    out = torch.matmul(torch.softmax(s, -1), v).transpose(1, 2)
    out = out.reshape(B_, S_, H_ * D)
    out.backward(gout.double())
    return out.detach(), r.grad


@pytest.mark.parametrize("causal", [False, True])
def test_previous_criterion_passes_a_scaled_dq(causal):
    """The gap on record: ferr < 0.02 and gerr < 0.08·max|ref dqkv| + 2e-3
    (one max over dq, dk and dv) accept a dQ that is 3 % off everywhere, on
    the inputs those tests use; the per-gradient bounds do not."""
    qkv, gout = ar.inputs("soft", B, H, S, 64)
    sc = ar.scale_of(64)
    ctx, lse = emu_fwd(qkv, sc, None, causal)
    dqkv = emu_bwd(qkv, gout, ctx, lse, sc, None, causal, "dq_097")
    out_r, grad_r = _autograd64(qkv, gout, sc, causal)
    ferr = (ctx.double() - out_r).abs().max().item()
    gerr = (dqkv.double() - grad_r).abs().max().item()
    gmax = grad_r.abs().max().item()
    print(f"causal={causal}: ferr {ferr:.3e} gerr {gerr:.3e} gmax {gmax:.3e}")
    assert ferr < 0.02 and gerr < 0.08 * gmax + 2e-3
    res, _ = ar.check_flash("scaled", "soft", qkv, gout, sc, None, causal,
                            ctx, lse, dqkv)
    assert [n for n, ok, _, _ in res if not ok] == ["dq"]


# ------------------------------------------------- inputs, masks, coverage
@pytest.mark.parametrize("D", [64, 128])
def test_ramps_move_the_running_max(D):
    """ramp_up: every row's maximum over key tile t+1 exceeds that over tile
    t by at least 2 (alpha <= e^-2 at both tile boundaries); ramp_down the
    mirror; |s| <= 32 in every family."""
    sc = ar.scale_of(D)
    assert sc * 4 * ar.RAMP_A[D] >= 8
    for family in ar.FAMILIES:
        qkv, _ = ar.inputs(family, B, H, S, D)
        q, k, _ = (qkv[:, :, i].transpose(1, 2).double() for i in range(3))
        s = torch.matmul(q, k.transpose(-1, -2)) * sc
        assert float(s.abs().max()) <= 32, (family, float(s.abs().max()))
        t = [s[..., a:a + 128].amax(-1) for a in (0, 128, 256)]
        if family == "ramp_up":
            assert float((t[1] - t[0]).min()) >= 2 and float((t[2] - t[1]).min()) >= 2
            # exact in bf16: the stored values are the ramp as drawn
            assert (qkv[:, :, 0, :, 0] == 4).all()
        elif family == "ramp_down":
            assert float((t[0] - t[1]).min()) >= 2 and float((t[1] - t[2]).min()) >= 2
        elif family == "sharp":
            assert 3 < float(s.std()) < 5
        else:
            assert float(s.std()) < 0.4


def test_soft_is_the_existing_draw():
    import attn_dropout_refs as old
    qkv, gout = ar.inputs("soft", B, H, S, 64)
    q0, g0 = old.inputs(B, H, S, "cpu")
    assert torch.equal(qkv, q0) and torch.equal(gout, g0)


def test_masks_and_empty_rows():
    for kind in ar.MASK_KINDS:
        m = ar.key_mask(kind, S, ar.FMIN)
        assert m.shape == (B, S) and not torch.equal(m[0], m[1]), kind
        assert (m[:, 0] != 0).any() == (kind in ("head", "empty"))
    assert (ar.key_mask("head", S, ar.FMIN)[:, :130] == ar.FMIN).all()
    assert (ar.key_mask("tile", S, ar.FMIN)[:, 128:256] == ar.FMIN).all()
    hole = ar.key_mask("hole", S, ar.FMIN)[0]
    assert hole[99] == 0 and hole[100] != 0 and hole[139] != 0 and hole[140] == 0
    assert (hole[-6:] != 0).all() and hole[-7] == 0
    # rows with no visible key: the empty batch row, and the first 130 rows
    # of a causal call under the head mask
    e = ~ar.visible(ar.key_mask("empty", S, ar.FMIN), B, S, False).any(-1)
    assert e[1].all() and not e[0].any()
    e = ~ar.visible(ar.key_mask("head", S, ar.FMIN), B, S, True).any(-1)
    assert e[:, 0, :130].all() and not e[:, 0, 130:].any()
    # -10000 is added, not excluded
    assert ar.visible(ar.key_mask("empty", S, -10000.0), B, S, False).all()
    assert not ar.visible(ar.key_mask("empty", S, float("-inf")), B, S, False)[1].any()


def test_empty_rows_are_pinned():
    """ctx = 0, lse = FLOOR to the bit, dq = 0, and a masked key's dK / dV
    row is exactly 0: a bound of 0, so any other value fails."""
    res, f, (ctx, lse, dqkv) = _run("sharp", 64, True, "head")
    assert all(ok for _, ok, _, _ in res)
    e = f["empty"]
    assert e.any() and (lse[e] == ar.FLOOR).all() and (f["lse_abs"][e] == 0).all()
    assert not ctx[:, :130].any() and not dqkv[:, :130].any()
    lse2 = lse.clone()
    lse2[0, 0, 5] = 0.0
    bad, _ = ar.check_flash("x", "sharp", *_case64_head(), ctx, lse2, dqkv)
    assert not dict((n, ok) for n, ok, _, _ in bad)["lse"]


def _case64_head():
    qkv, gout = ar.inputs("sharp", B, H, S, 64)
    return qkv, gout, ar.scale_of(64), ar.key_mask("head", S, ar.FMIN), True


@pytest.mark.parametrize("name", ["ctx", "lse", "dq", "dk", "dv"])
def test_no_element_is_left_out(name):
    """One wrong element, first or last of the tensor, fails its output and
    no other: nothing is skipped and no worst-k is forgiven."""
    qkv, gout = ar.inputs("sharp", B, H, S, 64)
    sc, mask = ar.scale_of(64), ar.key_mask("hole", S, ar.FMIN)
    ctx, lse = emu_fwd(qkv, sc, mask, False)
    dqkv = emu_bwd(qkv, gout, ctx, lse, sc, mask, False)
    for pos in (0, -1):
        c, l, d = ctx.clone(), lse.clone(), dqkv.clone()
        if name == "ctx":
            c.view(-1)[pos] += 1.0
            # the backward is checked on the kernel's own ctx, so it is run
            # again on the corrupted one
            d = emu_bwd(qkv, gout, c, l, sc, mask, False)
        elif name == "lse":
            l.view(-1)[pos] += 0.01
            d = emu_bwd(qkv, gout, c, l, sc, mask, False)
        else:
            part = d[:, :, "dq dk dv".split().index(name[:2])]
            part[0 if pos == 0 else -1, pos, pos, pos] += 1.0
        res, _ = ar.check_flash("one", "sharp", qkv, gout, sc, mask, False,
                                c, l, d)
        assert [n for n, ok, _, _ in res if not ok] == [name], (pos, res)
