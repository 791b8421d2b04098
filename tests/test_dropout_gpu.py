"""The dropout kernels on the GPU (csrc/dropout.hip, the *_drop* kernels of
csrc/layernorm.hip) against the CPU Philox reference, bit for bit, and
against fp64 with the bounds of dropout_refs.py / stream_refs.py.

Shapes (M, N), the smallest at which each code path can go wrong:
  (37, 256)    runtime C8 = 32 under 64 lanes; M no multiple of the 4 waves
  (133, 768)   C8 = 96: lanes 32-63 own one octet, lanes 0-31 two
  (37, 1536)   three octets per lane: the third misses the register cache
  (5, 2048)    ln_bwd's maximum: one row per block in the dgamma partials
  (4101, 1024) C8 = 128; the row loop repeats past the 1024 x 4-wave grid
"""
import pytest
import torch

import dropout_refs as dr
from stream_refs import REL_BF16, REL_F32, assert_close, assert_equal, rand_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, OFFSET, SITE = 0x1234_5678_9abc_def1, (3 << 32) + 7, 3
EPS = 1e-12
SHAPES = [(37, 256), (133, 768), (37, 1536), (5, 2048), (4101, 1024)]
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


def _rng(seed=SEED, offset=OFFSET):
    rng = _fx().DropoutRng(seed, DEV)
    rng.set_state(seed, offset)
    return rng


_CASES = {}


def case(M, N, p):
    """Inputs, the CPU reference mask and the fused forward + backward of one
    (shape, p), computed once and shared by the tests below (read-only)."""
    key = (M, N, p)
    if key in _CASES:
        return _CASES[key]
    ext = _ext()
    a = rand_bf16((M, N), 11, 1.0, 0.25, DEV)
    b = rand_bf16((M, N), 12, 2.0, -0.5, DEV)
    dy = rand_bf16((M, N), 13, 1.0, 0.0, DEV)
    gamma = (torch.rand(N, generator=torch.Generator().manual_seed(14)) + 0.5).to(DEV)
    beta = (torch.rand(N, generator=torch.Generator().manual_seed(15)) - 0.5).to(DEV)
    rng = _rng()
    y, s, mean, rstd, mask = ext.layernorm_drop_add_fwd(
        a, b, gamma, beta, EPS, rng.state, p, SITE)
    da, db, dgamma, dbeta = ext.layernorm_drop_add_bwd(
        dy, s, gamma, mean, rstd, mask, p)
    torch.cuda.synchronize()
    keep_ref = _ref().philox_dropout_mask(SEED, OFFSET, SITE, (M, N), p).to(DEV)
    c = dict(a=a, b=b, dy=dy, gamma=gamma, beta=beta, y=y, s=s, mean=mean,
             rstd=rstd, mask=mask, da=da, db=db, dgamma=dgamma, dbeta=dbeta,
             keep=keep_ref, scale=_ref().dropout_threshold(p)[2])
    _CASES[key] = c
    return c


# ------------------------------------------------------------------ 1. mask
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_fused_mask_matches_reference(M, N, p):
    c = case(M, N, p)
    assert c["mask"].dtype == torch.uint8 and tuple(c["mask"].shape) == (M, N // 8)
    assert_equal(dr.unpack_keep(c["mask"], (M, N)), c["keep"], f"mask[{M}x{N},p={p}]")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", SHAPES + [(3, 37, 24)])
def test_elementwise_mask_and_values(shape, p):
    ext = _ext()
    x = rand_bf16(shape, 21, 2.0, 0.0, DEV)
    y, mask = ext.dropout_fwd(x, _rng().state, p, SITE)
    n = x.numel()
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (n // 8,)
    keep = _ref().philox_dropout_mask(SEED, OFFSET, SITE, shape, p).to(DEV)
    assert_equal(dr.unpack_keep(mask, shape), keep, f"ew mask{shape}")
    scale = _ref().dropout_threshold(p)[2]
    # one fp32 multiply, one rounding to bf16: exact
    want = torch.where(keep, (x.float() * scale), torch.zeros((), device=DEV)).to(torch.bfloat16)
    assert_equal(y, want, f"ew y{shape}")
    dy = rand_bf16(shape, 22, 1.0, 0.0, DEV)
    dx = ext.dropout_bwd(dy, mask, p)
    want = torch.where(keep, (dy.float() * scale), torch.zeros((), device=DEV)).to(torch.bfloat16)
    assert_equal(dx, want, f"ew dx{shape}")


# ------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_fused_forward(M, N, p):
    c = case(M, N, p)
    tag = f"[{M}x{N},p={p}]"
    keep, s = c["keep"], c["s"]
    # dropped: a's bits pass through
    assert_equal(s[~keep], c["a"][~keep], "s_dropped" + tag)
    s_ref, s_abs = dr.drop_add_ref(c["a"], c["b"], keep, c["scale"])
    assert_close(s[keep], s_ref[keep], REL_BF16, s_abs[keep], "s_kept" + tag)
    r = dr.ln_fwd_ref(s, c["gamma"], c["beta"], EPS)
    assert_close(c["mean"], r["mean"], REL_F32, r["mean_abs"], "mean" + tag)
    assert_close(c["rstd"], r["rstd"], REL_F32, r["rstd_abs"], "rstd" + tag)
    assert_close(c["y"], r["y"], REL_BF16, r["y_abs"], "y" + tag)


# ------------------------------------------------------------------ 3. backward
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_fused_backward(M, N, p):
    c = case(M, N, p)
    tag = f"[{M}x{N},p={p}]"
    keep = c["keep"]
    dx0, dg0, db0 = _ext().layernorm_bwd(c["dy"], c["s"], c["gamma"], c["mean"],
                                         c["rstd"])
    assert_equal(c["da"], dx0, "da" + tag)
    assert_equal(c["dgamma"], dg0, "dgamma" + tag)
    assert_equal(c["dbeta"], db0, "dbeta" + tag)
    zero = torch.zeros_like(c["db"])
    assert_equal(c["db"][~keep], zero[~keep], "db_dropped" + tag)
    dx, dx_abs = dr.ln_bwd_dx_ref(c["dy"], c["s"], c["gamma"], c["mean"], c["rstd"])
    sc = c["scale"]
    assert_close(c["da"], dx, REL_BF16, dx_abs, "da_fp64" + tag)
    assert_close(c["db"][keep], (dx * sc)[keep], REL_BF16,
                 (dx_abs * sc + REL_F32 * (dx * sc).abs())[keep], "db_kept" + tag)


DIGEST_OUTPUTS = ("y", "s", "mean", "rstd", "mask", "da", "db", "dgamma", "dbeta")


def digests():
    """{'MxN,p': sha256 of every output of the fused forward and backward}.
    tests/test_dropout_knobs_gpu.py compares these across MPIAMD_LN_SPEC and
    MPIAMD_LN2: the results must not depend on either."""
    import hashlib
    out = {}
    for M, N in SHAPES:
        for p in PS:
            c = case(M, N, p)
            h = hashlib.sha256()
            for name in DIGEST_OUTPUTS:
                h.update(c[name].contiguous().view(torch.uint8).cpu().numpy().tobytes())
            out[f"{M}x{N},{p}"] = h.hexdigest()
    return out


def test_print_digests():
    for k, v in digests().items():
        print(f"\nDIGEST {k} {v}")  # at a line start under -s


# ------------------------------------------------------------------ 4. p == 0
def test_p_zero_is_layer_norm_add():
    Fx = _fx()
    M, N = 37, 256
    a0, b0 = rand_bf16((M, N), 31, 1.0, 0.0, DEV), rand_bf16((M, N), 32, 1.0, 0.0, DEV)
    dy = rand_bf16((M, N), 33, 1.0, 0.0, DEV)
    w0 = torch.rand(N, device=DEV) + 0.5
    bb0 = torch.rand(N, device=DEV) - 0.5

    def run(fn):
        ts = [t.clone().requires_grad_(True) for t in (a0, b0, w0, bb0)]
        y = fn(*ts)
        y.backward(dy)
        return [y.detach()] + [t.grad for t in ts]

    got = run(lambda a, b, w, bb: Fx.layer_norm_drop_add(a, b, w, bb, EPS, 0.0, None, 5))
    want = run(lambda a, b, w, bb: Fx.layer_norm_add(a, b, w, bb, EPS))
    for g, w, name in zip(got, want, ("y", "da", "db", "dgamma", "dbeta")):
        assert_equal(g, w, "p0 " + name)
    x = a0.clone().requires_grad_(True)
    assert Fx.dropout(x, 0.0, None, 0) is x


def test_autograd_functions_match_bindings():
    """Fx.layer_norm_drop_add / Fx.dropout route forward and backward to the
    kernels checked above."""
    Fx = _fx()
    M, N, p = 37, 256, 0.5
    c = case(M, N, p)
    a, b = c["a"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
    w, bb = c["gamma"].clone().requires_grad_(True), c["beta"].clone().requires_grad_(True)
    y, mask = Fx.layer_norm_drop_add_with_mask(a, b, w, bb, EPS, p, _rng(), SITE)
    y.backward(c["dy"])
    for got, name in ((y.detach(), "y"), (mask, "mask"), (a.grad, "da"), (b.grad, "db"),
                      (w.grad, "dgamma"), (bb.grad, "dbeta")):
        assert_equal(got, c[name], "fn " + name)
    x = c["b"].clone().requires_grad_(True)
    out = Fx.dropout(x, p, _rng(), SITE)
    out.backward(c["dy"])
    y2, m2 = _ext().dropout_fwd(c["b"], _rng().state, p, SITE)
    assert_equal(out.detach(), y2, "fn dropout y")
    assert_equal(x.grad, _ext().dropout_bwd(c["dy"], m2, p), "fn dropout dx")


# ------------------------------------------------------------------ 5. graph replay
def test_graph_replay_draws_fresh_masks():
    ext = _ext()
    M, N, p = 37, 256, 0.5
    c = case(M, N, p)
    rng = _rng()
    rng.tick()  # warm both kernels outside capture
    ext.layernorm_drop_add_fwd(c["a"], c["b"], c["gamma"], c["beta"], EPS, rng.state, p, SITE)
    rng.set_state(SEED, OFFSET)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, no parallel branches
        rng.tick()
        out = ext.layernorm_drop_add_fwd(c["a"], c["b"], c["gamma"], c["beta"], EPS,
                                         rng.state, p, SITE)
    assert rng.get_state() == (SEED, OFFSET)  # capture records, runs nothing
    seen = []
    for k in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        keep = _ref().philox_dropout_mask(SEED, OFFSET + k, SITE, (M, N), p).to(DEV)
        assert_equal(dr.unpack_keep(out[4], (M, N)), keep, f"replay {k}")
        seen.append(out[4].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert rng.get_state() == (SEED, OFFSET + 3)


def test_get_state_refuses_capture():
    rng = _rng()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rng.tick()
        with pytest.raises(RuntimeError, match="capture"):
            rng.get_state()


# ------------------------------------------------------------------ 6. determinism
def test_set_state_reproduces_bits():
    ext = _ext()
    M, N, p = 133, 768, 0.1
    c = case(M, N, p)
    rng = _rng(5, 0)
    rng.tick()
    rng.tick()
    assert rng.get_state() == (5, 2)
    rng.set_state(SEED, OFFSET)
    assert rng.get_state() == (SEED, OFFSET)
    out = ext.layernorm_drop_add_fwd(c["a"], c["b"], c["gamma"], c["beta"], EPS,
                                     rng.state, p, SITE)
    for got, name in zip(out, ("y", "s", "mean", "rstd", "mask")):
        assert_equal(got, c[name], "again " + name)
    other = ext.layernorm_drop_add_fwd(c["a"], c["b"], c["gamma"], c["beta"], EPS,
                                       rng.state, p, SITE + 1)
    assert not torch.equal(other[4], c["mask"])


# ------------------------------------------------------------------ 7. arguments
def test_bad_arguments_raise_before_launch():
    ext = _ext()
    c = case(37, 256, 0.5)
    a, b, g, bt = c["a"], c["b"], c["gamma"], c["beta"]
    st = _rng().state
    err = (RuntimeError, ValueError)
    odd = torch.zeros(4, 12, device=DEV, dtype=torch.bfloat16)  # N % 8 != 0
    with pytest.raises(err):
        ext.layernorm_drop_add_fwd(odd, odd, g[:12].contiguous(), bt[:12].contiguous(),
                                   EPS, st, 0.5, 0)
    with pytest.raises(err):
        ext.dropout_fwd(torch.zeros(3, 7, device=DEV, dtype=torch.bfloat16), st, 0.5, 0)
    with pytest.raises(err):  # wrong mask shape
        ext.layernorm_drop_add_bwd(c["dy"], c["s"], g, c["mean"], c["rstd"],
                                   c["mask"].reshape(-1), 0.5)
    with pytest.raises(err):
        ext.layernorm_drop_add_bwd(c["dy"], c["s"], g, c["mean"], c["rstd"],
                                   c["mask"][:, :-1].contiguous(), 0.5)
    with pytest.raises(err):
        ext.dropout_bwd(c["dy"], c["mask"].reshape(-1)[:-1].contiguous(), 0.5)
    with pytest.raises(err):  # state of another dtype / size
        ext.layernorm_drop_add_fwd(a, b, g, bt, EPS, st.to(torch.int32), 0.5, 0)
    with pytest.raises(err):
        ext.dropout_fwd(a, st.float(), 0.5, 0)
    with pytest.raises(err):
        ext.rng_tick(torch.zeros(3, device=DEV, dtype=torch.int64))
    with pytest.raises(err):  # CPU tensors
        ext.layernorm_drop_add_fwd(a.cpu(), b.cpu(), g.cpu(), bt.cpu(), EPS, st, 0.5, 0)
    with pytest.raises(err):
        ext.layernorm_drop_add_fwd(a, b, g, bt, EPS, st.cpu(), 0.5, 0)
    with pytest.raises(err):
        ext.dropout_fwd(a.cpu(), st, 0.5, 0)
    with pytest.raises(err):
        ext.rng_tick(st.cpu())
    wide = torch.zeros(2, 2056, device=DEV, dtype=torch.bfloat16)  # N > 2048
    with pytest.raises(err):
        ext.layernorm_drop_add_bwd(wide, wide, torch.ones(2056, device=DEV),
                                   torch.zeros(2, device=DEV), torch.ones(2, device=DEV),
                                   torch.zeros(2, 257, device=DEV, dtype=torch.uint8), 0.5)
    for p in (1.0, -0.1):
        with pytest.raises(err):
            ext.dropout_fwd(a, st, p, 0)
        with pytest.raises(ValueError):
            _fx().dropout(a, p, _rng(), 0)
    with pytest.raises(err):
        ext.dropout_fwd(a, st, 0.5, -1)  # site must fit a uint32


# ------------------------------------------------------------------ 8. model
def _tiny_model(dropout, seed=2):
    from mpi_operator_amd.models.bert import (BertConfig, BertForPreTraining,
                                              to_mi355x_bert)
    torch.manual_seed(seed)
    cfg = BertConfig(hidden=512, layers=1, heads=8, intermediate=2048, dropout=dropout)
    return to_mi355x_bert(BertForPreTraining(cfg), DEV)


def _batch(m, b=2, s=64):
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, m.cfg.vocab_size, (b, s), generator=g).to(DEV)
    nsp = torch.randint(0, 2, (b,), generator=g).to(DEV)
    return ids, ids.clone(), nsp


def test_model_train_losses_differ_and_eval_is_dropout_free():
    m = _tiny_model(0.1)
    m0 = _tiny_model(0.0)
    m0.load_state_dict(m.state_dict())
    ids, labels, nsp = _batch(m)
    m.train()
    m.seed_dropout(3)
    with torch.no_grad():
        l1 = m(ids, mlm_labels=labels, nsp_labels=nsp).item()
        l2 = m(ids, mlm_labels=labels, nsp_labels=nsp).item()
    assert l1 != l2, (l1, l2)
    assert m.bert._dropout_rng.get_state() == (3, 2)  # one tick per forward
    # re-seeding restarts the mask sequence (compared on the trunk's output:
    # the loss itself is summed with atomics and varies in its last bits)
    with torch.no_grad():
        m.seed_dropout(3)
        h1 = m.bert(ids)
        h2 = m.bert(ids)
        m.seed_dropout(3)
        h1b = m.bert(ids)
    assert not torch.equal(h1, h2)
    assert_equal(h1b, h1, "trunk after re-seed")
    m.eval()
    m0.eval()
    with torch.no_grad():
        a, an = m(ids)
        b, bn = m0(ids)
    assert_equal(a, b, "eval mlm logits")
    assert_equal(an, bn, "eval nsp logits")
    assert list(m.state_dict()) == list(m0.state_dict())


def test_model_rng_created_under_capture_raises():
    m = _tiny_model(0.1)
    ids, labels, nsp = _batch(m)
    m.train()
    t = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.add_(1.0)
        # raised ahead of the forward's first kernel
        with pytest.raises(RuntimeError, match="run one eager step first"):
            m(ids)
    assert m.bert._dropout_rng is None


def test_model_captured_step_draws_fresh_masks():
    from mpi_operator_amd.optim import FusedSGD
    m = _tiny_model(0.1)
    ids, labels, nsp = _batch(m)
    m.train()
    m.seed_dropout(4)
    opt = FusedSGD(m.parameters(), lr=0.0, momentum=0.9)

    def step():
        opt.zero_grad()
        loss = m(ids, mlm_labels=labels, nsp_labels=nsp)
        loss.backward()
        opt.step()
        return loss

    for _ in range(2):
        loss = step()
    loss = None  # no live autograd graph from the eager stream at capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = step()
    losses = []
    for _ in range(5):
        g.replay()
        torch.cuda.synchronize()
        losses.append(float(loss.detach()))
    print("replayed losses", losses)
    assert all(l == l for l in losses), losses
    assert len(set(losses)) > 1, losses
    assert m.bert._dropout_rng.get_state() == (4, 2 + 5)


def test_model_adamw_lowers_loss_with_dropout():
    from mpi_operator_amd.models.bert import bert_param_groups
    from mpi_operator_amd.optim import FusedAdamW
    m = _tiny_model(0.1)
    ids, labels, nsp = _batch(m)
    m.train()
    m.seed_dropout(5)
    opt = FusedAdamW(bert_param_groups(m, 0.01), lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = m(ids, mlm_labels=labels, nsp_labels=nsp)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("adamw losses", losses[0], losses[-1])
    assert all(l == l for l in losses), losses
    assert losses[-1] < losses[0], losses
