"""FusedAdamW / FusedLAMB on the HIP kernels (csrc/optimizer.hip).

Oracle: the same update in fp64 on the CPU from the identical (already
rounded) grads. Tolerance: in the same test the max-abs error of an fp32
torch run on the GPU against that oracle is measured — torch.optim.AdamW /
Adam for Adam, the LAMB formulas in fp32 torch ops for LAMB — and the
kernel's fp32 masters must be within 4x of it (operation-order differences;
a wrong bias correction or eps placement is off by > 1e-4). bf16 working
copies must equal master.to(bfloat16) bit for bit.

Tensor sizes are the smallest that reach every kernel path: numel < 8, one
element short of a block, exactly one interior block, interior + 1-element
tail, a per-tensor reduce across several blocks, and more than 40 tensors per
grad dtype (crosses the kernarg chunk), with bf16 and fp32 params mixed in
one group."""
import math

import pytest
import torch

from mpi_operator_amd import ops
from mpi_operator_amd.ops import reference as ref
from mpi_operator_amd.optim import FusedAdamW, FusedLAMB

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPB = 8192
F32, BF16 = torch.float32, torch.bfloat16
SIZES = [3, EPB - 1, EPB, EPB + 1, 3 * EPB + 5]
SPECS = ([(n, dt) for n in SIZES for dt in (F32, BF16)]
         + [(64, BF16)] * 45 + [(64, F32)] * 45)
LR, BETAS = 1e-2, (0.9, 0.999)


def _make(seed, steps, specs=SPECS, wscale=0.43, gscale=1.0):
    """Weights uniform in +-wscale and `steps` lists of grads, each already
    rounded to its param dtype. A per-tensor wscale/gscale list is allowed."""
    g = torch.Generator().manual_seed(seed)
    ws_ = wscale if isinstance(wscale, (list, tuple)) else [wscale] * len(specs)
    gs_ = gscale if isinstance(gscale, (list, tuple)) else [gscale] * len(specs)
    ws = [((torch.rand(n, generator=g) * 2 - 1) * s).to(dt)
          for (n, dt), s in zip(specs, ws_)]
    grads = [[(torch.randn(n, generator=g) * s).to(dt) for (n, dt), s in zip(specs, gs_)]
             for _ in range(steps)]
    return ws, grads


class Oracle:
    """fp64 CPU Adam / LAMB from the formulas."""

    def __init__(self, ws, kind, lr=LR, betas=BETAS, eps=None, wd=0.01,
                 adam_w_mode=True, max_grad_norm=None):
        self.kind, self.lr, self.betas, self.wd = kind, lr, betas, wd
        self.eps = eps if eps is not None else (1e-8 if kind == "adam" else 1e-6)
        self.adam_w_mode, self.max_grad_norm = adam_w_mode, max_grad_norm
        self.w = [w.double().cpu().clone() for w in ws]
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.t = 0

    def step(self, grads):
        self.t += 1
        b1, b2 = self.betas
        lr, wd, eps = self.lr, self.wd, self.eps
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        gs = [g.double().cpu() for g in grads]
        clip = 1.0
        if self.max_grad_norm is not None:  # clip_grad_norm_ semantics
            norm = math.sqrt(sum(float((g * g).sum()) for g in gs))
            clip = min(1.0, self.max_grad_norm / (norm + 1e-6))
        for i, g in enumerate(gs):
            g = g * clip
            w = self.w[i]
            if self.kind == "adam":
                if self.adam_w_mode:
                    w = w * (1 - lr * wd)
                else:
                    g = g + wd * w
            elif not self.adam_w_mode:
                g = g + wd * w
            m = self.m[i] = b1 * self.m[i] + (1 - b1) * g
            v = self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            if self.kind == "adam":
                w = w - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
            else:
                u = (m / bc1) / ((v / bc2).sqrt() + eps)
                if self.adam_w_mode:
                    u = u + wd * w
                nw, nu = float(w.norm()), float(u.norm())
                ratio = nw / nu if (nw > 0 and nu > 0) else 1.0
                w = w - lr * ratio * u
            self.w[i] = w


def _torch_adam_fp32(ws, grads_per_step, lrs, wd, adam_w_mode, max_grad_norm=None):
    """fp32 torch.optim.AdamW / Adam on the GPU from the same grads."""
    ps = [torch.nn.Parameter(w.float().to(DEV)) for w in ws]
    cls = torch.optim.AdamW if adam_w_mode else torch.optim.Adam
    opt = cls(ps, lr=lrs[0], betas=BETAS, eps=1e-8, weight_decay=wd)
    for lr, grads in zip(lrs, grads_per_step):
        opt.param_groups[0]["lr"] = lr
        for p, g in zip(ps, grads):
            p.grad = g.float().to(DEV)
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_grad_norm)
        opt.step()
    return [p.detach() for p in ps]


def _lamb_fp32(ws, grads_per_step, lrs, wd, adam_w_mode, eps=1e-6):
    """The LAMB formulas in fp32 torch ops on the GPU."""
    b1, b2 = BETAS
    w = [x.float().to(DEV) for x in ws]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    for t, (lr, grads) in enumerate(zip(lrs, grads_per_step), 1):
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        for i, g in enumerate(grads):
            g = g.float().to(DEV)
            if not adam_w_mode:
                g = g + wd * w[i]
            m[i] = b1 * m[i] + (1 - b1) * g
            v[i] = b2 * v[i] + (1 - b2) * g * g
            u = (m[i] / bc1) / ((v[i] / bc2).sqrt() + eps)
            if adam_w_mode:
                u = u + wd * w[i]
            nw, nu = w[i].norm(), u.norm()
            ratio = torch.where((nw > 0) & (nu > 0), nw / nu, torch.ones_like(nw))
            w[i] = w[i] - lr * ratio * u
    return w


def _fp32_ref(kind, ws, grads_per_step, lrs, wd, adam_w_mode, max_grad_norm=None):
    if kind == "adam":
        return _torch_adam_fp32(ws, grads_per_step, lrs, wd, adam_w_mode, max_grad_norm)
    assert max_grad_norm is None
    return _lamb_fp32(ws, grads_per_step, lrs, wd, adam_w_mode)


def _params(ws):
    return [torch.nn.Parameter(w.clone().to(DEV)) for w in ws]


def _masters(opt, params):
    return [opt.state[p]["master"] if p.dtype != F32 else p.data for p in params]


def _errs(tensors, oracle_w):
    return [float((t.double().cpu() - w).abs().max()) for t, w in zip(tensors, oracle_w)]


def _check(opt, params, ref_w, oracle, per_tensor=False):
    masters = _masters(opt, params)
    for mst in masters:
        assert torch.isfinite(mst).all()
    err, ref_err = _errs(masters, oracle.w), _errs(ref_w, oracle.w)
    print(f"kernel max err {max(err):.3e}  fp32 reference max err {max(ref_err):.3e}")
    assert max(ref_err) > 0
    if per_tensor:
        for i, (e, r) in enumerate(zip(err, ref_err)):
            assert e <= 4 * r, (i, e, r)
    assert max(err) <= 4 * max(ref_err), (max(err), max(ref_err))
    for p, mst in zip(params, masters):
        if p.dtype != F32:
            assert mst.dtype == F32
            assert torch.equal(p.data, mst.to(BF16))


def _run_eager(cls, ws, grads_per_step, **kw):
    params = _params(ws)
    opt = cls(params, **kw)
    for grads in grads_per_step:
        for p, g in zip(params, grads):
            p.grad = g.to(DEV)
        opt.step()
    return opt, params


KINDS = {"adam": FusedAdamW, "lamb": FusedLAMB}


# ---- 1. eager steps at every size ------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("adam_w_mode", [False, True])
def test_adamw_5_steps(adam_w_mode, wd):
    ws, grads = _make(11, 5)
    opt, params = _run_eager(FusedAdamW, ws, grads, lr=LR, weight_decay=wd,
                             adam_w_mode=adam_w_mode)
    oracle = Oracle(ws, "adam", wd=wd, adam_w_mode=adam_w_mode)
    for g in grads:
        oracle.step(g)
    ref_w = _fp32_ref("adam", ws, grads, [LR] * 5, wd, adam_w_mode)
    _check(opt, params, ref_w, oracle)
    assert int(opt.param_groups[0]["step"]) == 5


@pytest.mark.parametrize("adam_w_mode", [False, True])
def test_lamb_5_steps(adam_w_mode):
    ws, grads = _make(12, 5)
    opt, params = _run_eager(FusedLAMB, ws, grads, lr=LR, weight_decay=0.01,
                             adam_w_mode=adam_w_mode)
    oracle = Oracle(ws, "lamb", adam_w_mode=adam_w_mode)
    for g in grads:
        oracle.step(g)
    ref_w = _fp32_ref("lamb", ws, grads, [LR] * 5, 0.01, adam_w_mode)
    _check(opt, params, ref_w, oracle)


# ---- 2./3. graph replay -------------------------------------------------------
def _replay_case(kind, lrs):
    """One eager warm-up step, then ONE captured step() replayed for the
    remaining steps with fresh grads copied into the static grad tensors.
    lrs[k] is the learning rate of step k; a change takes effect through
    group['lr'] + refresh_hyperparams() between replays."""
    steps = len(lrs)
    ws, grads = _make(13, steps)
    dgrads = [[g.to(DEV) for g in gs] for gs in grads]
    params = _params(ws)
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = KINDS[kind](params, lr=lrs[0])

    def load(k):
        torch._foreach_copy_([p.grad for p in params], dgrads[k])

    load(0)
    opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(1, steps):
        load(k)
        if lrs[k] != opt.param_groups[0]["lr"]:
            opt.param_groups[0]["lr"] = lrs[k]
            opt.refresh_hyperparams()
        graph.replay()
    torch.cuda.synchronize()

    oracle = Oracle(ws, kind)
    for lr, g in zip(lrs, grads):
        oracle.lr = lr
        oracle.step(g)
    ref_w = _fp32_ref(kind, ws, grads, lrs, 0.01, True)
    _check(opt, params, ref_w, oracle)
    assert int(opt.param_groups[0]["step"]) == steps


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_graph_replay_advances_step_state(kind):
    # fails if the bias corrections are frozen at capture time
    _replay_case(kind, [LR] * 5)


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_lr_change_under_replay(kind):
    _replay_case(kind, [LR, 3e-3, 3e-3])


# ---- 4. LAMB trust ratios -------------------------------------------------------
def test_lamb_adjacent_tensors_with_norms_1e4_apart():
    # two fp32 tensors side by side in one launch, the second multi-block;
    # partials leaking across the boundary would move a ratio by orders
    specs = [(EPB + 5, F32), (2 * EPB + 7, F32), (EPB + 5, F32)]
    ws, grads = _make(15, 3, specs=specs, wscale=[0.43, 0.43e-4, 0.43])
    opt, params = _run_eager(FusedLAMB, ws, grads, lr=LR)
    oracle = Oracle(ws, "lamb")
    for g in grads:
        oracle.step(g)
    ref_w = _fp32_ref("lamb", ws, grads, [LR] * 3, 0.01, True)
    _check(opt, params, ref_w, oracle, per_tensor=True)


def _direct_lamb(ws, grads, wd):
    """One ops.lamb_step call on fresh state; returns (masters, ratio)."""
    masters = [w.float().to(DEV) for w in ws]
    dg = [g.to(DEV) for g in grads]
    m = [torch.zeros_like(x) for x in masters]
    v = [torch.zeros_like(x) for x in masters]
    outs = [torch.empty_like(x, dtype=BF16) if w.dtype == BF16 else None
            for x, w in zip(masters, ws)]
    scalars = torch.zeros(ref.OPT_SCALARS, device=DEV)
    scalars[ref.OPT_LR] = LR
    scalars[ref.OPT_CLIP] = 1.0
    nb = sum((w.numel() + EPB - 1) // EPB for w in ws)
    partials = torch.zeros(3 * nb, device=DEV)
    ratio = torch.full((len(ws),), -1.0, device=DEV)
    ops.lamb_step(masters, dg, m, v, outs, scalars, partials, ratio,
                  BETAS[0], BETAS[1], 1e-6, wd, True, None)
    return masters, ratio


def test_lamb_zero_weight_and_zero_grad_get_ratio_one():
    specs = [(EPB + 3, F32), (EPB + 3, F32), (3 * EPB + 5, F32)]
    ws, grads = _make(16, 1, specs=specs)
    ws[0].zero_()
    grads[0][1].zero_()
    masters, ratio = _direct_lamb(ws, grads[0], wd=0.0)
    assert ratio[0].item() == 1.0 and ratio[1].item() == 1.0
    assert ratio[2].item() > 0 and ratio[2].item() != 1.0
    for mst in masters:
        assert torch.isfinite(mst).all()
    assert torch.equal(masters[1].cpu(), ws[1])  # u == 0: untouched
    oracle = Oracle(ws, "lamb", wd=0.0)
    oracle.step(grads[0])
    ref_w = _fp32_ref("lamb", ws, grads, [LR], 0.0, True)
    err, ref_err = max(_errs(masters, oracle.w)), max(_errs(ref_w, oracle.w))
    print(f"kernel max err {err:.3e}  fp32 reference max err {ref_err:.3e}")
    assert ref_err > 0 and err <= 4 * ref_err


def test_lamb_is_deterministic():
    ws, grads = _make(17, 1)
    a, ra = _direct_lamb(ws, grads[0], wd=0.01)
    b, rb = _direct_lamb(ws, grads[0], wd=0.01)
    assert torch.equal(ra, rb)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 5. clipping -----------------------------------------------------------------
def _scaled_grads(grads_per_step, target_norm):
    out = []
    for grads in grads_per_step:
        norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
        out.append([(g.float() * (target_norm / norm)).to(g.dtype) for g in grads])
    return out


def test_clip_active_matches_clip_grad_norm():
    ws, grads = _make(18, 3)
    grads = _scaled_grads(grads, 10.0)
    opt, params = _run_eager(FusedAdamW, ws, grads, lr=LR, max_grad_norm=1.0)
    oracle = Oracle(ws, "adam", max_grad_norm=1.0)
    for g in grads:
        oracle.step(g)
    ref_w = _fp32_ref("adam", ws, grads, [LR] * 3, 0.01, True, max_grad_norm=1.0)
    _check(opt, params, ref_w, oracle)
    clip = opt._blocks[0][ref.OPT_CLIP].item()
    assert abs(clip - 0.1) < 1e-3, clip


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_clip_inactive_is_bit_identical_to_no_clip(kind):
    ws, grads = _make(19, 2)
    grads = _scaled_grads(grads, 0.1)
    oa, pa = _run_eager(KINDS[kind], ws, grads, lr=LR, max_grad_norm=1.0)
    ob, pb = _run_eager(KINDS[kind], ws, grads, lr=LR, max_grad_norm=None)
    for x, y in zip(_masters(oa, pa), _masters(ob, pb)):
        assert torch.equal(x, y)
    for x, y in zip(pa, pb):
        assert torch.equal(x.data, y.data)


# ---- 6. DistributedOptimizer (bucket-view grads, world size 1) -----------------
@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_through_distributed_optimizer(kind):
    from mpi_operator_amd.parallel import DistributedOptimizer
    specs = [(3, BF16), (EPB - 1, BF16), (EPB + 1, F32), (3, F32),
             (3 * EPB + 5, BF16), (EPB, F32)]
    ws, grads = _make(20, 1, specs=specs)
    coef = [g.to(DEV) for g in grads[0]]

    pa = _params(ws)
    oa = KINDS[kind](pa, lr=LR)
    dopt = DistributedOptimizer(oa)
    dopt.zero_grad()
    loss = sum((p.float() * c.float()).sum() for p, c in zip(pa, coef))
    loss.backward()
    # grads are now views into the flat buckets, at unaligned offsets too
    assert any(p.grad.storage_offset() % 8 for p in pa)
    for p, c in zip(pa, coef):
        assert torch.equal(p.grad, c)
    dopt.step()

    pb = _params(ws)
    ob = KINDS[kind](pb, lr=LR)
    for p, c in zip(pb, coef):
        p.grad = c.clone()
    ob.step()
    for x, y in zip(_masters(oa, pa), _masters(ob, pb)):
        assert torch.equal(x, y)
    for x, y in zip(pa, pb):
        assert torch.equal(x.data, y.data)


# ---- 7. model steps ----------------------------------------------------------------
@pytest.mark.parametrize("cls,lr", [(FusedAdamW, 1e-4), (FusedLAMB, 2e-3)])
def test_bert_base_descends(cls, lr):
    from mpi_operator_amd.models.bert import bert_base, bert_param_groups, to_mi355x_bert
    torch.manual_seed(2)
    m = to_mi355x_bert(bert_base(), "cuda")
    m.train()
    opt = cls(bert_param_groups(m, 0.01), lr=lr)
    ids = torch.randint(0, m.cfg.vocab_size, (2, 64), device="cuda")
    mlm_labels = ids.clone()
    nsp = torch.randint(0, 2, (2,), device="cuda")
    losses = []
    for _ in range(8):
        opt.zero_grad()
        mlm_logits, nsp_logits = m(ids)
        loss = m.loss(mlm_logits, nsp_logits, mlm_labels, nsp)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"{cls.__name__} lr={lr} losses {[round(l, 4) for l in losses]}")
    assert all(math.isfinite(l) for l in losses), losses
    assert losses[-1] < losses[0], losses
