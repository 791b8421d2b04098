"""FusedAdamW / FusedLAMB on the CPU reference path: torch.optim parity,
an fp64 LAMB written out here, and the state-dict round trip."""
import copy

import pytest
import torch

from mpi_operator_amd.optim import FusedAdamW, FusedLAMB

# fp32 weights of Linear(8, 8) stay below 0.5 (ulp 6e-8); 5 steps of a few
# roundings each stay well inside 1e-6 — the bound test_optim_cpu.py uses
ATOL = 1e-6


def _models(n=2):
    torch.manual_seed(3)
    a = torch.nn.Linear(8, 8)
    out = [a]
    for _ in range(n - 1):
        b = torch.nn.Linear(8, 8)
        b.load_state_dict(a.state_dict())
        out.append(b)
    return out


def _train(model, opt, x, steps):
    for _ in range(steps):
        opt.zero_grad()
        model(x).pow(2).mean().backward()
        opt.step()


@pytest.mark.parametrize("adam_w_mode", [True, False])
def test_fused_adamw_matches_torch(adam_w_mode):
    a, b = _models()
    oa = FusedAdamW(a.parameters(), lr=1e-2, weight_decay=0.01, adam_w_mode=adam_w_mode)
    tcls = torch.optim.AdamW if adam_w_mode else torch.optim.Adam
    ob = tcls(b.parameters(), lr=1e-2, weight_decay=0.01)
    x = torch.randn(4, 8)
    _train(a, oa, x, 5)
    _train(b, ob, x, 5)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=ATOL, rtol=0), (pa - pb).abs().max()
    assert int(oa.param_groups[0]["step"]) == 5


def _lamb_fp64(params, grads_per_step, lr, beta1, beta2, eps, wd):
    """LAMB in fp64 from the formulas: u = m_hat/(sqrt(v_hat)+eps) + wd*w,
    ratio = ||w||/||u|| (1 if either is 0), w -= lr*ratio*u."""
    w = [p.detach().double().clone() for p in params]
    m = [torch.zeros_like(t) for t in w]
    v = [torch.zeros_like(t) for t in w]
    for step, grads in enumerate(grads_per_step, 1):
        bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
        for i, g in enumerate(grads):
            g = g.double()
            m[i] = beta1 * m[i] + (1 - beta1) * g
            v[i] = beta2 * v[i] + (1 - beta2) * g * g
            u = (m[i] / bc1) / ((v[i] / bc2).sqrt() + eps) + wd * w[i]
            nw, nu = w[i].norm(), u.norm()
            ratio = (nw / nu).item() if (nw > 0 and nu > 0) else 1.0
            w[i] = w[i] - lr * ratio * u
    return w


def test_fused_lamb_matches_fp64_formulas():
    (a,) = _models(1)
    params = list(a.parameters())
    init = [p.detach().clone() for p in params]
    opt = FusedLAMB(params, lr=1e-2, weight_decay=0.01)
    x = torch.randn(4, 8)
    grads_per_step = []
    for _ in range(5):
        opt.zero_grad()
        a(x).pow(2).mean().backward()
        grads_per_step.append([p.grad.clone() for p in params])
        opt.step()
    want = _lamb_fp64(init, grads_per_step, 1e-2, 0.9, 0.999, 1e-6, 0.01)
    for p, w in zip(params, want):
        assert torch.allclose(p.double(), w, atol=ATOL, rtol=0), (p.double() - w).abs().max()


def test_lamb_zero_tensors_get_ratio_one():
    w0 = torch.zeros(5, requires_grad=True)   # ||w|| = 0
    w1 = torch.ones(5, requires_grad=True)    # grad 0, wd 0 -> ||u|| = 0
    opt = FusedLAMB([w0, w1], lr=0.1, weight_decay=0.0)
    w0.grad = torch.full((5,), 2.0)
    w1.grad = torch.zeros(5)
    opt.step()
    # first step: m_hat/sqrt(v_hat) = sign(g) -> w0 moves by lr * 1 * 1
    assert torch.allclose(w0, torch.full((5,), -0.1), atol=1e-6)
    assert torch.equal(w1, torch.ones(5))


def test_clip_matches_clip_grad_norm():
    a, b = _models()
    oa = FusedAdamW(a.parameters(), lr=1e-2, max_grad_norm=0.05)
    ob = torch.optim.AdamW(b.parameters(), lr=1e-2)
    x = torch.randn(4, 8) * 3
    for _ in range(3):
        oa.zero_grad(); ob.zero_grad()
        a(x).pow(2).mean().backward()
        b(x).pow(2).mean().backward()
        n = torch.nn.utils.clip_grad_norm_(b.parameters(), 0.05)
        assert n > 0.05  # the clip is active
        oa.step(); ob.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=ATOL, rtol=0), (pa - pb).abs().max()


@pytest.mark.parametrize("cls", [FusedAdamW, FusedLAMB])
def test_state_dict_round_trip(cls):
    a, b = _models()
    x = torch.randn(4, 8)
    oa = cls(a.parameters(), lr=1e-2)
    _train(a, oa, x, 2)
    sd = copy.deepcopy(oa.state_dict())
    assert int(sd["param_groups"][0]["step"]) == 2
    st = next(iter(sd["state"].values()))
    assert {"exp_avg", "exp_avg_sq"} <= set(st)

    b.load_state_dict(a.state_dict())
    ob = cls(b.parameters(), lr=1e-2)
    ob.load_state_dict(sd)
    assert int(ob.param_groups[0]["step"]) == 2
    _train(a, oa, x, 1)
    _train(b, ob, x, 1)
    assert int(ob.param_groups[0]["step"]) == 3
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


def test_load_into_a_stepped_optimizer_keeps_its_tensors():
    """A captured graph holds the addresses of the state tensors and of the
    scalar block: loading must write into them, not replace them."""
    a, b = _models()
    x = torch.randn(4, 8)
    oa = FusedAdamW(a.parameters(), lr=1e-2)
    ob = FusedAdamW(b.parameters(), lr=1e-2)
    _train(a, oa, x, 3)
    _train(b, ob, x, 1)
    sd = copy.deepcopy(oa.state_dict())
    pb = next(iter(b.parameters()))
    m_before, step_before = ob.state[pb]["exp_avg"], ob.param_groups[0]["step"]
    ob.load_state_dict(sd)
    assert ob.state[pb]["exp_avg"] is m_before
    assert ob.param_groups[0]["step"].data_ptr() == step_before.data_ptr()
    assert int(ob.param_groups[0]["step"]) == 3
    assert torch.equal(m_before, oa.state[next(iter(a.parameters()))]["exp_avg"])


def test_bf16_params_keep_fp32_master_across_load():
    torch.manual_seed(4)
    m = torch.nn.Linear(16, 4).to(torch.bfloat16)
    opt = FusedAdamW(m.parameters(), lr=1e-2)
    x = torch.randn(8, 16, dtype=torch.bfloat16)
    for _ in range(3):
        opt.zero_grad()
        m(x).float().pow(2).mean().backward()
        opt.step()
    st = opt.state[m.weight]
    assert st["master"].dtype == torch.float32
    assert torch.equal(st["master"].to(torch.bfloat16), m.weight.data)
    sd = copy.deepcopy(opt.state_dict())
    opt2 = FusedAdamW(m.parameters(), lr=1e-2)
    opt2.load_state_dict(sd)
    st2 = opt2.state[m.weight]
    for k in ("master", "exp_avg", "exp_avg_sq"):
        assert st2[k].dtype == torch.float32
        assert torch.equal(st2[k], st[k]) and st2[k] is not st[k]


def test_lr_change_is_picked_up_eagerly():
    a, b = _models()
    oa = FusedAdamW(a.parameters(), lr=1e-2)
    ob = torch.optim.AdamW(b.parameters(), lr=1e-2)
    x = torch.randn(4, 8)
    _train(a, oa, x, 2)
    _train(b, ob, x, 2)
    oa.param_groups[0]["lr"] = 3e-3
    ob.param_groups[0]["lr"] = 3e-3
    _train(a, oa, x, 2)
    _train(b, ob, x, 2)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=ATOL, rtol=0), (pa - pb).abs().max()


def test_make_trainer_accepts_adamw_and_lamb():
    from mpi_operator_amd.trainer import make_trainer
    for name, cls in (("adamw", FusedAdamW), ("lamb", FusedLAMB)):
        (m,) = _models(1)
        dopt = make_trainer(m, lr=1e-3, optimizer=name)
        assert isinstance(dopt.optimizer, cls)
    with pytest.raises(ValueError):
        make_trainer(_models(1)[0], optimizer="adagrad")


def test_bert_param_groups_exempt_bias_and_layernorm():
    from mpi_operator_amd.models.bert import BertConfig, BertForPreTraining, bert_param_groups
    cfg = BertConfig(vocab_size=64, hidden=16, layers=1, heads=2, intermediate=32, max_seq=8)
    model = BertForPreTraining(cfg)
    decay, exempt = bert_param_groups(model, 0.01)
    assert decay["weight_decay"] == 0.01 and exempt["weight_decay"] == 0.0
    names = {id(p): n for n, p in model.named_parameters()}
    exempt_names = {names[id(p)] for p in exempt["params"]}
    decay_names = {names[id(p)] for p in decay["params"]}
    assert exempt_names | decay_names == set(names.values())
    assert not exempt_names & decay_names
    assert all(n.endswith("bias") or ".ln" in n or "_ln" in n for n in exempt_names), exempt_names
    assert all(n.endswith("weight") for n in decay_names), decay_names
    assert "mlm_ln.weight" in exempt_names and "bert.embeddings.tok.weight" in decay_names
