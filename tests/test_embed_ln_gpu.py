"""Fx.embedding / Fx.embed_layer_norm (csrc/embedding.hip) against the fp64
references of ops/reference.py on the same bf16 inputs. Derived bounds: one
bf16 rounding errs by at most 2^-8 relative, an fp32 sum of T terms by at
most T·2^-23·Σ|term|."""
import os
import subprocess
import sys

import pytest
import torch

from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-12
SEED, SITE = 1234, 3
BF, F64 = torch.bfloat16, torch.float64


def _bf16(*shape):
    return torch.randn(*shape, device="cuda").to(BF)


def _patterns(name, R):
    """(idx, rows) per index pattern, built from the chunk size R."""
    if name == "distinct":
        return torch.randperm(300)[:257], 300
    if name == "equal":
        return torch.full((4 * R + 3,), 2), 5
    if name == "runs":  # runs start and end on, before and after chunk edges
        lens = [1, R - 1, R, R + 1, 2 * R + 1]
        return torch.repeat_interleave(torch.tensor([0, 3, 4, 7, 9]),
                                       torch.tensor(lens)), 11
    hit = torch.tensor([0, 30521, 103, 103, 2000, 0, 103, 15000])
    return hit.repeat(R // 4 + 1), 30522  # "vocab": a handful of rows hit


@pytest.mark.parametrize("hidden", [64, 1032])
@pytest.mark.parametrize("pattern", ["distinct", "equal", "runs", "vocab"])
def test_embedding_backward(pattern, hidden):
    torch.manual_seed(0)
    idx, rows = _patterns(pattern, Fx.EMBED_BWD_CHUNK)
    idx = idx[torch.randperm(idx.numel())].cuda()  # the sort is the op's job
    T = idx.numel()
    w = _bf16(rows, hidden).requires_grad_()
    dy = _bf16(T, hidden)
    y = Fx.embedding(idx, w)
    assert torch.equal(y, w.detach()[idx])
    (g1,) = torch.autograd.grad(y, w, dy)
    (g2,) = torch.autograd.grad(Fx.embedding(idx, w), w, dy)
    assert torch.equal(g1, g2), "second call differs"
    want = ref.embedding_bwd(dy.to(F64), idx, rows)
    mag = ref.embedding_bwd(dy.to(F64).abs(), idx, rows)
    err = (g1.to(F64) - want).abs()
    bound = 2.0 ** -8 * want.abs() + T * 2.0 ** -23 * mag
    print(pattern, hidden, "err/bound", (err / bound.clamp_min(1e-300)).max().item())
    assert (err <= bound).all()
    untouched = torch.ones(rows, dtype=torch.bool, device="cuda")
    untouched[idx] = False
    assert (g1[untouched] == 0).all()


def _case(B, S, hidden, with_type, packed, int32=False):
    V, P, TY = 97, max(S, 8) + 3, 2
    it = torch.int32 if int32 else torch.int64
    c = dict(tok=_bf16(V, hidden), pos=_bf16(P, hidden), typ=_bf16(TY, hidden),
             ln_w=torch.rand(hidden, device="cuda") + 0.5,
             ln_b=torch.randn(hidden, device="cuda") * 0.2,
             ids=torch.randint(0, V, (B, S), device="cuda", dtype=it),
             type_ids=None, position_ids=None, rows=(V, P, TY))
    c["ids"][0, : S // 2] = 5  # a run in the token table
    if with_type:
        c["type_ids"] = torch.randint(0, TY, (B, S), device="cuda", dtype=it)
    if packed:  # positions restart at 0 per sequence of length 3
        c["position_ids"] = (torch.arange(B * S, device="cuda") % 3).view(
            B, S).to(it)
    return c


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("with_type", [False, True])
@pytest.mark.parametrize("B,S", [(2, 5), (3, 129)])
@pytest.mark.parametrize("hidden", [64, 768, 1024, 1032])
def test_embed_layer_norm(hidden, B, S, with_type, packed, p):
    """Table-gradient bound: dsum carries one bf16 rounding per term, so
    2^-7·Σ|dsum_ref,i| over the row's run plus 2^-8·|ref|. With p > 0 the
    reference takes d = bf16(dy·keep·scale), the rounding of the reused
    dropout_bwd ahead of the LayerNorm backward (without it the bound, which
    is relative to dsum, was missed 2029-fold on a cancelled dsum element)."""
    torch.manual_seed(hidden + S)
    c = _case(B, S, hidden, with_type, packed, int32=(hidden == 64))
    rng = Fx.DropoutRng(SEED, "cuda")
    leaves = [c[k].requires_grad_() for k in ("tok", "pos", "typ", "ln_w", "ln_b")]
    y, mask = Fx.embed_layer_norm_with_mask(
        c["ids"], *leaves, EPS, c["type_ids"], c["position_ids"], p, rng, SITE)
    dy = _bf16(B, S, hidden)
    y.backward(dy)

    keep, scale = None, 1.0
    if p > 0:
        bits = (mask[:, None] >> torch.arange(8, device="cuda")) & 1 == 1
        keep = ref.philox_dropout_mask(SEED, 0, SITE, y.shape, p).cuda()
        assert torch.equal(bits.view(y.shape), keep)
        assert (y[~keep] == 0).all()
        scale = ref.dropout_threshold(p)[2]
    t64 = [t.detach().to(F64) for t in leaves]
    yr, s, mean, rstd = ref.embed_layer_norm_fwd(
        c["ids"], *t64, EPS, c["type_ids"], c["position_ids"], keep, scale, BF)
    assert ((y.to(F64) - yr).abs()
            <= 2.0 ** -8 * yr.abs() + 1e-5 * (1 + yr.abs())).all()
    d = dy if p == 0 else (dy.float() * keep * scale).to(BF)
    r = ref.embed_layer_norm_bwd(d.to(F64), c["ids"], s, mean, rstd, t64[3],
                                 c["rows"], c["type_ids"], c["position_ids"])
    dsum, want = r[0], dict(tok=r[1], pos=r[2], typ=r[3])
    pos_idx = ref._embed_positions(c["ids"], c["position_ids"])
    for k, idx in (("tok", c["ids"]), ("pos", pos_idx), ("typ", c["type_ids"])):
        if idx is None:
            assert c[k].grad is None
            continue
        mag = ref.embedding_bwd(dsum.abs(), idx, want[k].shape[0])
        err = (c[k].grad.to(F64) - want[k]).abs()
        bound = 2.0 ** -7 * mag + 2.0 ** -8 * want[k].abs()
        print("d" + k, "err/bound", (err / bound.clamp_min(1e-300)).max().item())
        assert (err <= bound).all(), k
    for got, exp in ((c["ln_w"].grad, r[4]), (c["ln_b"].grad, r[5])):
        assert (got.to(F64) - exp).norm() / exp.norm() < 0.02


def test_graph_replay_matches_eager():
    torch.manual_seed(2)
    c = _case(2, 64, 64, True, True)
    tabs = [c[k].requires_grad_() for k in ("tok", "pos", "typ", "ln_w", "ln_b")]
    dy = _bf16(2, 64, 64)

    def step():
        y = Fx.embed_layer_norm(c["ids"], *tabs, EPS, c["type_ids"],
                                c["position_ids"])
        return (y,) + torch.autograd.grad(y, tabs, dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for _ in range(2):  # new contents, same buffers
        c["ids"].copy_(torch.randint(0, 97, (2, 64), device="cuda"))
        c["position_ids"].copy_(torch.randint(0, 60, (2, 64), device="cuda"))
        g.replay()
        for got, exp in zip(out, step()):
            assert torch.equal(got, exp)


def test_specialised_widths_under_ln_spec():
    """The C8T = 96 / 128 kernels launch only with MPIAMD_LN_SPEC=1, read
    once per process: the hidden 768 / 1024 cases again in a child with it."""
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
           os.path.join("tests", "test_embed_ln_gpu.py"), "-k",
           "layer_norm[768- or layer_norm[1024-"]
    r = subprocess.run(cmd, env=dict(os.environ, MPIAMD_LN_SPEC="1"), cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "32 passed" in out, out[-3000:]


_CHILD = """
import sys, torch
from mpi_operator_amd.models import bert
from mpi_operator_amd.ops import functional as Fx
calls, fused = [], Fx.embed_layer_norm
Fx.embed_layer_norm = lambda *a, **k: calls.append(1) or fused(*a, **k)
torch.manual_seed(5)
cfg = bert.BertConfig(vocab_size=512, hidden=64, layers=2, heads=1, intermediate=128, max_seq=32, dropout=0.1)
m = bert.to_mi355x_bert(bert.BertForPreTraining(cfg), "cuda").train()
m.seed_dropout(7)
ids = torch.randint(0, 512, (3, 16), device="cuda")
typ = torch.randint(0, 2, (3, 16), device="cuda", dtype=torch.int32)
lab = ids.clone(); lab[:, ::2] = -100
nsp = torch.randint(0, 2, (3,), device="cuda")
am = (torch.arange(16, device="cuda")[None] < torch.tensor([16, 9, 4], device="cuda")[:, None]).long()
out = {}
for name in ("dense", "packed"):
    m.zero_grad(set_to_none=True)
    if name == "dense":
        loss = m(ids, typ, None, lab, nsp)
    else:
        pk = bert.pack_padded_batch(ids, typ, am, lab, max_seq=32)
        loss = m(pk.ids, pk.type_ids, None, pk.mlm_labels, nsp, cu_seqlens=pk.cu_seqlens, max_seqlen=pk.max_seqlen, position_ids=pk.position_ids)
    loss.backward()
    e = m.bert.embeddings
    out[name] = [loss.detach().float().cpu()] + [t.weight.grad.float().cpu() for t in (e.tok, e.pos, e.typ)]
out["fused_calls"] = len(calls)
torch.save(out, sys.argv[1])
"""


def test_model_fused_embed_matches_torch_chain(tmp_path):
    """Dropout 0.1 (same masks on both paths), int32 type ids with int64 ids."""
    res = {}
    for knob in ("1", "0"):  # read at import: fresh child processes
        path = str(tmp_path / f"embed{knob}.pt")
        env = dict(os.environ, MPIAMD_FUSED_EMBED=knob)
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res[knob] = torch.load(path)
    assert res["1"]["fused_calls"] == 2 and res["0"]["fused_calls"] == 0
    for name in ("dense", "packed"):
        (la, *ga), (lb, *gb) = res["1"][name], res["0"][name]
        assert abs(la - lb) < 0.05 * abs(lb) + 5e-2
        for a, b in zip(ga, gb):
            assert (a - b).abs().max() < 0.1 * b.abs().max() + 1e-4
