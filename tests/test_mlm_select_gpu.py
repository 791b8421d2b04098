"""csrc/mlm_select.hip: select, gather and scatter are pure copies and equal
torch indexing exactly; the head on the gathered rows against fp64, and the
model with max_predictions against its all-rows head, at the tolerances of
test_bert_gpu.test_mlm_head_loss_matches_composed_path."""
import pytest
import torch

from mpi_operator_amd.models import bert
from mpi_operator_amd.ops import functional as Fx
from mpi_operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
TILE = 2048  # Fx.MLM_SELECT_TILE; M = 5096 spans three tiles, the last partly
BF = torch.bfloat16


def _labels(M, kind):
    g = torch.Generator().manual_seed(M)
    lab = torch.randint(0, 30522, (M,), generator=g)
    lab[{"some": torch.rand(M, generator=g) >= 0.15, "all": torch.zeros(M, dtype=bool),
         "none": torch.ones(M, dtype=bool),
         # rows of the last tile's last active wave only
         "last_wave": torch.arange(M) < M - 56}[kind]] = -100
    return lab.cuda()


def _run(lab, x, dout, P):
    sel = Fx.mlm_select(lab, P)
    out = Fx.gather_rows(x, sel[0], sel[1])
    return sel + (out,) + torch.autograd.grad(out, x, dout)


@pytest.mark.parametrize("M,hidden,P,kind", [
    (5, 64, 4, "some"), (TILE - 1, 64, 400, "some"), (TILE + 3, 768, TILE + 3, "all"),
    (TILE + 3, 64, 100, "all"), (5096, 64, 128, "none"), (5096, 768, 900, "some"),
    (5096, 64, 200, "some"), (5096, 64, 64, "last_wave")])
def test_select_gather_scatter_exact(M, hidden, P, kind):
    assert Fx.MLM_SELECT_TILE == TILE
    lab = _labels(M, kind)
    x = torch.randn(M, hidden, device="cuda").to(BF).requires_grad_()
    dout = torch.randn(P, hidden, device="cuda").to(BF)
    pos, slot, labels_c, counts, out, dx = got = _run(lab, x, dout, P)
    for a, b in zip(got, _run(lab, x, dout, P)):
        assert torch.equal(a, b), "second call differs"
    rows = torch.nonzero(lab != -100).flatten()
    n = min(P, rows.numel())
    assert counts.tolist() == [n, rows.numel() - n]
    for a, b in zip(got[:4], ref.mlm_select(lab.cpu(), P)):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b)
    keep = torch.zeros(M, dtype=torch.bool, device="cuda")
    keep[rows[:n]] = True  # past the capacity the LAST rows are dropped
    assert torch.equal(slot >= 0, keep)
    assert torch.equal(out[:n], x.detach()[rows[:n]]) and (out[n:] == 0).all()
    assert torch.equal(dx[keep], dout[:n]) and (dx[~keep] == 0).all()


def _close(loss, want, grads, wants):
    assert abs(loss.item() - want.item()) < 2e-3 * abs(want.item()) + 1e-4
    for a, c in zip(grads, wants):
        a, c = a.double().cpu(), c.double().cpu()
        assert (a - c).norm() / (c.norm() + 1e-30) < 0.02, a.shape


def test_head_on_gathered_rows_matches_fp64():
    torch.manual_seed(7)
    M, K, V, P = 256, 768, 30522, 192
    h = ((torch.rand(M, K, device="cuda") * 2 - 1) * 0.5).to(BF).requires_grad_()
    w = ((torch.rand(V, K, device="cuda") * 2 - 1) * 0.05).to(BF).requires_grad_()
    b = (torch.randn(V, device="cuda") * 0.01).requires_grad_()
    tgt = torch.randint(0, V, (M,), device="cuda")
    tgt[::3] = -100
    pos, slot, labels_c, _ = Fx.mlm_select(tgt, P)
    loss = Fx.mlm_head_loss(Fx.gather_rows(h, pos, slot), w, b, labels_c)
    r = [t.detach().double().cpu().requires_grad_() for t in (h, w, b)]
    want = torch.nn.functional.cross_entropy(r[0] @ r[1].t() + r[2], tgt.cpu(),
                                             ignore_index=-100)
    _close(loss, want, torch.autograd.grad(loss, (h, w, b)), torch.autograd.grad(want, r))


@pytest.mark.parametrize("packed", [False, True])
def test_model_max_predictions_matches_all_rows_head(packed):
    torch.manual_seed(11)
    cfg = bert.BertConfig(vocab_size=1000, hidden=128, layers=2, heads=2,
                          intermediate=256, max_seq=128)
    m = bert.to_mi355x_bert(bert.BertForPreTraining(cfg), "cuda").train()
    ids = torch.randint(0, 1000, (2, 128), device="cuda")
    typ = torch.randint(0, 2, (2, 128), device="cuda")
    mask = torch.rand(2, 128, device="cuda") < 0.15
    lab = torch.where(mask & (mask.cumsum(1) <= 24), ids, -100)  # fits 2 * 24
    nsp = torch.tensor([1, 0], device="cuda")
    a, kw = (ids, typ, None, lab, nsp), {}
    if packed:
        am = torch.arange(128, device="cuda")[None] < torch.tensor([[128], [70]], device="cuda")
        pk = bert.pack_padded_batch(ids, typ, am, lab, token_budget=256, max_seq=128)
        a = (pk.ids, pk.type_ids, None, pk.mlm_labels, nsp)
        kw = dict(cu_seqlens=pk.cu_seqlens, max_seqlen=128, position_ids=pk.position_ids)
    params = list(m.parameters())
    want = m(*a, **kw)
    wants = torch.autograd.grad(want, params)
    loss = m(*a, **kw, max_predictions=2 * 24)
    assert m.mlm_counts.tolist() == [int((a[3] != -100).sum()), 0]
    _close(loss, want, torch.autograd.grad(loss, params), wants)


def test_graph_replay_on_other_labels_matches_eager():
    M, hidden, P = TILE + 3, 64, 300
    lab = _labels(M, "some")
    x = torch.randn(M, hidden, device="cuda").to(BF).requires_grad_()
    dout = torch.randn(P, hidden, device="cuda").to(BF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(lab, x, dout, P)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, no parallel branches
        out = _run(lab, x, dout, P)
    for new in (_labels(M, "last_wave"), _labels(M, "all")):  # 56, then M > P
        lab.copy_(new)
        g.replay()
        for got, exp in zip(out, _run(lab, x, dout, P)):
            assert torch.equal(got, exp)
