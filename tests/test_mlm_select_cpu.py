"""Fx.mlm_select / Fx.gather_rows on the CPU reference path against torch
boolean indexing, and BertForPreTraining(max_predictions=...) against the
all-rows head in fp32."""
import pytest
import torch

from mpi_operator_amd.models.bert import BertConfig, BertForPreTraining
from mpi_operator_amd.ops import functional as Fx


@pytest.mark.parametrize("capacity", [40, 7])  # above / below the 15 labelled
def test_select_and_gather_match_boolean_indexing(capacity):
    g = torch.Generator().manual_seed(0)
    M, n = 50, min(capacity, 15)
    labels = torch.full((M,), -100)
    rows = torch.randperm(M, generator=g)[:15].sort().values
    labels[rows] = torch.randint(0, 99, (15,), generator=g)
    pos, slot, labels_c, counts = Fx.mlm_select(labels.view(5, 10), capacity)
    assert counts.tolist() == [n, 15 - n] and pos.dtype == slot.dtype == torch.int32
    assert pos.tolist() == rows[:n].tolist() + [-1] * (capacity - n)
    assert labels_c.tolist() == labels[rows[:n]].tolist() + [-100] * (capacity - n)
    keep = torch.zeros(M, dtype=torch.bool)
    keep[rows[:n]] = True  # past the capacity the last rows are dropped
    assert slot[keep].tolist() == list(range(n)) and (slot[~keep] == -1).all()
    x = torch.randn(M, 16, generator=g, dtype=torch.float64).requires_grad_()
    out = Fx.gather_rows(x, pos, slot)
    assert torch.equal(out[:n], x.detach()[rows[:n]]) and (out[n:] == 0).all()
    dout = torch.randn(capacity, 16, generator=g, dtype=torch.float64)
    (dx,) = torch.autograd.grad(out, x, dout)
    assert torch.equal(dx[keep], dout[:n]) and (dx[~keep] == 0).all()


def test_model_max_predictions_matches_all_rows_head():
    torch.manual_seed(3)
    m = BertForPreTraining(BertConfig(vocab_size=500, hidden=64, layers=2, heads=2,
                                      intermediate=128, max_seq=32))
    ids, typ = torch.randint(0, 500, (3, 24)), torch.randint(0, 2, (3, 24))
    labels = torch.where(torch.rand(3, 24) < 0.2, ids, -100)
    labels[0, 0] = 5
    a = (ids, typ, None, labels, torch.tensor([0, 1, 1]))
    n, params = int((labels != -100).sum()), list(m.parameters())
    want = m(*a)
    grads = torch.autograd.grad(want, params)
    got = m(*a, max_predictions=n + 3)
    assert m.mlm_counts.tolist() == [n, 0]
    torch.testing.assert_close(got, want)
    for p, b in zip(torch.autograd.grad(got, params), grads):
        torch.testing.assert_close(p, b, rtol=1e-4, atol=1e-6)
    with pytest.raises(ValueError, match="max_predictions"):
        m(ids, max_predictions=8)
