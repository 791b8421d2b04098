"""Packed (unpadded) BERT batches on the CPU: a padded-and-masked batch and
the same sequences through pack_padded_batch give the same pre-training loss
and parameter gradients; pack_padded_batch round-trips and rejects what does
not fit."""
import pytest
import torch

from mpi_operator_amd.models.bert import (BertConfig, BertForPreTraining,
                                          pack_padded_batch)

B, S = 3, 48
LENS = [48, 17, 5]
VOCAB = 1000


def _cfg(**kw):
    return BertConfig(vocab_size=VOCAB, hidden=128, layers=2, heads=2,
                      intermediate=256, max_seq=64, **kw)


def _padded_batch():
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(1, VOCAB, (B, S), generator=g)
    typ = torch.randint(0, 2, (B, S), generator=g)
    mask = (torch.arange(S)[None] < torch.tensor(LENS)[:, None]).long()
    labels = torch.where(torch.rand(B, S, generator=g) < 0.3,
                         torch.randint(0, VOCAB, (B, S), generator=g),
                         torch.full((B, S), -100))
    labels = torch.where(mask.bool(), labels, torch.full((B, S), -100))
    labels[2, 0] = 7  # the shortest sequence has a label for certain
    nsp = torch.tensor([1, 0, 1])
    return ids, typ, mask, labels, nsp


def test_pack_padded_batch_round_trips():
    ids, typ, mask, labels, _ = _padded_batch()
    pk = pack_padded_batch(ids, typ, mask, labels, token_budget=80,
                           max_sequences=5)
    assert pk.cu_seqlens.dtype == torch.int32
    assert pk.cu_seqlens.tolist() == [0, 48, 65, 70, 70, 70]
    assert pk.max_seqlen == 48
    for t in (pk.ids, pk.type_ids, pk.position_ids, pk.mlm_labels):
        assert t.shape == (1, 80)
    cu = pk.cu_seqlens.tolist()
    for b, n in enumerate(LENS):
        sl = slice(cu[b], cu[b + 1])
        assert torch.equal(pk.ids[0, sl], ids[b, :n])
        assert torch.equal(pk.type_ids[0, sl], typ[b, :n])
        assert torch.equal(pk.mlm_labels[0, sl], labels[b, :n])
        assert torch.equal(pk.position_ids[0, sl], torch.arange(n))
    # the tail: id 0, position 0, label -100
    assert (pk.ids[0, 70:] == 0).all() and (pk.type_ids[0, 70:] == 0).all()
    assert (pk.position_ids[0, 70:] == 0).all()
    assert (pk.mlm_labels[0, 70:] == -100).all()


def test_pack_padded_batch_defaults_and_optional_fields():
    ids, _, mask, _, _ = _padded_batch()
    pk = pack_padded_batch(ids, None, mask, None)
    assert pk.ids.shape == (1, 70) and pk.type_ids is None
    assert pk.mlm_labels is None
    assert pk.cu_seqlens.tolist() == [0, 48, 65, 70]


def test_pack_padded_batch_errors():
    ids, typ, mask, labels, _ = _padded_batch()
    with pytest.raises(ValueError, match="token_budget"):
        pack_padded_batch(ids, typ, mask, labels, token_budget=69)
    with pytest.raises(ValueError, match="max_seq"):
        pack_padded_batch(ids, typ, mask, labels, max_seq=47)
    with pytest.raises(ValueError, match="max_sequences"):
        pack_padded_batch(ids, typ, mask, labels, max_sequences=2)
    holes = mask.clone()
    holes[1, 3] = 0
    with pytest.raises(ValueError, match="prefix"):
        pack_padded_batch(ids, typ, holes, labels)
    pack_padded_batch(ids, typ, mask, labels, token_budget=70, max_seq=48)


def _loss_and_grads(model, *args, **kw):
    for p in model.parameters():
        p.grad = None
    loss = model(*args, **kw)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone()
                           for n, p in model.named_parameters()}


def test_packed_loss_and_gradients_match_padded():
    """MLM + NSP loss and every parameter gradient, fp32, no dropout:
    rtol 1e-4, atol 1e-6."""
    torch.manual_seed(3)
    model = BertForPreTraining(_cfg()).train()
    ids, typ, mask, labels, nsp = _padded_batch()
    loss_p, grads_p = _loss_and_grads(model, ids, typ, mask, labels, nsp)

    pk = pack_padded_batch(ids, typ, mask, labels, token_budget=80,
                           max_sequences=5, max_seq=model.cfg.max_seq)
    nsp_k = torch.tensor([1, 0, 1, -100, -100])  # empty slots are ignored
    loss_k, grads_k = _loss_and_grads(
        model, pk.ids, pk.type_ids, None, pk.mlm_labels, nsp_k,
        cu_seqlens=pk.cu_seqlens, max_seqlen=pk.max_seqlen,
        position_ids=pk.position_ids)

    torch.testing.assert_close(loss_k, loss_p, rtol=1e-4, atol=1e-6)
    assert grads_k.keys() == grads_p.keys()
    for n in grads_p:
        torch.testing.assert_close(grads_k[n], grads_p[n], rtol=1e-4,
                                   atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")
    assert any(g.abs().max() > 0 for g in grads_p.values())


def test_packed_logits_path_and_argument_errors():
    torch.manual_seed(4)
    model = BertForPreTraining(_cfg()).eval()
    ids, typ, mask, labels, _ = _padded_batch()
    pk = pack_padded_batch(ids, typ, mask, labels, token_budget=80,
                           max_sequences=5)
    kw = dict(cu_seqlens=pk.cu_seqlens, max_seqlen=pk.max_seqlen,
              position_ids=pk.position_ids)
    with torch.no_grad():
        mlm, nsp = model(pk.ids, pk.type_ids, **kw)
        mlm_p, nsp_p = model(ids, typ, mask)
    assert mlm.shape == (1, 80, VOCAB) and nsp.shape == (5, 2)
    torch.testing.assert_close(nsp[:3], nsp_p, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(mlm[0, 48:65], mlm_p[1, :17], rtol=1e-4,
                               atol=1e-5)
    with pytest.raises(ValueError, match="attn_mask"):
        model(pk.ids, pk.type_ids, torch.ones(1, 80), **kw)
    with pytest.raises(ValueError, match="max_seqlen"):
        model(pk.ids, pk.type_ids, cu_seqlens=pk.cu_seqlens, max_seqlen=65,
              position_ids=pk.position_ids)
    with pytest.raises(ValueError, match=r"\[1, T\]"):
        model(ids, typ, cu_seqlens=pk.cu_seqlens)
