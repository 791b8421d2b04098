"""The fp64 references of the fused BERT embedding block (the yardstick of
test_embed_ln_gpu.py) against torch autograd, rounding disabled. No GPU."""
import pytest
import torch
import torch.nn.functional as F

from mpi_operator_amd.ops import reference as ref

EPS = 1e-12


@pytest.mark.parametrize("with_type", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("with_keep", [False, True])
def test_reference_matches_torch_autograd(with_type, with_pos, with_keep):
    torch.manual_seed(11)
    B, S, N, V, P, TY = 3, 7, 24, 50, 9, 2
    f64 = dict(dtype=torch.float64)
    tok, pos, typ = (torch.randn(r, N, **f64).requires_grad_()
                     for r in (V, P, TY))
    ln_w = (torch.rand(N, **f64) + 0.5).requires_grad_()
    ln_b = torch.randn(N, **f64).requires_grad_()
    ids = torch.randint(0, V, (B, S))
    ids[0, :4] = 5  # a repeated row
    type_ids = torch.randint(0, TY, (B, S)) if with_type else None
    position_ids = torch.randint(0, P, (B, S)) if with_pos else None
    keep = torch.rand(B, S, N) > 0.3 if with_keep else None
    scale = 1.25 if with_keep else 1.0
    dy = torch.randn(B, S, N, **f64)

    p_idx = position_ids if with_pos else torch.arange(S).expand(B, S)
    x = F.embedding(ids, tok) + F.embedding(p_idx, pos)
    if with_type:
        x = x + F.embedding(type_ids, typ)
    want = F.layer_norm(x, (N,), ln_w, ln_b, EPS)
    if with_keep:
        want = want * keep * scale
    want.backward(dy)

    with torch.no_grad():
        y, s, mean, rstd = ref.embed_layer_norm_fwd(
            ids, tok, pos, typ, ln_w, ln_b, EPS, type_ids, position_ids, keep,
            scale)
        _, dtok, dpos, dtyp, dw, db = ref.embed_layer_norm_bwd(
            dy, ids, s, mean, rstd, ln_w, (V, P, TY), type_ids, position_ids,
            keep, scale)
    pairs = [(y, want), (dtok, tok.grad), (dpos, pos.grad), (dw, ln_w.grad),
             (db, ln_b.grad)]
    if with_type:
        pairs.append((dtyp, typ.grad))
    else:
        assert dtyp is None and typ.grad is None
    for got, exp in pairs:
        assert (got - exp).abs().max().item() <= 1e-12 * (1 + exp.abs().max().item())
