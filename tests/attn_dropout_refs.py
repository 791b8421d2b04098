"""Shared by test_attn_dropout_cpu.py and test_attn_dropout_gpu.py: the fp32
reference chain with a dropout mask inserted, and the one-hot inputs that
read a kernel's dropout mask out of its outputs exactly.

The read-outs use that P > 0 wherever the key is valid, so an output element
that is a single term P[i, j]·keep[i, j]·(nonzero) is nonzero iff keep[i, j]:

  forward  V_w[j, d] = (j == 64w + d)   ->  ctx_w[i, d] != 0  <=>  keep[i, 64w+d]
  dK/dV    dO_w[i, d] = (i == 64w + d)  ->  dV_w[j, d]  != 0  <=>  keep[64w+d, j]
  dQ       K_w[j, d] = (j == 64w + d), ctx = 0 (delta = 0), lse = 0, small Q
           ->  dQ_w[i, d] = rs·keep·(dO·V^T)[i, 64w+d]·P·scale, nonzero iff
           keep, unless (dO·V^T)[i, 64w+d] itself rounds to 0
for each 64-column window w < ceil(S/64). `fwd`, `bwd` below are callables
over (qkv, ...) so the same read-out drives the CPU reference and the GPU
kernels.
"""
import torch

D = 64
SCALE = 0.125
FMIN = torch.finfo(torch.float32).min


def key_mask(S, valid, device):
    mask = torch.zeros(len(valid), S, device=device)
    for b, n in enumerate(valid):
        mask[b, n:] = FMIN
    return mask


def inputs(B, H, S, device):
    """qkv and the output cotangent of test_flash_attention_gpu._case (same
    seeds and scaling), drawn on the CPU so both test files see one input."""
    g = torch.Generator().manual_seed(1000 + S)
    qkv = (torch.randn(B, S, 3, H, D, generator=g) * 0.5).to(torch.bfloat16)
    gout = torch.randn(B, S, H * D, generator=g).to(torch.bfloat16)
    return qkv.to(device), gout.to(device)


def chain(qkv, gout, mask, keep, rs, dtype=torch.float32):
    """(out, dqkv, lse) of the plain autograd chain in `dtype` on the bf16
    inputs, with P replaced by rs·P∘keep (keep None: no dropout)."""
    B, S, _, H, _ = qkv.shape
    r = qkv.to(dtype).requires_grad_()
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if mask is not None:
        s = s + mask[:, None, None, :].to(dtype)
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep.to(dtype) * rs
    out = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D)
    out.backward(gout.to(dtype))
    lse = torch.logsumexp(s.detach(), dim=-1)
    return out.detach(), r.grad.detach(), lse


def windows(S):
    return range((S + 63) // 64)


def _onehot_rows(S, w, device):
    """[S, 64] bf16 with row 64w + d holding e_d."""
    e = torch.zeros(S, D, dtype=torch.bfloat16, device=device)
    n = min(D, S - 64 * w)
    idx = torch.arange(n, device=device)
    e[64 * w + idx, idx] = 1
    return e


def _valid_cols(mask, B, S, device):
    if mask is None:
        return torch.ones(B, S, dtype=torch.bool, device=device)
    return mask == 0


def read_fwd_mask(fwd, qkv, mask):
    """fwd(qkv) -> ctx [B,S,H*64]. Returns the bool [B,H,S,S] pattern
    keep & valid-key read from the forward's nonzeros."""
    B, S, _, H, _ = qkv.shape
    got = torch.zeros(B, H, S, S, dtype=torch.bool, device=qkv.device)
    for w in windows(S):
        x = qkv.clone()
        x[:, :, 2] = _onehot_rows(S, w, qkv.device)[None, :, None, :]
        ctx = fwd(x).reshape(B, S, H, D)
        n = min(D, S - 64 * w)
        got[:, :, :, 64 * w:64 * w + n] = (ctx[..., :n] != 0).permute(0, 2, 1, 3)
        assert (ctx[..., n:] == 0).all()
    return got


def read_dkv_mask(bwd, qkv, ctx, lse, mask):
    """bwd(qkv, ctx, dctx, lse) -> dqkv. Pattern from the nonzeros of dV."""
    B, S, _, H, _ = qkv.shape
    got = torch.zeros(B, H, S, S, dtype=torch.bool, device=qkv.device)
    for w in windows(S):
        do = _onehot_rows(S, w, qkv.device)[None, :, None, :].expand(B, S, H, D)
        dv = bwd(qkv, ctx, do.reshape(B, S, H * D).contiguous(), lse)[:, :, 2]
        n = min(D, S - 64 * w)
        # dv[b, j, h, d] <-> keep[b, h, 64w + d, j]
        got[:, :, 64 * w:64 * w + n, :] = (dv[..., :n] != 0).permute(0, 2, 3, 1)
        assert (dv[..., n:] == 0).all()
    return got


def read_dq_mask(bwd, qkv, gout, mask):
    """Pattern from the nonzeros of dQ with one-hot K, ctx = 0, lse = 0 and
    Q scaled by 2^-6 (P = exp(q·k·scale) stays within 2 % of 1). Returns
    (pattern, left_out): left_out marks valid elements whose dO·V^T term
    rounds to a bf16 zero, which no mask can be read from."""
    B, S, _, H, _ = qkv.shape
    dev = qkv.device
    got = torch.zeros(B, H, S, S, dtype=torch.bool, device=dev)
    zero_ctx = torch.zeros(B, S, H * D, dtype=torch.bfloat16, device=dev)
    zero_lse = torch.zeros(B, H, S, dtype=torch.float32, device=dev)
    small = qkv.clone()
    small[:, :, 0] = (small[:, :, 0].float() / 64).to(torch.bfloat16)
    for w in windows(S):
        x = small.clone()
        x[:, :, 1] = _onehot_rows(S, w, dev)[None, :, None, :]
        dq = bwd(x, zero_ctx, gout, zero_lse)[:, :, 0]
        n = min(D, S - 64 * w)
        got[:, :, :, 64 * w:64 * w + n] = (dq[..., :n] != 0).permute(0, 2, 1, 3)
        assert (dq[..., n:] == 0).all()
    do = gout.reshape(B, S, H, D).transpose(1, 2).float()
    v = qkv[:, :, 2].transpose(1, 2).float()
    dp = torch.matmul(do, v.transpose(-1, -2))
    # the smallest factor dS can carry next to dp: P >= exp(-1), scale, rs >= 1
    left = (dp * (SCALE * 0.36)).to(torch.bfloat16) == 0
    left &= _valid_cols(mask, B, S, dev)[:, None, None, :]
    return got, left
