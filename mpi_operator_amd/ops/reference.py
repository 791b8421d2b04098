"""Plain-PyTorch reference implementations of every hot op.

These serve two roles:
  1. CPU execution path (tests and bring-up run on CPU-only machines).
  2. fp32 golden model for the HIP-kernel numerics tests
     (tests compare the gfx950 kernels against these at fp32).

Shapes follow the framework's layout contract: activations are logical NCHW
(PyTorch convention) and, on GPU, channels-last in memory (NHWC); conv
weights are logical [K, C, R, S] and channels-last in memory ([K][R][S][C]).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def conv2d_fwd(x, w, stride: int, padding: int):
    return F.conv2d(x, w, bias=None, stride=stride, padding=padding)


def conv2d_dgrad(dy, w, x_shape, stride: int, padding: int):
    return torch.nn.grad.conv2d_input(x_shape, w, dy, stride=stride, padding=padding)


def conv2d_wgrad(x, dy, w_shape, stride: int, padding: int):
    return torch.nn.grad.conv2d_weight(x, w_shape, dy, stride=stride, padding=padding)


def bn_relu_fwd_train(x, gamma, beta, eps: float, relu: bool):
    """Returns (y, batch_mean, batch_invstd)."""
    dims = (0, 2, 3)
    xf = x.float()
    mean = xf.mean(dim=dims)
    var = xf.var(dim=dims, unbiased=False)
    invstd = (var + eps).rsqrt()
    xhat = (xf - mean[None, :, None, None]) * invstd[None, :, None, None]
    y = xhat * gamma.float()[None, :, None, None] + beta.float()[None, :, None, None]
    if relu:
        y = F.relu(y)
    return y.to(x.dtype), mean, invstd


def bn_relu_fwd_eval(x, gamma, beta, running_mean, running_var, eps: float, relu: bool):
    invstd = (running_var.float() + eps).rsqrt()
    scale = gamma.float() * invstd
    shift = beta.float() - running_mean.float() * scale
    y = x.float() * scale[None, :, None, None] + shift[None, :, None, None]
    if relu:
        y = F.relu(y)
    return y.to(x.dtype)


def bn_relu_bwd(dy, x, y, gamma, mean, invstd, relu: bool):
    """Returns (dx, dgamma, dbeta). ``y`` is the post-activation output
    (used for the ReLU mask); ``mean``/``invstd`` are the saved batch stats."""
    dims = (0, 2, 3)
    dyf = dy.float()
    if relu:
        dyf = dyf * (y.float() > 0)
    xf = x.float()
    xhat = (xf - mean[None, :, None, None]) * invstd[None, :, None, None]
    dbeta = dyf.sum(dim=dims)
    dgamma = (dyf * xhat).sum(dim=dims)
    n = x.numel() / x.shape[1]
    dx = (
        gamma.float()[None, :, None, None]
        * invstd[None, :, None, None]
        * (dyf - dbeta[None, :, None, None] / n - xhat * dgamma[None, :, None, None] / n)
    )
    return dx.to(dy.dtype), dgamma, dbeta


def max_pool2d_fwd(x, kernel: int, stride: int, padding: int):
    y, idx = F.max_pool2d(x, kernel, stride, padding, return_indices=True)
    return y, idx


def max_pool2d_bwd(dy, idx, x_shape, kernel: int, stride: int, padding: int):
    return F.max_unpool2d(dy, idx, kernel, stride, padding, output_size=x_shape[2:])


def global_avg_pool_fwd(x):
    return x.float().mean(dim=(2, 3)).to(x.dtype)


def global_avg_pool_bwd(dy, x_shape):
    n, c, h, w = x_shape
    return (dy.float() / (h * w))[:, :, None, None].expand(n, c, h, w).to(dy.dtype)


def linear_fwd(x, w, b):
    return F.linear(x, w, b)


def softmax_cross_entropy_fwd(logits, target):
    """Returns (loss_mean, softmax_probs) — probs saved for backward."""
    lf = logits.float()
    logp = F.log_softmax(lf, dim=-1)
    loss = F.nll_loss(logp, target)
    return loss, logp.exp()


def softmax_cross_entropy_bwd(probs, target, grad_scale: float):
    d = probs.clone()
    d[torch.arange(d.shape[0], device=d.device), target] -= 1.0
    return d * (grad_scale / d.shape[0])


def sgd_momentum_step(params32, grads32, momenta, bf16_outs, lr, momentum, weight_decay, nesterov=False):
    """fp32 master-weight SGD with momentum; writes updated fp32 masters and
    refreshed bf16 working copies in one pass (the HIP kernel fuses this)."""
    for p, g, m, out in zip(params32, grads32, momenta, bf16_outs):
        gf = g.float()
        if weight_decay:
            gf = gf.add(p, alpha=weight_decay)
        m.mul_(momentum).add_(gf)
        step = gf.add(m, alpha=momentum) if nesterov else m
        p.add_(step, alpha=-lr)
        if out is not None:
            out.copy_(p.to(out.dtype))


# Layout of the optimizers' per-group scalar block (8 fp32; slot 0 holds the
# int32 step count as a bit pattern) — mirrors csrc/optimizer.hip.
OPT_STEP, OPT_LR, OPT_BC1, OPT_BC2, OPT_CLIP = 0, 1, 2, 3, 4
OPT_SCALARS = 8


def optim_tick(scalars, grads, beta1, beta2, max_grad_norm=None):
    """Advance the scalar block by one step (the reference of optim_tick_k):
    step += 1, bias corrections in double, clip scale with
    torch.nn.utils.clip_grad_norm_ semantics. Returns (lr, bc1, bc2, clip)
    as Python floats — bc1/bc2 unrounded, as torch.optim computes them."""
    step_i = scalars.view(torch.int32)[OPT_STEP:OPT_STEP + 1]
    step_i += 1
    step = int(step_i)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    clip = 1.0
    if max_grad_norm:
        sq = sum(float(g.double().pow(2).sum()) for g in grads)
        clip = min(1.0, max_grad_norm / (sq ** 0.5 + 1e-6))
    scalars[OPT_BC1] = bc1
    scalars[OPT_BC2] = bc2
    scalars[OPT_CLIP] = clip
    return float(scalars[OPT_LR]), bc1, bc2, clip


def adamw_step(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs, scalars,
               beta1, beta2, eps, weight_decay, adam_w_mode=True,
               max_grad_norm=None):
    """torch.optim.AdamW (adam_w_mode) / torch.optim.Adam-with-L2 update on
    fp32 masters, in torch's operation order; refreshes bf16 working copies."""
    lr, bc1, bc2, clip = optim_tick(scalars, grads, beta1, beta2, max_grad_norm)
    for p, g, m, v, out in zip(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs):
        gf = g.float()
        if clip != 1.0:
            gf = gf * clip
        if adam_w_mode:
            p.mul_(1.0 - lr * weight_decay)
        elif weight_decay:
            gf = gf.add(p, alpha=weight_decay)
        m.lerp_(gf, 1.0 - beta1)
        v.mul_(beta2).addcmul_(gf, gf, value=1.0 - beta2)
        denom = (v.sqrt() / bc2 ** 0.5).add_(eps)
        p.addcdiv_(m, denom, value=-lr / bc1)
        if out is not None:
            out.copy_(p.to(out.dtype))


def lamb_step(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs, scalars,
              beta1, beta2, eps, weight_decay, adam_w_mode=True,
              max_grad_norm=None):
    """LAMB: Adam moments, u = m_hat / (sqrt(v_hat) + eps) + wd*w, per-tensor
    trust ratio ||w|| / ||u|| (1 if either norm is 0), w -= lr * ratio * u."""
    lr, bc1, bc2, clip = optim_tick(scalars, grads, beta1, beta2, max_grad_norm)
    for p, g, m, v, out in zip(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs):
        gf = g.float()
        if clip != 1.0:
            gf = gf * clip
        if not adam_w_mode and weight_decay:
            gf = gf.add(p, alpha=weight_decay)
        m.mul_(beta1).add_(gf, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(gf, gf, value=1.0 - beta2)
        u = (m / bc1) / ((v / bc2).sqrt() + eps)
        if adam_w_mode and weight_decay:
            u = u.add(p, alpha=weight_decay)
        nw, nu = float(p.norm()), float(u.norm())
        ratio = nw / nu if (nw > 0 and nu > 0) else 1.0
        p.add_(u, alpha=-lr * ratio)
        if out is not None:
            out.copy_(p.to(out.dtype))


def masked_softmax_cross_entropy_fwd(logits, target, ignore_index=-100):
    """fp32 golden oracle for the MLM masked CE (mean over valid rows)."""
    x = logits.float()
    mx = x.max(dim=1, keepdim=True).values
    e = (x - mx).exp()
    probs = e / e.sum(dim=1, keepdim=True)
    valid = target != ignore_index
    n = int(valid.sum().item())
    if n == 0:
        return x.new_zeros(()), probs
    lse = e.sum(dim=1).log() + mx.squeeze(1)
    picked = x[valid].gather(1, target[valid].unsqueeze(1)).squeeze(1)
    loss = (lse[valid] - picked).sum() / n
    return loss, probs


def masked_softmax_cross_entropy_bwd(probs, target, grad_scale: float,
                                     ignore_index=-100):
    valid = target != ignore_index
    n = max(int(valid.sum().item()), 1)
    d = probs.clone()
    rows = torch.arange(d.shape[0], device=d.device)
    d[rows[valid], target[valid]] -= 1.0
    d[~valid] = 0.0
    return d * (grad_scale / n)


def dgelu(x):
    """tanh-approx GELU derivative (fp32) — oracle for the fused FFN bwd."""
    xf = x.float()
    c = 0.7978845608028654
    u = c * (xf + 0.044715 * xf ** 3)
    t = torch.tanh(u)
    return 0.5 * (1 + t) + 0.5 * xf * (1 - t * t) * c * (1 + 3 * 0.044715 * xf * xf)


def _flash_scores(qkv, scale: float, mask):
    """fp32 scaled, masked scores [B,H,S,S] plus q, k, v as [B,H,S,D]."""
    q, k, v = (qkv[:, :, i].transpose(1, 2).float() for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s + mask.float().reshape(qkv.shape[0], 1, 1, qkv.shape[1])
    return s, q, k, v


def flash_attention_fwd(qkv, heads: int, scale: float, mask=None, keep=None,
                        drop_scale: float = 1.0):
    """Specification of flash_attn_fwd_k. qkv [B,S,3,H,D], mask [B,S]
    additive or None → (ctx [B,S,H·D] in qkv's dtype, lse [B,H,S] fp32).
    Keeps the per-row log-sum-exp, not the probabilities.
    keep (bool [B,H,S,S]) and drop_scale = 1/(1 - p_eff) apply dropout to
    the probabilities: ctx = drop_scale·(P∘keep)·V; lse is that of the
    undropped softmax."""
    B, S, _, H, D = qkv.shape
    assert H == heads
    s, _, _, v = _flash_scores(qkv, scale, mask)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        p = p * keep.to(p.dtype) * drop_scale
    ctx = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * D)
    return ctx.to(qkv.dtype), lse


def flash_attention_bwd(qkv, ctx, dctx, lse, scale: float, mask=None,
                        keep=None, drop_scale: float = 1.0):
    """Specification of the flash backward kernels: P is recomputed from
    lse and the softmax-gradient row term is delta = rowsum(dctx∘ctx);
    no saved probabilities. Returns dqkv [B,S,3,H,D].
    With keep / drop_scale (see flash_attention_fwd): dP = drop_scale·keep∘
    (dO·Vᵀ), dV = drop_scale·(P∘keep)ᵀ·dO, and delta is unchanged, since
    rowsum(dP∘P) = rowsum(dO∘O) still holds for the dropped O."""
    B, S, _, H, D = qkv.shape
    s, q, k, v = _flash_scores(qkv, scale, mask)
    p = torch.exp(s - lse.float().unsqueeze(-1))
    do = dctx.reshape(B, S, H, D).transpose(1, 2).float()
    o = ctx.reshape(B, S, H, D).transpose(1, 2).float()
    delta = (do * o).sum(-1, keepdim=True)
    dp = torch.matmul(do, v.transpose(-1, -2))
    pk = p
    if keep is not None:
        kf = keep.to(p.dtype) * drop_scale
        dp = dp * kf
        pk = p * kf
    ds = (dp - delta) * p * scale
    dv = torch.matmul(pk.transpose(-1, -2), do)
    dq = torch.matmul(ds, k)
    dk = torch.matmul(ds.transpose(-1, -2), q)
    dqkv = torch.stack(
        [dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)], dim=2)
    return dqkv.to(qkv.dtype)


def _varlen_bounds(cu_seqlens, total: int):
    """cu_seqlens → python ints, with the kernels' preconditions checked
    (the reference may read them on the host; the kernels never do)."""
    cu = [int(c) for c in cu_seqlens.tolist()]
    if len(cu) < 2 or cu[0] != 0 or cu[-1] > total or any(
            b < a for a, b in zip(cu, cu[1:])):
        raise ValueError(f"cu_seqlens must start at 0, not decrease and end "
                         f"at or below T={total}, got {cu}")
    return cu


def flash_attention_varlen_fwd(qkv, cu_seqlens, max_seqlen: int, heads: int,
                               scale: float, keep=None,
                               drop_scale: float = 1.0):
    """Specification of the packed (varlen) forward. qkv [T,3,H,D] holds
    N = len(cu_seqlens) − 1 sequences back to back, sequence n in rows
    cu[n]..cu[n+1]−1 → (ctx [T,H·D] in qkv's dtype, lse [H,T] fp32): each
    sequence is flash_attention_fwd of its own slice as a [1,L] batch, empty
    slots contribute nothing, rows at or past cu[N] are zeros.
    keep: optional list of N bool [H,L,L] masks (None for an empty slot),
    see varlen_attn_dropout_keep."""
    T, _, H, D = qkv.shape
    cu = _varlen_bounds(cu_seqlens, T)
    ctx = qkv.new_zeros(T, H * D)
    lse = torch.zeros(H, T, dtype=torch.float32, device=qkv.device)
    for n, (a, b) in enumerate(zip(cu, cu[1:])):
        if b == a:
            continue
        if b - a > max_seqlen:
            raise ValueError(f"sequence {n} has {b - a} > max_seqlen rows")
        kn = keep[n][None] if keep is not None else None
        c, l = flash_attention_fwd(qkv[a:b][None], heads, scale, None, kn,
                                   drop_scale)
        ctx[a:b], lse[:, a:b] = c[0], l[0]
    return ctx, lse


def flash_attention_varlen_bwd(qkv, ctx, dctx, lse, cu_seqlens,
                               max_seqlen: int, scale: float, keep=None,
                               drop_scale: float = 1.0):
    """Specification of the packed backward: flash_attention_bwd per
    sequence slice. Returns dqkv [T,3,H,D], zeros at or past cu[N]."""
    T, _, H, D = qkv.shape
    cu = _varlen_bounds(cu_seqlens, T)
    dqkv = torch.zeros_like(qkv)
    for n, (a, b) in enumerate(zip(cu, cu[1:])):
        if b == a:
            continue
        kn = keep[n][None] if keep is not None else None
        dqkv[a:b] = flash_attention_bwd(
            qkv[a:b][None], ctx[a:b][None], dctx[a:b][None],
            lse[:, a:b][None], scale, None, kn, drop_scale)[0]
    return dqkv


# ---------------------------------------------------------------- dropout
# The random-number scheme of csrc/philox.h, bit for bit, on the CPU.
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 from its definition. counter: four uint32 values or
    equal-shaped arrays, key: two uint32 values → the four output words as
    uint32 arrays. 64-bit products in numpy uint64 (M0*c0 overflows int64)."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        hi0, lo0 = p0 >> s32, p0 & m32
        hi1, lo1 = p1 >> s32, p1 & m32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + PHILOX_W0) & 0xFFFFFFFF  # the key is bumped after each round
        k1 = (k1 + PHILOX_W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def dropout_threshold(p: float):
    """p → (thr, p_eff, scale): thr = round(p·65536) of the 16-bit draw,
    p_eff = thr/65536, scale = 1/(1 - p_eff) rounded once to fp32.
    ValueError outside 0 <= p < 1 or where thr would reach 65536."""
    import numpy as np
    if not (0.0 <= p < 1.0):
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    thr = int(round(p * 65536.0))
    if thr > 65535:
        raise ValueError(f"dropout probability {p} rounds to 1 (thr = {thr})")
    p_eff = thr / 65536.0
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p_eff)))
    return thr, p_eff, scale


def philox_dropout_mask(seed: int, offset: int, site: int, shape, p: float):
    """The keep mask (True = kept) the dropout kernels draw for a contiguous
    tensor of `shape`: key (seed_lo, seed_hi), counter (octet, site,
    offset_lo, offset_hi) with octet = flat index // 8; element j of the
    octet takes r_j = (w[j >> 1] >> 16·(j & 1)) & 0xffff, kept iff r_j >= thr."""
    import numpy as np
    thr, _, _ = dropout_threshold(p)
    n = 1
    for d in shape:
        n *= int(d)
    if n % 8 or n // 8 >= 1 << 32:
        raise ValueError(f"element count {n} must be a multiple of 8 below 2^35")
    if not 0 <= site < 1 << 32:
        raise ValueError(f"site {site} does not fit a uint32")
    seed &= (1 << 64) - 1
    offset &= (1 << 64) - 1
    octet = np.arange(n // 8, dtype=np.uint64)
    w = philox4x32_10(
        (octet, site, offset & 0xFFFFFFFF, offset >> 32),
        (seed & 0xFFFFFFFF, seed >> 32))
    r = np.empty((n // 8, 8), dtype=np.uint32)
    for j in range(8):
        r[:, j] = (w[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF)
    keep = r >= np.uint32(thr)
    return torch.from_numpy(keep.reshape(tuple(int(d) for d in shape)))


def attn_dropout_call_slot(B: int, H: int, S: int):
    """(call, slot), int64 [B·H, S, S] each: the Philox call (counter word 0)
    and the 16-bit slot 0..7 within it that element (bh, i, j) of the
    attention probabilities draws from — csrc/philox.h's attention scheme:
    u = i & 15, band = i >> 4, half = (u >> 2) & 1,
    slot = (u & 3) + 4·(u >> 3), NB = ceil(S/16),
    call = ((bh·NB + band)·2 + half)·S + j."""
    import numpy as np
    nb = (S + 15) // 16
    if B < 1 or H < 1 or S < 1 or B * H * nb * 2 * S >= 1 << 32:
        raise ValueError(f"B·H·ceil(S/16)·2·S must be in [1, 2^32), got "
                         f"B={B} H={H} S={S}")
    bh = np.arange(B * H, dtype=np.int64)[:, None, None]
    i = np.arange(S, dtype=np.int64)[None, :, None]
    j = np.arange(S, dtype=np.int64)[None, None, :]
    u = i & 15
    band, half = i >> 4, (u >> 2) & 1
    slot = (u & 3) + 4 * (u >> 3)
    call = ((bh * nb + band) * 2 + half) * S + j
    return call, np.broadcast_to(slot, call.shape)


def attn_dropout_keep(seed: int, offset: int, site: int, B: int, H: int,
                      S: int, p: float):
    """The keep mask (True = kept), bool [B,H,S,S], that the attention
    kernels draw for the softmax output of a [B,S,3,H,64] qkv: key (seed_lo,
    seed_hi), counter (call, site, offset_lo, offset_hi) with call and slot of
    attn_dropout_call_slot; r = (w[slot >> 1] >> 16·(slot & 1)) & 0xffff,
    kept iff r >= thr."""
    import numpy as np
    thr, _, _ = dropout_threshold(p)
    if not 0 <= site < 1 << 32:
        raise ValueError(f"site {site} does not fit a uint32")
    seed &= (1 << 64) - 1
    offset &= (1 << 64) - 1
    call, slot = attn_dropout_call_slot(B, H, S)
    # one evaluation per distinct call: [B·H·NB·2·S]
    nb = (S + 15) // 16
    w = philox4x32_10(
        (np.arange(B * H * nb * 2 * S, dtype=np.uint64), site,
         offset & 0xFFFFFFFF, offset >> 32),
        (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(w, axis=-1)  # [calls, 4]
    word = w[call, slot >> 1]
    r = (word >> (16 * (slot & 1)).astype(np.uint32)) & np.uint32(0xFFFF)
    keep = r >= np.uint32(thr)
    return torch.from_numpy(np.ascontiguousarray(keep.reshape(B, H, S, S)))


def varlen_attn_dropout_keep(seed: int, offset: int, site: int, cu_seqlens,
                             H: int, max_seqlen: int, p: float):
    """The keep masks of a packed (varlen) batch: a list of N bool [H,L,L]
    tensors (None for an empty slot). csrc/philox.h keys sequence n as batch
    row n of a dense [N, max_seqlen] batch with rows and columns counted
    within the sequence, so mask n is
    attn_dropout_keep(seed, offset, site, N, H, max_seqlen, p)[n, :, :L, :L]."""
    cu = [int(c) for c in cu_seqlens.tolist()]
    N = len(cu) - 1
    lens = [b - a for a, b in zip(cu, cu[1:])]
    if max(lens) > max_seqlen:
        raise ValueError(f"a sequence is longer than max_seqlen={max_seqlen}")
    dense = attn_dropout_keep(seed, offset, site, N, H, max_seqlen, p)
    return [dense[n, :, :L, :L].clone() if L else None
            for n, L in enumerate(lens)]
