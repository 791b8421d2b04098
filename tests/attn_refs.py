"""fp64 references, per-element bounds, input families and key masks of the
attention edge tests (test_attn_edges_gpu.py on the GPU, test_attn_refs_cpu.py
for the harness itself). Plain torch on the CPU, in the style of conv_refs.py;
comparison is stream_refs.check_close with rel = 0 and a per-element bound.

Visibility. Key j is visible to row i of batch row b when j < S, mask[b, j] >
-1e30 (a smaller value excludes the key exactly; a larger finite one such as
-10000 is ADDED to the score) and, under causal, j <= i. Exclusion is by
selection (masked_fill(-inf)), never by adding finfo.min. A row with no
visible key has P = 0, ctx = 0, contributes nothing to any gradient, and its
lse is the kernels' running-max floor FLOOR, to the bit.

Forward reference: s, P = softmax(s), O = P·V and lse in fp64 from the bf16
inputs. Backward reference: the fp64 evaluation of the specification
reference.flash_attention_bwd on the kernel's OWN ctx (bf16) and lse (fp32):
    P = exp(s - lse), delta = rowsum(dO∘ctx), dP = dO·Vᵀ (dropout: ∘keep·rs),
    dS = (dP - delta)∘P·scale, dV = (P∘keep·rs)ᵀ·dO, dK = dSᵀ·Q, dQ = dS·K.
delta is taken from the rounded ctx by design, so a comparison with fp64
autograd would have to allow for that rounding, which alone exceeds |dQ| on
one-hot rows; against the specification the bound stays a few % of |ref|, and
end-to-end correctness follows from this check plus the forward check.

Bounds, per element. u = 2^-8 (REL_BF16: one rounding to bf16), w = 2^-12
(fp32 sum order, the fast exp, second-order terms: each below 1e-5 relative),
and r_ij = u + w + x_ij the relative error of one parked P_ij, where
    x_ij = 2^-23·|s_ij| + 2^-24·|lse_i|
is what the fp32 roundings of the exponent s·scale + mask - m (or - lse) do to
exp: 4e-6 at |s| <= 32, but 1.8e-3 on a row whose every key carries a -10000
mask, which the issue's u' = u + w alone would not cover. The kernels
(flash_attention.hip and, read for this, flash_attention_d128.hip: the same
quantities in both) round to bf16 the unnormalized P parked for P·V, P and dS
in the backward's recompute, and each output:

    ctx : u·|O|  + Σ_j r_ij·Pk_ij·|v_jd|            Pk = P (dropout: P∘keep·rs)
    dV  : u·|dV| + Σ_i r_ij·Pk_ij·|dO_id|
    dQ  : u·|dQ| + Σ_j e_ij·|k_jd|
    dK  : u·|dK| + Σ_i e_ij·|q_id|
    e_ij = r_ij·|dS_ij| + D·2^-24·(Σ_d|dO_id·ctx_id| + Σ_d|dO_id·v_jd|·kr_ij)
                          ·P_ij·scale
The second term of e_ij is the fp32 sums of delta and, added here to the
issue's derivation because it cancels against delta just the same, of dP
(kr = keep·rs under dropout, else 1). An element no visible term reaches has
a bound of 0 and must be exactly 0.

lse : D·2^-24·scale·max_j Σ_d|q_id·k_jd| + 2^-22·|ref| + LSE_C, where LSE_C
stands for the hardware's fast exp / log and is 4 x the worst |lse - ref|
measured on the GPU (test_attn_edges_gpu.py records the measurement). Where
every visible |s| <= 32 the bound is capped at LSE_CAP = 1e-4: the worst-case
first term alone passes that on the sharp inputs (about 2e-4 at D = 128:
128·2^-24·scale·Σ_d|q·k| with Σ_d|q·k| near 330), and a
score rounded to bf16, off by 4e-3·|s|, is the bug this check has to separate
from noise. The cap only ever tightens the bound.

Fused attention (attention.hip, read for this): the forward normalizes P in
fp32 and parks / saves bf16(P), so ctx has the flash bound and the saved
probs |probs - P| <= r_ij·P_ij. Its backward reads the saved probs Ps as an
exact input; the specification on them is
    dP = dO·Vᵀ, t = rowsum(dP∘Ps), dS = (dP - t)∘Ps·scale,
    dV = Psᵀ·dO, dK = dSᵀ·Q, dQ = dS·K
with only dS and the outputs rounded:
    dV  : u·|dV| + w·Σ_i Ps_ij·|dO_id|
    e_ij = (u + w)·|dS_ij| + (D·2^-24·Σ_d|dO_id·v_jd| + S·2^-24·T_i
           + c·u·(|dP_ij| + T_i))·Ps_ij·scale,       T_i = Σ_j|dP_ij|·Ps_ij
c = 0 for the fused kernel (S = 128), 1 for the torch chain of every other S,
whose dP matmul returns bf16. A row with no visible key gets P = 0 from
both (the kernel selects 1/sum = 0 where the sum is 0).
"""
import functools

import torch

from stream_refs import REL_BF16, WORST, check_close

U = REL_BF16
W = 2.0 ** -12
U32 = 2.0 ** -24
VISIBLE_ABOVE = -1e30
FMIN = torch.finfo(torch.float32).min
# FA_FLOOR of csrc/flash_common.h as the fp32 it is
FLOOR = float(torch.tensor(-3.4e38, dtype=torch.float32))
LSE_CAP = 1e-4
# 4 x 6.14e-6, the worst |lse - ref| over every case of test_attn_edges_gpu.py
# whose visible scores stay within |s| <= 32 (see that module's docstring)
LSE_C = 2.46e-5

FAMILIES = ("soft", "sharp", "ramp_up", "ramp_down")
MASK_KINDS = ("tail", "head", "hole", "tile", "empty")
MASK_VALUES = (FMIN, float("-inf"), -10000.0)
# ramp amplitude per head dim: scale·4·A = 28 (D = 64), 28.3 (D = 128), so
# the 40-key last tile of S = 296 still climbs 3.8 over its predecessor
RAMP_A = {64: 56.0, 128: 80.0}


def scale_of(D):
    return D ** -0.5


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(family, B, H, S, D):
    """(qkv [B,S,3,H,D], gout [B,S,H·D]) bf16 on the CPU, seeded by S. `soft`
    is attn_dropout_refs.inputs (D = 64: the same numbers). Cached: treat
    the result as read-only."""
    g = torch.Generator().manual_seed(1000 + S)
    x = torch.randn(B, S, 3, H, D, generator=g) * 0.5
    gout = torch.randn(B, S, H * D, generator=g).to(torch.bfloat16)
    if family == "sharp":
        x[:, :, :2] *= 4  # q, k ~ randn·2
    elif family in ("ramp_up", "ramp_down"):
        j = torch.arange(S, dtype=torch.float32)
        if family == "ramp_down":
            j = S - 1 - j
        x[:, :, 0, :, 0] = 4
        x[:, :, 1, :, 0] = (RAMP_A[D] * j / S)[None, :, None]
    else:
        assert family == "soft", family
    return x.to(torch.bfloat16), gout


def key_mask(kind, S, value, B=2):
    """[B, S] fp32 additive mask; the two batch rows differ."""
    m = torch.zeros(B, S)
    if kind == "tail":
        m[1, S - max(1, S // 8):] = value
    elif kind == "head":  # a whole first tile plus 2
        m[0, :130] = value
        m[1, :130] = value
        m[1, S - 3:] = value
    elif kind == "hole":  # across the tile edge, plus the last keys
        lo, hi = (100, 140) if S >= 160 else (S // 3, S // 3 + S // 8 + 1)
        m[0, lo:hi] = value
        m[1, lo + 1:hi + 1] = value
        m[:, S - min(6, S // 4):] = value
    elif kind == "tile":  # a whole interior tile
        assert S >= 257
        m[0, 128:256] = value
        m[1, 128:257] = value
    elif kind == "empty":
        m[1, :] = value
    else:
        raise ValueError(kind)
    return m


def visible(mask, B, S, causal):
    """bool [B, 1, S, S]."""
    vis = torch.ones(B, 1, S, S, dtype=torch.bool)
    if mask is not None:
        vis = vis & (mask > VISIBLE_ABOVE)[:, None, None, :]
    if causal:
        vis = vis & torch.ones(S, S, dtype=torch.bool).tril()
    return vis


# -------------------------------------------------------------- references
def _heads(t, B, S, H, D):
    return t.detach().cpu().reshape(B, S, H, D).transpose(1, 2).to(torch.float64)


def _rows(t):  # [B,H,S,D] -> [B,S,H·D]
    B, H, S, D = t.shape
    return t.transpose(1, 2).reshape(B, S, H * D)


def _scores(qkv, scale, mask, causal):
    B, S, _, H, D = qkv.shape
    x = qkv.detach().cpu()
    q, k, v = (x[:, :, i].transpose(1, 2).to(torch.float64) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    sabs = torch.matmul(q.abs(), k.abs().transpose(-1, -2)) * scale
    vis = visible(mask, B, S, causal)
    if mask is not None:
        add = torch.where(mask > VISIBLE_ABOVE, mask, torch.zeros_like(mask))
        s = s + add.to(torch.float64)[:, None, None, :]
    vis = vis.expand(B, H, S, S)
    s = s.masked_fill(~vis, float("-inf"))
    return s, sabs, vis, q, k, v


def fwd_ref(qkv, scale, mask=None, causal=False, keep=None, rs=1.0):
    """Every forward reference and bound of one case, as a dict:
    ctx, ctx_abs [B,S,H·D]; lse, lse_abs [B,H,S] (FLOOR and 0 on the rows
    with no visible key); P [B,H,S,S] and its relative error r; empty
    [B,H,S] bool; small: every visible |s| <= 32."""
    B, S, _, H, D = qkv.shape
    s, sabs, vis, q, k, v = _scores(qkv, scale, mask, causal)
    empty = ~vis.any(-1)
    lse = torch.logsumexp(s, -1)
    lse = torch.where(empty, torch.full_like(lse, FLOOR), lse)
    P = torch.where(vis, (s - lse[..., None]).exp(), torch.zeros_like(s))
    sv = torch.where(vis, s, torch.zeros_like(s))
    r = U + W + 2 * U32 * sv.abs() + U32 * lse.abs()[..., None] * ~empty[..., None]
    Pk = P if keep is None else P * keep.cpu().to(torch.float64) * rs
    O = torch.matmul(Pk, v)
    ctx_abs = U * O.abs() + torch.matmul(r * Pk, v.abs())
    small = bool((sv.abs() <= 32).all())
    lse_abs = (D * U32 * sabs.masked_fill(~vis, 0.0).amax(-1)
               + 2.0 ** -22 * lse.abs() + LSE_C)
    if small:
        lse_abs = lse_abs.clamp_max(LSE_CAP)
    lse_abs = torch.where(empty, torch.zeros_like(lse_abs), lse_abs)
    return dict(ctx=_rows(O), ctx_abs=_rows(ctx_abs), lse=lse, lse_abs=lse_abs,
                P=P, r=r, empty=empty, small=small, vis=vis)


def bwd_ref(qkv, gout, ctx, lse, scale, mask=None, causal=False, keep=None,
            rs=1.0):
    """The flash backward specification in fp64 on the kernel's own ctx and
    lse: dict(dq, dq_abs, dk, dk_abs, dv, dv_abs), each [B,S,H,D]."""
    B, S, _, H, D = qkv.shape
    s, _, vis, q, k, v = _scores(qkv, scale, mask, causal)
    l = lse.detach().cpu().to(torch.float64)[..., None]
    P = torch.where(vis, (s - l).exp(), torch.zeros_like(s))
    sv = torch.where(vis, s, torch.zeros_like(s))
    r = U + W + 2 * U32 * sv.abs() + U32 * l.abs() * vis.any(-1, keepdim=True)
    do, o = _heads(gout, B, S, H, D), _heads(ctx, B, S, H, D)
    kr = torch.ones(()) if keep is None else keep.cpu().to(torch.float64) * rs
    delta = (do * o).sum(-1, keepdim=True)
    dP = torch.matmul(do, v.transpose(-1, -2)) * kr
    dS = (dP - delta) * P * scale
    Pk = P * kr
    e = r * dS.abs() + D * U32 * (
        (do * o).abs().sum(-1, keepdim=True)
        + torch.matmul(do.abs(), v.abs().transpose(-1, -2)) * kr) * P * scale
    dv = torch.matmul(Pk.transpose(-1, -2), do)
    dq, dk = torch.matmul(dS, k), torch.matmul(dS.transpose(-1, -2), q)
    out = dict(
        dv=dv, dv_abs=U * dv.abs() + torch.matmul((r * Pk).transpose(-1, -2), do.abs()),
        dq=dq, dq_abs=U * dq.abs() + torch.matmul(e, k.abs()),
        dk=dk, dk_abs=U * dk.abs() + torch.matmul(e.transpose(-1, -2), q.abs()))
    return {n: t.transpose(1, 2) for n, t in out.items()}


def fused_bwd_ref(qkv, gout, probs, scale, torch_chain):
    """The fused attention backward specification in fp64 on the kernel's
    own saved probs [B,H,S,S] (module docstring). torch_chain: the S != 128
    route, whose dP is rounded to bf16."""
    B, S, _, H, D = qkv.shape
    x = qkv.detach().cpu()
    q, k, v = (x[:, :, i].transpose(1, 2).to(torch.float64) for i in range(3))
    Ps = probs.detach().cpu().to(torch.float64)
    do = _heads(gout, B, S, H, D)
    dP = torch.matmul(do, v.transpose(-1, -2))
    T = (dP.abs() * Ps).sum(-1, keepdim=True)
    dS = (dP - (dP * Ps).sum(-1, keepdim=True)) * Ps * scale
    c = 1.0 if torch_chain else 0.0
    e = (U + W) * dS.abs() + (
        D * U32 * torch.matmul(do.abs(), v.abs().transpose(-1, -2))
        + S * U32 * T + c * U * (dP.abs() + T)) * Ps * scale
    dv = torch.matmul(Ps.transpose(-1, -2), do)
    dq, dk = torch.matmul(dS, k), torch.matmul(dS.transpose(-1, -2), q)
    out = dict(
        dv=dv, dv_abs=U * dv.abs() + W * torch.matmul(Ps.transpose(-1, -2), do.abs()),
        dq=dq, dq_abs=U * dq.abs() + torch.matmul(e, k.abs()),
        dk=dk, dk_abs=U * dk.abs() + torch.matmul(e.transpose(-1, -2), q.abs()))
    return {n: t.transpose(1, 2) for n, t in out.items()}


# ------------------------------------------------------------- comparison
def compare(tag, got, ref, names):
    """[(name, ok, worst ratio, message)] of got[n] against ref[n] within
    ref[n + '_abs'], every element of every tensor."""
    res = []
    for n in names:
        ok, worst, msg = check_close(got[n].detach().cpu(), ref[n], 0.0,
                                     ref[n + "_abs"], f"{tag}.{n}")
        res.append((n, ok, worst, msg))
    return res


def assert_all(family, results):
    """Record the worst ratio per (kernel family, output) in
    stream_refs.WORST, print them, and fail on the first bound missed."""
    for n, ok, worst, msg in results:
        key = f"{family}.{n}"
        WORST[key] = max(WORST.get(key, 0.0), worst)
        print(f"RATIO {msg.split(':')[0]} {worst:.4f}")
    for n, ok, worst, msg in results:
        assert ok, msg


def split_dqkv(dqkv):
    return dict(dq=dqkv[:, :, 0], dk=dqkv[:, :, 1], dv=dqkv[:, :, 2])


def check_flash(tag, family, qkv, gout, scale, mask, causal, ctx, lse, dqkv,
                keep=None, rs=1.0):
    """The whole per-case check of a flash forward + backward: ctx, lse, dq,
    dk, dv each against its own bound (an element with bound 0 — masked keys'
    dK / dV, everything of a row with no visible key, that row's lse against
    FLOOR — must match exactly; a NaN or Inf fails any bound). Returns the
    result list of compare() and the forward reference."""
    f = fwd_ref(qkv, scale, mask, causal, keep, rs)
    res = compare(tag, dict(ctx=ctx, lse=lse), f, ("ctx", "lse"))
    b = bwd_ref(qkv, gout, ctx, lse, scale, mask, causal, keep, rs)
    res += compare(tag, split_dqkv(dqkv), b, ("dq", "dk", "dv"))
    return res, f
