"""fp64 references and the per-element comparator of the streaming-kernel
tests (test_stream_kernels_gpu.py on the GPU, test_stream_refs_cpu.py for the
references themselves). Everything here is plain torch and device-agnostic:
each builder computes on the device of its inputs.

Comparison is per element,  |out - ref| <= rel*|ref| + abs_i,  where abs_i is
a tensor built from the magnitudes of the terms of that element's expression
(what cancellation can expose). The three scales used:

  REL_BF16 = 2^-8   one rounding of an fp32 value to bf16 (half a bf16 ulp
                    relative to the value at the bottom of its binade)
  ABS_TERM = 2^-16  x sum|terms|: 256 fp32 ulps of the terms that cancel
  STAT     = 2^-18  x sum|summands| for an fp32 sum whose chain is <= ~600
                    adds deep (2^-24 * sqrt(600) ~ 2^-19.4, plus one bit)
"""
import torch

REL_BF16 = 2.0 ** -8
ABS_TERM = 2.0 ** -16
STAT = 2.0 ** -18
REL_F32 = 2.0 ** -22  # a few fp32 ulps: a handful of fused multiply-adds

# worst observed |out-ref| / bound per name, filled by assert_close
WORST = {}


def bf16r(t):
    """Round to bf16 (the kernels' input precision); stays bf16."""
    return t.to(torch.bfloat16)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _bc(t, ref):
    if torch.is_tensor(t):
        return t.to(torch.float64).to(ref.device).expand_as(ref)
    return torch.full_like(ref, float(t))


def check_close(out, ref, rel, abs_i, name):
    """Returns (ok, worst_ratio, message). ratio = |out-ref| / bound per
    element (0 where both are 0, inf where only the bound is)."""
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    o = out.detach().to(torch.float64)
    r = ref.detach().to(torch.float64).to(o.device)
    err = (o - r).abs()
    bound = rel * r.abs() + _bc(abs_i, r)
    # a non-finite output is never within a bound
    err = torch.where(torch.isfinite(o), err, torch.full_like(err, float("inf")))
    bad = ~(err <= bound)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    if ratio.numel() == 0:
        return True, 0.0, f"{name}: empty"
    flat = int(torch.argmax(torch.nan_to_num(ratio, nan=float("inf"))))
    worst = float(ratio.reshape(-1)[flat])
    nbad = int(bad.sum())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)) \
        if ratio.dim() else ()
    msg = (f"{name}: {nbad} of {ratio.numel()} elements out of bound; worst at "
           f"{idx}: out={float(o.reshape(-1)[flat])!r} ref={float(r.reshape(-1)[flat])!r} "
           f"err={float(err.reshape(-1)[flat]):.3e} "
           f"bound={float(bound.reshape(-1)[flat]):.3e} ratio={worst:.3f}")
    return nbad == 0, worst, msg


def assert_close(out, ref, rel, abs_i, name):
    ok, worst, msg = check_close(out, ref, rel, abs_i, name)
    key = name.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"RATIO {name} {worst:.4f}")
    assert ok, msg


def assert_equal(out, ref, name):
    """Bit-exact comparison with the same failure report."""
    assert out.shape == ref.shape and out.dtype == ref.dtype, (
        name, out.shape, ref.shape, out.dtype, ref.dtype)
    r = ref.to(out.device)
    if torch.equal(out, r):
        return
    bad = out != r
    if out.dtype.is_floating_point:  # -0 == +0 above; report sign flips too
        bad |= torch.signbit(out) != torch.signbit(r)
    nbad = int(bad.sum())
    assert nbad > 0, f"{name}: torch.equal is False but no element differs"
    err = (out.to(torch.float64) - r.to(torch.float64)).abs()
    err = torch.where(bad, err, torch.zeros_like(err))
    flat = int(torch.argmax(err))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), err.shape))
    raise AssertionError(
        f"{name}: {nbad} of {out.numel()} elements differ; worst at {idx}: "
        f"out={out.reshape(-1)[flat].item()!r} ref={r.reshape(-1)[flat].item()!r}")


# ------------------------------------------------------------------ inputs
def bn_input(shape, offset=True, seed=0, device="cpu"):
    """x = 3*U(-1,1) + offset_c, per-channel offsets spread over [-16, 16]
    (mean^2/var reaches ~80: E[x^2] - mean^2 is actually exercised), or the
    zero-mean 3*U(-1,1) alone. bf16, channels_last."""
    N, C, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.rand(N, C, H, W, generator=g) * 2 - 1) * 3
    if offset:
        off = torch.linspace(-16, 16, C)[torch.randperm(C, generator=g)]
        x = x + off[None, :, None, None]
    return cl(bf16r(x).to(device))


def rand_bf16(shape, seed, scale=1.0, shift=0.0, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = (torch.rand(*shape, generator=g) * 2 - 1) * scale + shift
    t = bf16r(t).to(device)
    return cl(t) if t.dim() == 4 else t


def pool_pattern(shape, shift=-125, device="cpu"):
    """x[n,c,h,w] = ((97h + 41w + 13c + 29n) mod 251) + shift: integers of
    magnitude <= 251, exact in bf16, and no two elements of one K<=3 window
    are equal (97*dr + 41*ds != 0 mod 251 for |dr|,|ds| <= 2), so the argmax
    of every window is unique. shift=-251 makes every value negative."""
    N, C, H, W = shape
    n = torch.arange(N, device=device)[:, None, None, None]
    c = torch.arange(C, device=device)[None, :, None, None]
    h = torch.arange(H, device=device)[None, None, :, None]
    w = torch.arange(W, device=device)[None, None, None, :]
    v = (97 * h + 41 * w + 13 * c + 29 * n) % 251 + shift
    return cl(v.to(torch.bfloat16))


# ------------------------------------------------------------------ masks
def pack_mask(pos):
    """[N,C,H,W] bool -> [M, C/8] uint8; bit j of byte [m, c8] is channel
    8*c8 + j of row m = (n, h, w)."""
    N, C, H, W = pos.shape
    p = pos.permute(0, 2, 3, 1).reshape(N * H * W, C // 8, 8).to(torch.int32)
    wts = (1 << torch.arange(8, device=pos.device, dtype=torch.int32))
    return (p * wts).sum(-1).to(torch.uint8)


def unpack_mask(mask, shape):
    """Inverse of pack_mask: [M, C/8] uint8 -> [N,C,H,W] bool."""
    N, C, H, W = shape
    bits = (mask.to(torch.int32)[..., None] >> torch.arange(
        8, device=mask.device, dtype=torch.int32)) & 1
    return bits.reshape(N, H, W, C).permute(0, 3, 1, 2).bool()


# ------------------------------------------------------------------ batchnorm
def _c(v):  # [C] -> broadcastable over [N,C,H,W]
    return v[None, :, None, None]


def bn_fwd_ref(x, gamma, beta, eps, relu, res, rm0, rv0, momentum):
    """fp64 training forward. Returns a dict of references and, under
    '<name>_abs', the absolute part of each bound (see module docstring)."""
    d = (0, 2, 3)
    xd = x.to(torch.float64)
    g, b = gamma.to(torch.float64), beta.to(torch.float64)
    M = xd.numel() // xd.shape[1]
    mean = xd.mean(d)
    ex2 = (xd * xd).mean(d)
    eabs = xd.abs().mean(d)
    var = ((xd - _c(mean)) ** 2).mean(d)
    invstd = (var + eps).rsqrt()
    scale = g * invstd
    shift = b - mean * scale
    y = xd * _c(scale) + _c(shift)
    y_abs = (xd * _c(scale)).abs() + _c(shift).abs()
    if res is not None:
        rd = res.to(torch.float64)
        y = y + rd
        y_abs = y_abs + rd.abs()
    if relu:
        y = y.clamp_min(0)
    unbias = M / (M - 1) if M > 1 else 1.0
    out = dict(M=M, y=y, y_abs=ABS_TERM * y_abs, mean=mean, var=var,
               invstd=invstd, mean_abs=STAT * eabs)
    # var = E[x^2] - mean^2: the two means' bounds, propagated to first order
    var_abs = STAT * (ex2 + 2 * mean.abs() * eabs)
    # conditioning of E[x^2] - mean^2, per channel, from the reference's own
    # mean and var; var == 0 (one row) leaves invstd = rsqrt(eps), which the
    # caller checks directly
    out["invstd_abs"] = invstd * STAT * (1 + mean * mean / var.clamp_min(1e-300))
    if rm0 is not None:
        r0, v0 = rm0.to(torch.float64), rv0.to(torch.float64)
        out["running_mean"] = r0 * (1 - momentum) + mean * momentum
        out["running_mean_abs"] = STAT * (r0.abs() * (1 - momentum) + eabs * momentum)
        out["running_var"] = v0 * (1 - momentum) + var * unbias * momentum
        out["running_var_abs"] = (STAT * v0.abs() * (1 - momentum)
                                  + var_abs * unbias * momentum)
    return out


def bn_eval_ref(x, gamma, beta, rm, rv, eps, relu):
    xd = x.to(torch.float64)
    invstd = (rv.to(torch.float64) + eps).rsqrt()
    scale = gamma.to(torch.float64) * invstd
    shift = beta.to(torch.float64) - rm.to(torch.float64) * scale
    y = xd * _c(scale) + _c(shift)
    y_abs = ABS_TERM * ((xd * _c(scale)).abs() + _c(shift).abs())
    return (y.clamp_min(0) if relu else y), y_abs


def bn_bwd_ref(dy, x, pos, gamma, mean, invstd):
    """fp64 backward from the kernel's own inputs (mean/invstd as saved by
    the forward). pos: [N,C,H,W] bool ReLU gate, or None without ReLU."""
    d = (0, 2, 3)
    dyd, xd = dy.to(torch.float64), x.to(torch.float64)
    if pos is not None:
        dyd = dyd * pos.to(dyd.device)
    g = gamma.to(torch.float64)
    mn, iv = mean.to(torch.float64), invstd.to(torch.float64)
    M = xd.numel() // xd.shape[1]
    xhat = (xd - _c(mn)) * _c(iv)
    dbeta = dyd.sum(d)
    dgamma = (dyd * xhat).sum(d)
    k1 = g * iv
    k2 = k1 * dbeta / M
    k3 = k1 * dgamma / M
    t1, t3 = _c(k1) * dyd, _c(k3) * xhat
    dx = t1 - _c(k2) - t3
    return dict(dx=dx, dx_abs=ABS_TERM * (t1.abs() + _c(k2).abs() + t3.abs()),
                dbeta=dbeta, dbeta_abs=STAT * dyd.abs().sum(d),
                dgamma=dgamma, dgamma_abs=STAT * (dyd * xhat).abs().sum(d))


# ------------------------------------------------------------------ max-pool
def pool_ref(x, dy, K, stride, pad):
    """torch's own max_pool2d in fp64 (the pattern has no ties, so its argmax
    is THE argmax). Returns y (bf16), idx = r*K + s as uint8 [N,HO,WO,C],
    dx fp64 from autograd and the sum of |dy| scattered the same way."""
    F = torch.nn.functional
    xd = x.to(torch.float64).contiguous().requires_grad_(True)
    y, flat = F.max_pool2d(xd, K, stride, pad, return_indices=True)
    N, C, HO, WO = y.shape
    W = x.shape[3]
    ho = torch.arange(HO, device=x.device)[None, None, :, None]
    wo = torch.arange(WO, device=x.device)[None, None, None, :]
    r = flat // W - (ho * stride - pad)
    s = flat % W - (wo * stride - pad)
    assert int(r.min()) >= 0 and int(r.max()) < K and int(s.min()) >= 0 and int(s.max()) < K
    idx = (r * K + s).permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    dx = dx_abs = None
    if dy is not None:
        dyd = dy.to(torch.float64).contiguous()
        dx, = torch.autograd.grad(y, xd, dyd, retain_graph=True)
        dx_abs, = torch.autograd.grad(y, xd, dyd.abs())
        dx_abs = ABS_TERM * dx_abs
    return cl(y.detach().to(torch.bfloat16)), idx, dx, dx_abs


def pool_scatter(dy, idx, x_shape, K, stride, pad):
    """dx from an argmax byte tensor (the kernel's idx layout), fp64: every
    window adds its dy at window position idx = r*K + s."""
    N, C, H, W = x_shape
    HO, WO = dy.shape[2], dy.shape[3]
    pos = idx.permute(0, 3, 1, 2).to(torch.int64)  # [N,C,HO,WO]
    ho = torch.arange(HO, device=dy.device)[None, None, :, None]
    wo = torch.arange(WO, device=dy.device)[None, None, None, :]
    h = ho * stride - pad + pos // K
    w = wo * stride - pad + pos % K
    ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
    flat = (h.clamp(0, H - 1) * W + w.clamp(0, W - 1)).reshape(N, C, -1)
    src = (dy.to(torch.float64) * ok).reshape(N, C, -1)
    dx = torch.zeros(N, C, H * W, dtype=torch.float64, device=dy.device)
    dx.scatter_add_(2, flat, src)
    return dx.reshape(N, C, H, W)


def pool_tied_windows(x, K, stride, pad):
    """Number of (window, channel) pairs whose maximum is attained twice."""
    F = torch.nn.functional
    N, C, H, W = x.shape
    xf = x.to(torch.float32).contiguous().reshape(N * C, 1, H, W)
    xp = F.pad(xf, (pad, pad, pad, pad), value=float("-inf"))
    cols = F.unfold(xp, K, stride=stride)  # [N*C, K*K, L]
    mx = cols.max(1, keepdim=True).values
    return int(((cols == mx).sum(1) > 1).sum())


# ------------------------------------------------------------------ softmax
def xent_ref(logits, target):
    """fp64 loss (batch mean), probs and the bounds of both."""
    x = logits.to(torch.float64)
    B = x.shape[0]
    mx = x.max(1, keepdim=True).values
    e = (x - mx).exp()
    s = e.sum(1, keepdim=True)
    probs = e / s
    xt = x.gather(1, target.to(x.device)[:, None])
    rows = s.log() + mx - xt
    loss = rows.mean()
    # each row's loss is log(sum) + max - x_t: its three terms are the
    # summands of the batch mean
    loss_abs = STAT * (s.log().abs() + mx.abs() + xt.abs()).sum() / B
    # a probability is one term over a sum of positive terms: relative STAT
    return loss, loss_abs, probs, STAT * probs


def xent_bwd_ref(probs, target, dloss):
    p = probs.to(torch.float64)
    B = p.shape[0]
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, target.to(p.device)[:, None], 1.0)
    sc = float(dloss) / B
    return (p - onehot) * sc, ABS_TERM * (p + onehot) * abs(sc)


# ------------------------------------------------------------------ sgd
def sgd_ref(p, g, m, lr, mu, wd, nesterov):
    """fp64 algebra of one step. Returns (p_new, p_abs, m_new, m_abs); the
    absolute parts are REL_F32 x the terms of each expression (master - lr*
    step cancels for some elements, where no fp32 evaluation, torch's own
    included, holds a bound relative to the result alone)."""
    pd, gd, md = p.to(torch.float64), g.to(torch.float64), m.to(torch.float64)
    gj = gd + wd * pd
    m_new = mu * md + gj
    m_abs = REL_F32 * (abs(mu) * md.abs() + gd.abs() + abs(wd) * pd.abs())
    step = gj + mu * m_new if nesterov else m_new
    step_abs = (gd.abs() + abs(wd) * pd.abs()) * (1 + (mu if nesterov else 0)) \
        + abs(mu) * md.abs() * (mu if nesterov else 1)
    p_new = pd - lr * step
    p_abs = REL_F32 * (pd.abs() + abs(lr) * step_abs)
    return p_new, p_abs, m_new, m_abs
