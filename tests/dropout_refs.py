"""fp64 references and bounds of the dropout tests (test_dropout_gpu.py),
built the stream_refs way: per element |out - ref| <= rel*|ref| + abs_i with
abs_i assembled from the magnitudes of the terms of the expression the kernel
evaluates. Plain torch, device-agnostic.

LayerNorm forward, as ln_fwd_drop_add_k evaluates it in fp32 over a row of N
bf16 values s (exact in fp32):

  mu   = sum(s) / N                       sum bound STAT * mean|s|
  var  = sum(s^2) / N - mu^2              the two means' bounds to first
                                          order, plus the subtraction's own
                                          rounding REL_F32 * (E[s^2] + mu^2)
  rstd = rsqrt(var + eps)                 d rstd = rstd/2 * dvar / (var+eps)
  y    = bf16((s - mu) * rstd * g + b)    REL_BF16 for the rounding, ABS_TERM
                                          x the terms that cancel (s*rstd*g,
                                          mu*rstd*g, b), and the errors of mu
                                          and rstd carried through

LayerNorm backward (ln_bwd_drop_dx_k, from the SAVED fp32 mean / rstd, which
are inputs here, not quantities under test):

  xh = (x - mu) * rstd;  s1 = mean(g*dy);  s2 = mean(g*dy*xh)
  dx = rstd * (g*dy - s1 - xh*s2)         ABS_TERM x (|g*dy| + |s1| +
                                          (|x|+|mu|)*rstd*|s2|) for the
                                          cancelling terms (xh's own
                                          cancellation included), STAT x the
                                          summands of s1 and s2
"""
import torch

from stream_refs import ABS_TERM, REL_F32, STAT


def unpack_keep(mask, shape):
    """uint8 keep bytes (bit j of byte o = element 8*o + j of the flat,
    contiguous tensor) -> bool tensor of `shape`."""
    bits = (mask.reshape(-1).to(torch.int32)[:, None] >> torch.arange(
        8, device=mask.device, dtype=torch.int32)) & 1
    return bits.reshape(shape).bool()


def drop_add_ref(a, b, keep, scale):
    """fp64 a + keep*b*scale and the absolute part of its bound: the fp32
    multiply and add round once each, or once together if contracted."""
    ad, bd = a.to(torch.float64), b.to(torch.float64) * scale
    k = keep.to(ad.device)
    return ad + bd * k, REL_F32 * (ad.abs() + bd.abs())


def ln_fwd_ref(s, gamma, beta, eps):
    """fp64 LayerNorm of the rows of s [M, N]; dict of references and
    '<name>_abs' absolute bound parts (module docstring)."""
    sd = s.to(torch.float64)
    g, b = gamma.to(torch.float64), beta.to(torch.float64)
    mean = sd.mean(1)
    eabs = sd.abs().mean(1)
    ex2 = (sd * sd).mean(1)
    var = ((sd - mean[:, None]) ** 2).mean(1)
    rstd = (var + eps).rsqrt()
    mean_abs = STAT * eabs
    var_abs = (STAT * (ex2 + 2 * mean.abs() * eabs)
               + REL_F32 * (ex2 + mean * mean))
    rstd_abs = 0.5 * rstd * var_abs / (var + eps)
    y = (sd - mean[:, None]) * rstd[:, None] * g + b
    mean_bnd = REL_F32 * mean.abs() + mean_abs
    rstd_bnd = REL_F32 * rstd + rstd_abs
    y_abs = (ABS_TERM * ((sd.abs() + mean.abs()[:, None]) * rstd[:, None] * g.abs()
                         + b.abs())
             + rstd[:, None] * g.abs() * mean_bnd[:, None]
             + (sd - mean[:, None]).abs() * g.abs() * rstd_bnd[:, None])
    return dict(mean=mean, mean_abs=mean_abs, rstd=rstd, rstd_abs=rstd_abs,
                y=y, y_abs=y_abs)


def ln_bwd_dx_ref(dy, x, gamma, mean, rstd):
    """fp64 dx of LayerNorm from the kernel's own inputs (mean / rstd as the
    forward saved them). Returns (dx, dx_abs)."""
    dyd, xd = dy.to(torch.float64), x.to(torch.float64)
    g = gamma.to(torch.float64)
    mu = mean.to(torch.float64)[:, None]
    rs = rstd.to(torch.float64)[:, None]
    xh = (xd - mu) * rs
    gd = g * dyd
    s1 = gd.mean(1, keepdim=True)
    s2 = (gd * xh).mean(1, keepdim=True)
    dx = rs * (gd - s1 - xh * s2)
    s1_bnd = STAT * gd.abs().mean(1, keepdim=True)
    s2_bnd = STAT * (gd * xh).abs().mean(1, keepdim=True)
    dx_abs = rs * (ABS_TERM * (gd.abs() + s1.abs()
                               + (xd.abs() + mu.abs()) * rs * s2.abs())
                   + s1_bnd + xh.abs() * s2_bnd)
    return dx, dx_abs
