"""fp64 references, per-element bounds and the edge geometries of the
implicit-GEMM convolution tests (test_conv_edges_gpu.py on the GPU,
test_conv_refs_cpu.py for the references and bounds themselves). Plain torch;
the references always compute on the CPU, from an explicit zero-padded gather
(F.unfold / F.fold of a padded tensor) and an fp64 matmul, so they depend on
no convolution library of the device.

Bound, per output element:

    |out - ref| <= rel*|ref| + n * 2^-24 * T

  rel = 2^-8 (stream_refs.REL_BF16): the single rounding of the fp32
        accumulator to bf16; 0 for an fp32 output.
  T   = sum |terms| of that element: the same expression evaluated on |x|,
        |w|, |dy|.
  n   = number of summands: R*S*C (fwd), R*S*Kout (dgrad), N*HO*WO (wgrad).
        Padding taps count, so the bound is a little loose.

n * 2^-24 * T is the worst-case error of an fp32 sum of n exactly
representable bf16 x bf16 products taken in ANY order (each of the n-1 adds
rounds a partial sum that never exceeds T by half an ulp, 2^-24 relative), so
every kernel route and every split-K count shares it. It is derived, not
measured. Elements that no term reaches (dx rows and columns no window covers,
dead stride-2 parities, outputs whose whole window is padding) have T = 0 and
therefore a bound of exactly 0: they must be exactly 0.
"""
import functools

import torch

from stream_refs import REL_BF16, assert_close, rand_bf16  # noqa: F401

F = torch.nn.functional
U32 = 2.0 ** -24  # unit roundoff of fp32

# id -> (N, C, H, W, Kout, R, S, stride, pad); what each reaches is asserted
# by test_conv_refs_cpu.py::test_geometries_keep_their_edges
CASES = {
    "nonsq-3x3": (3, 16, 9, 13, 24, 3, 3, 1, 1),
    "nonsq-3x3-s2": (3, 16, 13, 9, 24, 3, 3, 2, 1),
    "k1x3": (2, 8, 11, 14, 16, 1, 3, 1, 1),
    "k3x1": (2, 8, 14, 11, 16, 3, 1, 1, 1),
    "k5x5": (2, 8, 12, 10, 16, 5, 5, 1, 2),
    "k3x3-p0": (2, 8, 12, 10, 16, 3, 3, 1, 0),
    "k3x3-p2": (2, 8, 12, 10, 16, 3, 3, 1, 2),
    "k1x1-s2": (2, 16, 10, 7, 32, 1, 1, 2, 0),
    "k1x1-s2-p1": (2, 16, 10, 7, 32, 1, 1, 2, 1),
    "k2x2-s2": (2, 16, 9, 12, 32, 2, 2, 2, 0),
    "k1x3-s2": (2, 16, 9, 12, 32, 1, 3, 2, 0),
    "splitk": (2, 128, 9, 7, 128, 3, 3, 1, 1),
    "c24-k136": (2, 24, 6, 5, 136, 3, 3, 1, 1),
    "s3": (2, 8, 13, 11, 16, 3, 3, 3, 1),
    "wgrad-8way": (5, 8, 31, 29, 16, 3, 3, 1, 1),
    "one-pixel-3x3": (1, 8, 3, 3, 8, 3, 3, 1, 0),
    "one-pixel-1x1": (1, 8, 1, 1, 8, 1, 1, 1, 0),
}
NO_DGRAD = ("s3",)  # conv2d_dgrad supports stride 1 and 2 only

# conv2d_dgrad_acc: (N, C, H, W, Kout), 1x1 stride 1 pad 0
ACC_GEOM = (3, 16, 9, 13, 24)


def out_hw(geom):
    N, C, H, W, K, R, S, st, pad = geom
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


def live_parities(geom):
    """The (h%2, w%2) sub-images of dx a stride-2 conv reaches: parity p is
    live on an axis if some tap r has (p + pad - r) even."""
    _, _, _, _, _, R, S, _, pad = geom
    return [(ph, pw) for ph in (0, 1) for pw in (0, 1)
            if len(range((ph + pad) & 1, R, 2)) and len(range((pw + pad) & 1, S, 2))]


def conv_splits_model(M, ncols, K):
    """The fwd/dgrad split-K heuristic of the bindings (no knob set)."""
    tiles = ((M + 127) // 128) * ((ncols + 127) // 128)
    nk = (K + 63) // 64
    if tiles >= 256 or nk < 16:
        return 1
    return max(1, min(512 // tiles, nk // 8, 16))


def wgrad_splits_model(Kout, RSC, M, budget=512):
    """The wgrad split count of the bindings."""
    tiles = ((Kout + 127) // 128) * ((RSC + 127) // 128)
    nk = (M + 63) // 64
    s = min(max(budget // tiles, 1), max(nk // 8, 1), 256)
    return s & ~7 if s >= 8 else s


def inputs(geom, seed, device="cpu"):
    """Independent random bf16 x, w, dy of one geometry (channels_last)."""
    N, C, H, W, K, R, S, st, pad = geom
    HO, WO = out_hw(geom)
    x = rand_bf16((N, C, H, W), seed, device=device)
    w = rand_bf16((K, C, R, S), seed + 1, scale=0.5, device=device)
    dy = rand_bf16((N, K, HO, WO), seed + 2, device=device)
    return x, w, dy


def poison(shape, like):
    """Allocate a tensor of an output's shape, dtype and (channels_last for
    4-D) layout on `like`'s device, fill it with NaN and free it. Called
    right before a kernel whose binding allocates its output with at::empty,
    the caching allocator then usually hands that same block out again, so
    an element the kernel never writes reads NaN (which check_close fails)
    and not stale, plausible data. Best effort only: nothing guarantees the
    block is reused, so a pass does not prove every element was written."""
    fmt = torch.channels_last if len(shape) == 4 else torch.contiguous_format
    t = torch.empty(shape, dtype=like.dtype, device=like.device,
                    memory_format=fmt)
    t.fill_(float("nan"))
    del t


# ------------------------------------------------------------- references
def _cols(x, geom):
    """Explicit zero-padded gather: [N, C*R*S, HO*WO], fp64, on the CPU."""
    N, C, H, W, K, R, S, st, pad = geom
    xp = F.pad(x.detach().to("cpu", torch.float64).contiguous(),
               (pad, pad, pad, pad))
    return F.unfold(xp, (R, S), stride=st)


def _fwd(x, w, geom):
    N, C, H, W, K, R, S, st, pad = geom
    HO, WO = out_hw(geom)
    wm = w.detach().to("cpu", torch.float64).contiguous().reshape(K, C * R * S)
    return (wm @ _cols(x, geom)).reshape(N, K, HO, WO)


def _dgrad(dy, w, geom):
    N, C, H, W, K, R, S, st, pad = geom
    wm = w.detach().to("cpu", torch.float64).contiguous().reshape(K, C * R * S)
    dym = dy.detach().to("cpu", torch.float64).contiguous().reshape(N, K, -1)
    # scatter of every window's contribution back onto the padded input
    dxp = F.fold(wm.t() @ dym, (H + 2 * pad, W + 2 * pad), (R, S), stride=st)
    return dxp[:, :, pad:pad + H, pad:pad + W].contiguous()


def _wgrad(x, dy, geom):
    N, C, H, W, K, R, S, st, pad = geom
    dym = dy.detach().to("cpu", torch.float64).contiguous().reshape(N, K, -1)
    return (dym @ _cols(x, geom).transpose(1, 2)).sum(0).reshape(K, C, R, S)


def summands(geom):
    N, C, H, W, K, R, S, st, pad = geom
    HO, WO = out_hw(geom)
    return dict(y=R * S * C, dx=R * S * K, dw=N * HO * WO)


def fwd_ref(x, w, geom):
    """(y fp64, absolute part of the bound)."""
    return _fwd(x, w, geom), summands(geom)["y"] * U32 * _fwd(x.abs(), w.abs(), geom)


def dgrad_ref(dy, w, geom):
    return (_dgrad(dy, w, geom),
            summands(geom)["dx"] * U32 * _dgrad(dy.abs(), w.abs(), geom))


def wgrad_ref(x, dy, geom):
    return (_wgrad(x, dy, geom),
            summands(geom)["dw"] * U32 * _wgrad(x.abs(), dy.abs(), geom))


def dgrad_acc_ref(dy, w, dx0):
    """dx0 + dy.w of a 1x1 stride-1 conv: one more summand, |dx0| joins T."""
    N, K, H, W = dy.shape
    geom = (N, w.shape[1], H, W, K, 1, 1, 1, 0)
    d0 = dx0.detach().to("cpu", torch.float64)
    ref = d0 + _dgrad(dy, w, geom)
    T = d0.abs() + _dgrad(dy.abs(), w.abs(), geom)
    return ref, (K + 1) * U32 * T


@functools.lru_cache(maxsize=None)
def case_refs(name, seed=100):
    """CPU inputs and every reference of one case, made once, never modified."""
    geom = CASES[name]
    x, w, dy = inputs(geom, seed)
    y, y_abs = fwd_ref(x, w, geom)
    dw, dw_abs = wgrad_ref(x, dy, geom)
    dx, dx_abs = dgrad_ref(dy, w, geom)
    return dict(geom=geom, x=x, w=w, dy=dy, y=y, y_abs=y_abs, dx=dx,
                dx_abs=dx_abs, dw=dw, dw_abs=dw_abs)
