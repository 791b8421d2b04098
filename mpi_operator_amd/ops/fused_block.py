"""Fused ResNet bottleneck (GPU training path): one autograd Function spans
conv1→bn1relu→conv2→bn2relu→conv3→bn3(+residual add+relu) and the optional
downsample branch, chaining the HIP primitives manually.

What the fusion buys over per-op autograd (per block, per step):
  - the residual join's add is folded into bn3's apply pass (one fewer full
    activation read+write);
  - the join's BACKWARD sum (conv1-dgrad + skip-grad·mask, an at::add plus a
    masking pass per block in autograd) is ONE streaming kernel over separate
    tensors (an accumulate epilogue on conv1's dgrad was measured 2x slower,
    see csrc/elementwise.hip), and between linked blocks that kernel also
    emits the backward statistics of the BN that consumes the sum
    (MPIAMD_FUSEBN_JOIN below);
  - autograd bookkeeping for 6+ interior nodes disappears.

Numerics are identical to the unfused path: same GEMM kernels, same order.
Only the opt-in epilogue statistics (MPIAMD_FUSEBN_EPI, see below) change the
fp32 summation order of the forward statistics on unsplit conv routes.
"""
from __future__ import annotations

import torch

from ._backend import hip_ext

import os as _os

# BN-statistics fusion (docs/tuning.md, profiles/BENCH_HISTORY.md).
#   MPIAMD_FUSEBN         master gate (default on); "0" turns all four
#                         parts off.
#   MPIAMD_FUSEBN_EPI     forward Σy/Σy² out of the conv GEMM epilogue on
#                         every unsplit route (8-wave and 256² kernels
#                         included). Default OFF: it is faster (+2.2%) but
#                         reorders the fp32 sums of the statistics, and a
#                         training trajectory amplifies that to O(1) logit
#                         differences within ten steps — results must stay
#                         what they were. "1" enables for A/B.
#   MPIAMD_FUSEBN_SPLITK  forward split-K convs: the split-K reduce also
#                         emits the stats slab. Default on: tensor and
#                         statistics bit-identical to the unfused pair.
#   MPIAMD_FUSEBN_BWD     backward: the split-K dgrad reduce also emits the
#                         Σ(dy·m), Σ(dy·m·x̂) slab of the BN that consumes
#                         it. Default on: bit-identical likewise.
#   MPIAMD_FUSEBN_JOIN    backward: the residual-join gradient kernel of
#                         block i also emits the Σ(dy·m), Σ(dy·m·x̂) slab(s)
#                         of block i-1's bn3 (and downsample BN), which take
#                         that gradient as their dy. Bit-identical likewise.
# The sub-gates only act under the master gate; each is "1"/"0".
_FUSEBN = _os.environ.get("MPIAMD_FUSEBN", "1") == "1"
_FUSEBN_EPI = _FUSEBN and _os.environ.get("MPIAMD_FUSEBN_EPI", "0") == "1"
_FUSEBN_SPLITK = _FUSEBN and _os.environ.get("MPIAMD_FUSEBN_SPLITK", "1") == "1"
_FUSEBN_BWD = _FUSEBN and _os.environ.get("MPIAMD_FUSEBN_BWD", "1") == "1"
_FUSEBN_JOIN = _FUSEBN and _os.environ.get("MPIAMD_FUSEBN_JOIN", "1") == "1"

_EMPTY = None


def _empty():
    global _EMPTY
    if _EMPTY is None:
        _EMPTY = torch.empty(0)
    return _EMPTY


class _JoinLink:
    """What block i needs from block i-1 to compute, inside its own join
    gradient kernel, the backward statistics of the BN layers that consume
    that gradient: block i-1's bn3 (a3, m3, v3) and, if it has one, its
    downsample BN (ad, md, vd); both gate dy by block i-1's join mask mk3.
    Filled by block i-1's forward and carried to block i as a Python
    attribute of the activation between them.

    Block i's backward leaves dxt and the slab(s) here; block i-1's backward
    uses the slabs only if the dout it is handed IS that dxt and clears them
    either way. Holding the reference is what makes an equal pointer mean the
    same values: the storage cannot be freed and reused, and autograd does
    not accumulate a second consumer's gradient into a tensor that is
    referenced elsewhere (it sums into a new one, which then fails the test)."""
    __slots__ = ("a3", "mk3", "m3", "v3", "ad", "md", "vd",
                 "dxt", "slab", "slab_ds")

    def __init__(self):
        for f in self.__slots__:
            setattr(self, f, None)

    def take(self, dout):
        """Called by block i-1's backward, i.e. after every consumer of its
        output has run its own: (slab, slab_ds) if dout is the dxt the slabs
        were computed from, else (None, None). Empties the link in both
        cases, so that nothing stale survives into another backward and the
        activations are held no longer than autograd's saved tensors are (a
        second backward under retain_graph then finds an empty link and runs
        unlinked)."""
        dxt, slab, slab_ds = self.dxt, self.slab, self.slab_ds
        for f in self.__slots__:
            setattr(self, f, None)
        if (dxt is not None and dout.data_ptr() == dxt.data_ptr()
                and dout.shape == dxt.shape and dout.stride() == dxt.stride()
                and dout.dtype == dxt.dtype):
            return slab, slab_ds
        return None, None


class BottleneckFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, link_in, link_out, stride, eps, momentum,
                w1, g1, b1, rm1, rv1,
                w2, g2, b2, rm2, rv2,
                w3, g3, b3, rm3, rv3,
                wd, gd, bd, rmd, rvd):
        ext = hip_ext()
        e = _empty()

        def conv_bn(xin, w, st, pad, g, b, eps_, relu, rm, rv, mom, res):
            """conv with BN stats fused into the GEMM epilogue (unsplit
            routes) or the split-K reduce; an empty slab (no stats produced
            for this shape) takes the partials pass.
            Returns the relu bitmask too (backward skips the y re-read)."""
            if not (_FUSEBN_EPI or _FUSEBN_SPLITK):
                a = ext.conv2d_fwd(xin, w, st, pad)
                y, m, v, mk = ext.bn_fwd_train(a, g, b, eps_, relu, rm, rv,
                                               mom, res)
                return a, y, m, v, mk
            a, slab = ext.conv2d_fwd_bn(xin, w, st, pad, _FUSEBN_SPLITK,
                                        _FUSEBN_EPI)
            if slab.numel() > 0:
                y, m, v, mk = ext.bn_fwd_train_pre(a, slab, g, b, eps_, relu,
                                                   rm, rv, mom, res)
            else:
                y, m, v, mk = ext.bn_fwd_train(a, g, b, eps_, relu, rm, rv,
                                               mom, res)
            return a, y, m, v, mk

        a1, y1, m1, v1, mk1 = conv_bn(x, w1, 1, 0, g1, b1, eps, True, rm1,
                                      rv1, momentum, e)
        a2, y2, m2, v2, mk2 = conv_bn(y1, w2, stride, 1, g2, b2, eps, True,
                                      rm2, rv2, momentum, e)
        has_ds = wd is not None
        if has_ds:
            ad, res, md, vd, _ = conv_bn(x, wd, stride, 0, gd, bd, eps,
                                         False, rmd, rvd, momentum, e)
        else:
            ad = res = md = vd = None
        a3, out, m3, v3, mk3 = conv_bn(y2, w3, 1, 0, g3, b3, eps, True, rm3,
                                       rv3, momentum, res if has_ds else x)
        saved = [x, a1, y1, a2, y2, a3, out, m1, v1, m2, v2, m3, v3,
                 w1, g1, w2, g2, w3, g3, mk1, mk2, mk3]
        if has_ds:
            saved += [ad, md, vd, wd, gd]
        ctx.save_for_backward(*saved)
        ctx.stride = stride
        ctx.has_ds = has_ds
        # link_in: the producer of x; usable only for the activation it was
        # filled for
        if link_in is not None and (link_in.a3 is None
                                    or link_in.a3.shape != x.shape):
            link_in = None
        ctx.link_in = link_in
        ctx.link_out = link_out
        if link_out is not None:
            link_out.a3, link_out.mk3 = a3, mk3
            link_out.m3, link_out.v3 = m3, v3
            if has_ds:
                link_out.ad, link_out.md, link_out.vd = ad, md, vd
        return out

    @staticmethod
    def backward(ctx, dout):
        ext = hip_ext()
        st = ctx.stride
        (x, a1, y1, a2, y2, a3, out, m1, v1, m2, v2, m3, v3,
         w1, g1, w2, g2, w3, g3, mk1, mk2, mk3) = ctx.saved_tensors[:22]
        if ctx.has_ds:
            ad, md, vd, wd, gd = ctx.saved_tensors[22:]

        dout = dout.contiguous(memory_format=torch.channels_last)
        # The join's ReLU mask (out > 0) is applied INSIDE each consumer
        # (bn_bwd's relu path reads `out` anyway) — the old materialized
        # g = dout·(out>0) was pure data movement (2 extra passes/block).

        def dgrad_bn(dyo, w, st_, pad, a, y, g, m, v, mk):
            """dgrad feeding a BN(+ReLU) backward: a split-K dgrad's reduce
            also emits that BN's partial-stats slab; an empty slab (unsplit
            or stride-2 dgrad) takes the partials pass."""
            if not _FUSEBN_BWD or st_ != 1:
                dy = ext.conv2d_dgrad(dyo, w, y.shape[2], y.shape[3], st_, pad)
                return ext.bn_bwd(dy, a, y, g, m, v, True, mk)
            dy, slab = ext.conv2d_dgrad_bn(dyo, w, y.shape[2], y.shape[3],
                                           st_, pad, a, y, m, v, True, mk)
            if slab.numel() > 0:
                return ext.bn_bwd_pre(dy, slab, a, y, g, m, v, True, mk)
            return ext.bn_bwd(dy, a, y, g, m, v, True, mk)

        def bn_bwd_join(slab, a, g, m, v):
            """BN backward of a layer whose dy is dout: from the slab the
            next block's join kernel left, else with the partials pass."""
            if slab is not None:
                return ext.bn_bwd_pre(dout, slab, a, out, g, m, v, True, mk3)
            return ext.bn_bwd(dout, a, out, g, m, v, True, mk3)

        slab3 = slabd = None
        if ctx.link_out is not None:
            slab3, slabd = ctx.link_out.take(dout)
        dx3, dg3, db3 = bn_bwd_join(slab3, a3, g3, m3, v3)
        dw3 = ext.conv2d_wgrad(y2, dx3, 1, 1, 1, 0)
        dx2, dg2, db2 = dgrad_bn(dx3, w3, 1, 0, a2, y2, g2, m2, v2, mk2)
        dw2 = ext.conv2d_wgrad(y1, dx2, 3, 3, st, 1)
        dx1, dg1, db1 = dgrad_bn(dx2, w2, st, 1, a1, y1, g1, m1, v1, mk1)
        dw1 = ext.conv2d_wgrad(x, dx1, 1, 1, 1, 0)

        dx0 = ext.conv2d_dgrad(dx1, w1, x.shape[2], x.shape[3], 1, 0)
        if ctx.has_ds:
            # mask from the join output (the downsample BN itself has no
            # ReLU): dy_ds = dout·(out>0), applied inside bn_bwd
            # the join mask (out>0) is bn3's mask
            dad, dgd, dbd = bn_bwd_join(slabd, ad, gd, md, vd)
            dwd = ext.conv2d_wgrad(x, dad, 1, 1, st, 0)
            skip = ext.conv2d_dgrad(dad, wd, x.shape[2], x.shape[3], st, 0)
            ja, jmask = skip, _empty()  # dxt = skip + dx0
        else:
            dwd = dgd = dbd = None
            ja, jmask = dout, mk3  # one-pass join: dxt = dx0 + dout·(out>0)
        lk = ctx.link_in
        if lk is not None and lk.a3 is not None:
            # the same sum, and the partial stats of the producer block's
            # bn3 / downsample BN while dxt is still in registers
            e = _empty()
            has_d = lk.ad is not None
            res = ext.join_bwd_stats(ja, jmask, dx0, lk.a3, lk.m3, lk.v3,
                                     lk.mk3, lk.ad if has_d else e,
                                     lk.md if has_d else e,
                                     lk.vd if has_d else e)
            dxt = res[0]
            lk.dxt, lk.slab = dxt, res[1]
            lk.slab_ds = res[2] if has_d else None
        elif ctx.has_ds:
            dxt = ext.add_bf16(ja, dx0)
        else:
            dxt = ext.add_relu_bwd_add_mask(ja, jmask, dx0)

        f32 = torch.float32
        return (dxt, None, None, None, None, None,
                dw1, dg1.to(f32), db1.to(f32), None, None,
                dw2, dg2.to(f32), db2.to(f32), None, None,
                dw3, dg3.to(f32), db3.to(f32), None, None,
                dwd, dgd.to(f32) if dgd is not None else None,
                dbd.to(f32) if dbd is not None else None, None, None)


def fused_bottleneck(x, block):
    """Run `block` (a models.resnet.Bottleneck) through the fused Function."""
    ds = block.downsample
    if ds is not None:
        wd, bnd = ds[0].weight, ds[1]
        args = (wd, bnd.weight, bnd.bias, bnd.running_mean, bnd.running_var)
    else:
        args = (None, None, None, None, None)
    # producer-side link for the join/BN-stats fusion: filled by this block's
    # forward, picked up by the next block from the activation it rides on
    link_in = getattr(x, "_mpiamd_join_link", None) if _FUSEBN_JOIN else None
    link_out = _JoinLink() if _FUSEBN_JOIN else None
    out = BottleneckFn.apply(
        x, link_in, link_out,
        block.conv2.stride, block.bn1.eps, block.bn1.momentum,
        block.conv1.weight, block.bn1.weight, block.bn1.bias,
        block.bn1.running_mean, block.bn1.running_var,
        block.conv2.weight, block.bn2.weight, block.bn2.bias,
        block.bn2.running_mean, block.bn2.running_var,
        block.conv3.weight, block.bn3.weight, block.bn3.bias,
        block.bn3.running_mean, block.bn3.running_var,
        *args)
    if link_out is not None:
        out._mpiamd_join_link = link_out
    return out
