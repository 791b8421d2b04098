"""Autograd-integrated ops with HIP (gfx950) dispatch.

Dispatch rule (see ``_backend``): CUDA/ROCm tensors run the hand-written HIP
kernels — a missing extension raises; CPU tensors run the PyTorch reference.

GPU layout/dtype contract (MI355X-first):
  - activations: logical NCHW, channels-last memory (NHWC), bf16
  - conv weights: logical [K,C,R,S], channels-last memory ([K][R][S][C]), bf16
  - conv dgrad/wgrad: dx bf16, dw fp32 (accumulated exactly in fp32)
  - BN gamma/beta and all per-channel stats: fp32

Reference parity: these ops cover the tf_cnn_benchmarks ResNet hot path the
reference delegates to external CUDA images.
"""
from __future__ import annotations

import torch

from . import reference as ref
from ._backend import hip_ext


def _cl(t):  # channels_last view check for 4-D activations
    return t.is_contiguous(memory_format=torch.channels_last)


# Side-stream weight-gradient overlap was tried and REJECTED (round 2):
# running the dw/db GEMMs on a second HIP stream concurrently with the
# dgrad chain measured 1363 -> 1310 seq/s on BERT-Large bs32 — the wgrad
# and dgrad pipelined GEMMs contend for CUs and both fall off their tuned
# occupancy; correctness also requires record_stream on every cross-stream
# input. Kernels stay single-stream; join_wgrad_stream() remains as a
# no-op contract point for FusedSGD.


def join_wgrad_stream():
    return None


class Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride: int, padding: int):
        ctx.stride, ctx.padding = stride, padding
        ctx.save_for_backward(x, w)
        if x.is_cuda:
            assert _cl(x) and _cl(w), "conv2d: GPU tensors must be channels_last"
            return hip_ext().conv2d_fwd(x, w, stride, padding)
        return ref.conv2d_fwd(x, w, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        st, pad = ctx.stride, ctx.padding
        dx = dw = None
        if dy.is_cuda:
            dy = dy.contiguous(memory_format=torch.channels_last)
            if ctx.needs_input_grad[0]:
                dx = hip_ext().conv2d_dgrad(dy, w, x.shape[2], x.shape[3], st, pad)
            if ctx.needs_input_grad[1]:
                dw = hip_ext().conv2d_wgrad(x, dy, w.shape[2], w.shape[3], st, pad)
                dw = dw.to(w.dtype)
        else:
            if ctx.needs_input_grad[0]:
                dx = ref.conv2d_dgrad(dy, w, x.shape, st, pad)
            if ctx.needs_input_grad[1]:
                dw = ref.conv2d_wgrad(x, dy, w.shape, st, pad).to(w.dtype)
        return dx, dw, None, None


def conv2d(x, w, stride: int = 1, padding: int = 0):
    return Conv2dFn.apply(x, w, stride, padding)


class BNReLUFn(torch.autograd.Function):
    """Fused BatchNorm(+ReLU) with batch stats (training mode). On GPU the
    finalize kernel also updates running_mean/var in place (buffers, no
    autograd) — saving the eager per-layer stat updates."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float, relu: bool,
                running_mean=None, running_var=None, momentum: float = 0.1):
        if x.is_cuda:
            assert _cl(x), "bn_relu: GPU tensors must be channels_last"
            empty = torch.empty(0)
            y, mean, invstd, mask = hip_ext().bn_fwd_train(
                x, gamma, beta, eps, relu,
                running_mean if running_mean is not None else empty,
                running_var if running_var is not None else empty, momentum,
                empty)
        else:
            y, mean, invstd = ref.bn_relu_fwd_train(x, gamma, beta, eps, relu)
            mask = torch.empty(0, dtype=torch.uint8)
            if running_mean is not None:
                with torch.no_grad():
                    n = x.numel() / x.shape[1]
                    var = invstd.pow(-2) - eps
                    running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
                    running_var.mul_(1 - momentum).add_(var * n / max(n - 1, 1), alpha=momentum)
        ctx.relu = relu
        ctx.save_for_backward(x, y, gamma, mean, invstd, mask)
        ctx.mark_non_differentiable(mean, invstd)
        # without this, autograd materializes a zero tensor for dmean and
        # dinvstd on EVERY backward (2 fill launches × every BN layer × step)
        ctx.set_materialize_grads(False)
        return y, mean, invstd

    @staticmethod
    def backward(ctx, dy, _dmean=None, _dinvstd=None):
        x, y, gamma, mean, invstd, mask = ctx.saved_tensors
        if dy.is_cuda:
            dy = dy.contiguous(memory_format=torch.channels_last)
            dx, dgamma, dbeta = hip_ext().bn_bwd(dy, x, y, gamma, mean,
                                                 invstd, ctx.relu, mask)
        else:
            dx, dgamma, dbeta = ref.bn_relu_bwd(dy, x, y, gamma, mean, invstd, ctx.relu)
        return (dx, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None, None,
                None, None, None)


def bn_relu_train(x, gamma, beta, eps: float = 1e-5, relu: bool = True,
                  running_mean=None, running_var=None, momentum: float = 0.1):
    return BNReLUFn.apply(x, gamma, beta, eps, relu, running_mean, running_var, momentum)


def bn_relu_eval(x, gamma, beta, running_mean, running_var, eps: float = 1e-5, relu: bool = True):
    if x.is_cuda:
        invstd = (running_var.float() + eps).rsqrt()
        scale = gamma.float() * invstd
        shift = beta.float() - running_mean.float() * scale
        return hip_ext().bn_fwd_eval(x, scale, shift, relu)
    return ref.bn_relu_fwd_eval(x, gamma, beta, running_mean, running_var, eps, relu)


class MaxPool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel: int, stride: int, padding: int):
        ctx.kernel, ctx.stride, ctx.padding = kernel, stride, padding
        ctx.x_shape = x.shape
        if x.is_cuda:
            assert _cl(x)
            y, idx = hip_ext().maxpool_fwd(x, kernel, stride, padding)
        else:
            y, idx = ref.max_pool2d_fwd(x, kernel, stride, padding)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        if dy.is_cuda:
            dy = dy.contiguous(memory_format=torch.channels_last)
            dx = hip_ext().maxpool_bwd(dy, idx, ctx.x_shape[2], ctx.x_shape[3],
                                       ctx.kernel, ctx.stride, ctx.padding)
        else:
            dx = ref.max_pool2d_bwd(dy, idx, ctx.x_shape, ctx.kernel, ctx.stride, ctx.padding)
        return dx, None, None, None


def max_pool2d(x, kernel: int = 3, stride: int = 2, padding: int = 1):
    return MaxPool2dFn.apply(x, kernel, stride, padding)


class GlobalAvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.x_shape = x.shape
        if x.is_cuda:
            assert _cl(x)
            return hip_ext().gap_fwd(x)
        return ref.global_avg_pool_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        if dy.is_cuda:
            return hip_ext().gap_bwd(dy.contiguous(), ctx.x_shape[2], ctx.x_shape[3])
        return ref.global_avg_pool_bwd(dy, ctx.x_shape)


def global_avg_pool(x):
    return GlobalAvgPoolFn.apply(x)


class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.b_dtype = b.dtype
        if x.is_cuda:
            return hip_ext().linear_fwd(x, w, b)
        return ref.linear_fwd(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        if dy.is_cuda:
            dy = dy.contiguous()
            dx, dw, db = hip_ext().linear_bwd(dy, x, w)
            return dx, dw.to(w.dtype), db.to(ctx.b_dtype)
        dx = dy @ w
        dw = dy.transpose(0, 1).float() @ x.float()
        db = dy.float().sum(0)
        return dx, dw.to(w.dtype), db.to(ctx.b_dtype)


def linear(x, w, b):
    return LinearFn.apply(x, w, b)


class LayerNormFn(torch.autograd.Function):
    """Fused LayerNorm over the last dim (bf16 activations, fp32 params) —
    one wave per row, shfl row reduction; bwd reduces dgamma/dbeta through
    per-block fp32 slabs (ops/csrc/layernorm.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps: float):
        y, mean, rstd = hip_ext().layernorm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dg, db = hip_ext().layernorm_bwd(dy, x, weight, mean, rstd)
        return dx, dg, db, None


def layer_norm(x, weight, bias, eps: float = 1e-12):
    return LayerNormFn.apply(x, weight, bias, eps)


class SoftmaxCrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        if logits.is_cuda:
            loss, probs = hip_ext().softmax_xent_fwd(logits.contiguous(), target)
        else:
            loss, probs = ref.softmax_cross_entropy_fwd(logits, target)
        ctx.save_for_backward(probs, target)
        ctx.dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, dloss):
        probs, target = ctx.saved_tensors
        if probs.is_cuda:
            # dloss stays on-device: reading it on the host would insert a
            # per-step D2H sync and break hipGraph capture of the train step
            d = hip_ext().softmax_xent_bwd(probs, target,
                                           dloss.reshape(1).float().contiguous())
            return d.to(ctx.dtype), None
        return ref.softmax_cross_entropy_bwd(probs, target, float(dloss)).to(ctx.dtype), None


def softmax_cross_entropy(logits, target):
    return SoftmaxCrossEntropyFn.apply(logits, target)


def sgd_momentum_step(params32, grads, momenta, bf16_outs, lr, momentum, weight_decay, nesterov=False):
    """Fused multi-tensor SGD: fp32 masters + momentum + bf16 working-copy refresh."""
    if params32 and params32[0].is_cuda:
        hip_ext().sgd_step(list(params32), list(grads), list(momenta),
                           [o if o is not None else torch.empty(0) for o in bf16_outs],
                           lr, momentum, weight_decay, nesterov)
    else:
        ref.sgd_momentum_step(params32, grads, momenta, bf16_outs, lr, momentum, weight_decay, nesterov)


OPTIM_EPB = 8192  # elements per block of the multi-tensor optimizer kernels


def optim_block_count(tensors) -> int:
    """Slots one partials slab needs for `tensors` (one per kernel block)."""
    return sum((t.numel() + OPTIM_EPB - 1) // OPTIM_EPB for t in tensors)


def _hip_outs(bf16_outs):
    return [o if o is not None else torch.empty(0) for o in bf16_outs]


def adamw_step(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs, scalars, partials,
               beta1, beta2, eps, weight_decay, adam_w_mode=True, max_grad_norm=None):
    """Fused multi-tensor AdamW (adam_w_mode) / Adam+L2: advances the device
    step state in `scalars` (layout: reference.OPT_*), then updates fp32
    masters and moments and refreshes the bf16 working copies. `partials`
    (>= optim_block_count slots) is only touched when max_grad_norm is set."""
    if params32 and params32[0].is_cuda:
        hip_ext().adam_step(list(params32), list(grads), list(exp_avgs), list(exp_avg_sqs),
                            _hip_outs(bf16_outs), scalars, partials, beta1, beta2, eps,
                            weight_decay, bool(adam_w_mode), max_grad_norm or 0.0)
    else:
        ref.adamw_step(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs, scalars,
                       beta1, beta2, eps, weight_decay, adam_w_mode, max_grad_norm)


def lamb_step(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs, scalars, partials, ratio,
              beta1, beta2, eps, weight_decay, adam_w_mode=True, max_grad_norm=None):
    """Fused multi-tensor LAMB: stage 1 (moments + norm partials), per-tensor
    trust ratio, stage 2 (apply). `partials` holds 3 slabs of
    optim_block_count slots, `ratio` one slot per tensor."""
    if params32 and params32[0].is_cuda:
        hip_ext().lamb_step(list(params32), list(grads), list(exp_avgs), list(exp_avg_sqs),
                            _hip_outs(bf16_outs), scalars, partials, ratio, beta1, beta2,
                            eps, weight_decay, bool(adam_w_mode), max_grad_norm or 0.0)
    else:
        ref.lamb_step(params32, grads, exp_avgs, exp_avg_sqs, bf16_outs, scalars,
                      beta1, beta2, eps, weight_decay, adam_w_mode, max_grad_norm)


class AddReLUFn(torch.autograd.Function):
    """Fused residual add + ReLU (the Bottleneck join — hot elementwise)."""

    @staticmethod
    def forward(ctx, a, b):
        if a.is_cuda:
            assert _cl(a) and _cl(b)
            y = hip_ext().add_relu_fwd(a, b)
        else:
            y = torch.relu(a + b)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        if dy.is_cuda:
            dx = hip_ext().add_relu_bwd(dy.contiguous(memory_format=torch.channels_last), y)
        else:
            dx = dy * (y > 0)
        return dx, dx


def add_relu(a, b):
    return AddReLUFn.apply(a, b)


class MaskedSoftmaxCrossEntropyFn(torch.autograd.Function):
    """MLM-head CE with ignore_index (mean over valid rows). Forward reads
    the bf16 logits once and keeps only [B,2] stats; backward recomputes
    probabilities from the saved bf16 logits — no fp32 logits cast, no fp32
    probs (the torch path's ~1.5 GB of extra HBM traffic at BERT-Large
    scale). Reference role: the loss of the out-of-tree BERT images
    (SURVEY §2.3 N7-class fused op)."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        if logits.is_cuda:
            out, stats = hip_ext().masked_xent_fwd(logits.contiguous(), target,
                                                   ignore_index)
            ctx.save_for_backward(logits, target, stats, out)
            ctx.ignore_index = ignore_index
            # loss = sum / max(count, 1) — stays on device (graph-safe)
            return out[0] / out[1].clamp(min=1.0)
        loss, probs = ref.masked_softmax_cross_entropy_fwd(logits, target,
                                                           ignore_index)
        ctx.save_for_backward(probs, target)
        ctx.cpu_path = True
        ctx.dtype = logits.dtype
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, dloss):
        if getattr(ctx, "cpu_path", False):
            probs, target = ctx.saved_tensors
            d = ref.masked_softmax_cross_entropy_bwd(
                probs, target, float(dloss), ctx.ignore_index)
            return d.to(ctx.dtype), None, None
        logits, target, stats, out = ctx.saved_tensors
        d = hip_ext().masked_xent_bwd(logits, target, stats, out,
                                      dloss.reshape(1).float().contiguous(),
                                      ctx.ignore_index)
        return d, None, None


def masked_softmax_cross_entropy(logits, target, ignore_index=-100):
    return MaskedSoftmaxCrossEntropyFn.apply(logits, target, ignore_index)


class MlmHeadLossFn(torch.autograd.Function):
    """Fused MLM decoder + masked CE: the vocab-scale logits live ONLY in a
    [M, roundup(V,8)] padded buffer — the decoder GEMM writes it (bias in
    the epilogue), CE reads it strided, and the backward kernel writes the
    padded dlogits (zeroed pads) that the dx/dw GEMMs and db colsum consume
    in place. Removes the per-step pad zero-fill + strided copy and the
    unpadded logits materialization of the linear+CE composition."""

    @staticmethod
    def forward(ctx, h, w, b, target, ignore_index):
        out, logits_pad, stats = hip_ext().mlm_head_fwd(h, w, b, target,
                                                        ignore_index)
        ctx.save_for_backward(h, w, logits_pad, stats, out, target)
        ctx.ignore_index = ignore_index
        ctx.V = w.shape[0]
        return out[0] / out[1].clamp(min=1.0)

    @staticmethod
    def backward(ctx, dloss):
        h, w, logits_pad, stats, out, target = ctx.saved_tensors
        dh, dw, db = hip_ext().mlm_head_bwd(
            logits_pad, ctx.V, target, stats, out,
            dloss.reshape(1).float().contiguous(), h, w, ctx.ignore_index)
        return dh, dw, db, None, None


def mlm_head_loss(h, w, b, target, ignore_index=-100):
    return MlmHeadLossFn.apply(h, w, b, target, ignore_index)


class FfnFn(torch.autograd.Function):
    """BERT FFN pair fc2(gelu(fc1(x))) with the GELU fused into the GEMM
    epilogues on both sides: fc1's epilogue emits (gelu(h), gelu'(h)) off a
    single tanh; the backward fc2-dx GEMM multiplies by the SAVED gelu'(h)
    in its epilogue (exp-free — recomputing the tanh there serialized ~27 us
    of v_exp per layer after the MFMA work). The two standalone GELU
    elementwise passes over the [M, intermediate] activation disappear.
    x: [M, H]; w1: [I, H]; w2: [H, I]. On CPU `aux` holds the
    pre-activation instead and the derivative is recomputed in fp32."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        if x.is_cuda:
            g, aux = hip_ext().linear_gelu_fwd(x, w1, b1)  # aux = gelu'(h)
            y = hip_ext().linear_fwd(g, w2, b2)
        else:
            aux = ref.linear_fwd(x, w1, b1.float()).float()  # aux = h_pre
            g = torch.nn.functional.gelu(aux, approximate="tanh").to(x.dtype)
            y = ref.linear_fwd(g, w2, b2)
        ctx.save_for_backward(x, w1, w2, g, aux)
        ctx.b_dtypes = (b1.dtype, b2.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, g, aux = ctx.saved_tensors
        bd1, bd2 = ctx.b_dtypes
        if dy.is_cuda:
            dy = dy.contiguous()
            # fc2 weight grads; its dx is produced by the fused-dgelu GEMM
            dw2, db2 = hip_ext().linear_wgrad_only(dy, g)
            dh = hip_ext().linear_gelu_dgrad(dy, w2, aux)
            dx, dw1, db1 = hip_ext().linear_bwd(dh, x, w1)
            return (dx, dw1.to(w1.dtype), db1.to(bd1),
                    dw2.to(w2.dtype), db2.to(bd2))
        dg = dy @ w2
        dh = (dg.float() * ref.dgelu(aux)).to(dy.dtype)
        dx = dh @ w1
        dw1 = dh.transpose(0, 1).float() @ x.float()
        db1 = dh.float().sum(0)
        dw2 = dy.transpose(0, 1).float() @ g.float()
        db2 = dy.float().sum(0)
        return (dx, dw1.to(w1.dtype), db1.to(bd1), dw2.to(w2.dtype),
                db2.to(bd2))


def ffn(x, w1, b1, w2, b2):
    return FfnFn.apply(x, w1, b1, w2, b2)


class AttentionFn(torch.autograd.Function):
    """Fused MHA forward (QKᵀ→softmax→PV in one kernel, probs saved bf16);
    backward runs the standard four batched GEMMs + softmax-grad through
    torch (shapes are library-friendly; the forward was the launch-bound
    chain). qkv: [B, S, 3, H, 64] → ctx [B, S, H·64]."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, mask):
        out, probs = hip_ext().attn_fwd(qkv.contiguous(), heads, scale, mask,
                                        True)
        ctx.save_for_backward(qkv, probs)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, probs = ctx.saved_tensors
        B, S, _, H, D = qkv.shape
        if S == 128 and D == 64:
            # fused backward: dP/dS/dQ/dK/dV in one kernel per (b, h),
            # written straight into the dqkv layout
            return (hip_ext().attn_bwd(qkv, dout, probs, ctx.scale),
                    None, None, None)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))  # B,H,S,D
        do = dout.view(B, S, H, D).transpose(1, 2)
        p = probs.float()
        dv = torch.matmul(p.transpose(-1, -2).to(do.dtype), do)
        dp = torch.matmul(do, v.transpose(-1, -2)).float()
        ds = (dp - (dp * p).sum(-1, keepdim=True)) * p * ctx.scale
        ds = ds.to(do.dtype)
        dq = torch.matmul(ds, k)
        dk = torch.matmul(ds.transpose(-1, -2), q)
        dqkv = torch.stack(
            [dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)],
            dim=2)
        return dqkv, None, None, None


class AttentionDropFn(torch.autograd.Function):
    """AttentionFn with dropout on the probabilities, drawn inside the
    kernel (csrc/philox.h attention scheme). The saved probs tensor is
    bf16(P) with the sign bit set where dropped — P >= 0, so it carries the
    mask at no extra memory and the backward draws nothing."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, mask, p, state, site):
        qkv = qkv.contiguous()
        out, probs = hip_ext().attn_drop_fwd(qkv, heads, scale, mask, state,
                                             p, site)
        ctx.save_for_backward(qkv, probs)
        ctx.scale, ctx.p = scale, p
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, probs = ctx.saved_tensors
        B, S, _, H, D = qkv.shape
        none = (None,) * 6
        if S == 128 and D == 64:
            return (hip_ext().attn_drop_bwd(qkv, dout.contiguous(), probs,
                                            ctx.scale, ctx.p),) + none
        rs = ref.dropout_threshold(ctx.p)[2]
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))  # B,H,S,D
        do = dout.view(B, S, H, D).transpose(1, 2)
        # the sign bit itself, not `< 0`: a dropped +0 is -0
        keep = ~torch.signbit(probs)
        p = probs.abs().float()
        pk = torch.where(keep, probs, torch.zeros((), dtype=probs.dtype,
                                                  device=probs.device))
        dv = (torch.matmul(pk.transpose(-1, -2), do).float() * rs).to(do.dtype)
        dp = torch.matmul(do, v.transpose(-1, -2)).float() * keep * rs
        ds = (dp - (dp * p).sum(-1, keepdim=True)) * p * ctx.scale
        ds = ds.to(do.dtype)
        dq = torch.matmul(ds, k)
        dk = torch.matmul(ds.transpose(-1, -2), q)
        dqkv = torch.stack(
            [dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)],
            dim=2)
        return (dqkv,) + none


def _check_attn_dropout(qkv, p, rng):
    _check_p(p)
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16):
        raise ValueError("attention dropout (p > 0) runs on GPU bf16 only")
    if rng is None:
        raise ValueError("attention dropout (p > 0) needs a DropoutRng")


def attention(qkv, heads, scale, mask=None, p: float = 0.0, rng=None,
              site: int = 0):
    """Fused MHA for S <= 256. p > 0 (GPU bf16 only) drops out the softmax
    output with masks from `rng` at call site `site`; p == 0 is the
    dropout-free kernel itself."""
    if p == 0:
        return AttentionFn.apply(qkv, heads, scale, mask)
    _check_attn_dropout(qkv, p, rng)
    return AttentionDropFn.apply(qkv, heads, scale, mask, p, rng.state, site)


class FlashAttentionFn(torch.autograd.Function):
    """Tiled online-softmax MHA (ops/csrc/flash_attention.hip): any sequence
    length, optional additive key mask [B, S]. Saves qkv, ctx, the per-row
    log-sum-exp [B, H, S] and the mask — no [B, H, S, S] probs; the backward
    recomputes P from lse (deterministic, no atomics).
    qkv: [B, S, 3, H, 64] → ctx [B, S, H·64]."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, mask):
        qkv = qkv.contiguous()
        if qkv.is_cuda and qkv.dtype == torch.bfloat16:
            out, lse = hip_ext().flash_attn_fwd(qkv, heads, scale, mask)
        else:
            out, lse = ref.flash_attention_fwd(qkv, heads, scale, mask)
        ctx.save_for_backward(qkv, out, lse, mask)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mask = ctx.saved_tensors
        if qkv.is_cuda and qkv.dtype == torch.bfloat16:
            dqkv = hip_ext().flash_attn_bwd(qkv, out, dout.contiguous(), lse,
                                            ctx.scale, mask)
        else:
            dqkv = ref.flash_attention_bwd(qkv, out, dout, lse, ctx.scale,
                                           mask)
        return dqkv, None, None, None


class FlashAttentionDropFn(torch.autograd.Function):
    """FlashAttentionFn with dropout on the probabilities. Nothing of the
    mask is saved: the backward kernels draw it again from the random-number
    state the forward read. That state is cloned in forward (16 bytes, a
    device copy: capturable), so an rng.tick() between forward and backward
    cannot desynchronise the two."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, mask, p, state, site):
        qkv = qkv.contiguous()
        state = state.clone()
        out, lse = hip_ext().flash_attn_drop_fwd(qkv, heads, scale, mask,
                                                 state, p, site)
        ctx.save_for_backward(qkv, out, lse, mask, state)
        ctx.scale, ctx.p, ctx.site = scale, p, site
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mask, state = ctx.saved_tensors
        dqkv = hip_ext().flash_attn_drop_bwd(qkv, out, dout.contiguous(), lse,
                                             ctx.scale, mask, state, ctx.p,
                                             ctx.site)
        return (dqkv,) + (None,) * 6


def flash_attention(qkv, heads, scale, mask=None, p: float = 0.0, rng=None,
                    site: int = 0):
    """softmax(Q·Kᵀ·scale + mask)·V for qkv [B, S, 3, H, 64] → [B, S, H·64].

    mask: optional additive key mask [B, S] (0 = keep, a large negative
    such as finfo(float32).min = drop), shared by all heads and query rows.
    CUDA bf16 runs the HIP kernels; anything else the fp32 reference.
    A batch row with NO valid key is outside the contract: its output and
    gradients are only guaranteed to be finite.
    p > 0 (GPU bf16 only) drops out the softmax output with masks from
    `rng` at call site `site`; p == 0 is the dropout-free path itself."""
    if p == 0:
        return FlashAttentionFn.apply(qkv, heads, scale, mask)
    _check_attn_dropout(qkv, p, rng)
    return FlashAttentionDropFn.apply(qkv, heads, scale, mask, p, rng.state,
                                      site)


class FlashAttentionVarlenFn(torch.autograd.Function):
    """FlashAttentionFn over a packed batch (the VARLEN kernels of
    ops/csrc/flash_attention.hip): qkv [T, 3, H, 64] holds the sequences back
    to back, cu_seqlens (int32 [N + 1], on qkv's device) their bounds.
    Saves qkv, ctx, lse [H, T] and cu_seqlens; cu_seqlens is read on the
    device only, so nothing syncs and a captured call replays on new lengths.
    → ctx [T, H·64]."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, heads, scale):
        qkv = qkv.contiguous()
        if qkv.is_cuda and qkv.dtype == torch.bfloat16:
            out, lse = hip_ext().flash_attn_varlen_fwd(qkv, cu_seqlens,
                                                       max_seqlen, heads, scale)
        else:
            out, lse = ref.flash_attention_varlen_fwd(qkv, cu_seqlens,
                                                      max_seqlen, heads, scale)
        ctx.save_for_backward(qkv, out, lse, cu_seqlens)
        ctx.scale, ctx.max_seqlen = scale, max_seqlen
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, cu_seqlens = ctx.saved_tensors
        if qkv.is_cuda and qkv.dtype == torch.bfloat16:
            dqkv = hip_ext().flash_attn_varlen_bwd(
                qkv, out, dout.contiguous(), lse, cu_seqlens, ctx.max_seqlen,
                ctx.scale)
        else:
            dqkv = ref.flash_attention_varlen_bwd(
                qkv, out, dout, lse, cu_seqlens, ctx.max_seqlen, ctx.scale)
        return dqkv, None, None, None, None


class FlashAttentionVarlenDropFn(torch.autograd.Function):
    """FlashAttentionVarlenFn with dropout on the probabilities; the state
    clone and the redrawn masks are those of FlashAttentionDropFn."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, heads, scale, p, state,
                site):
        qkv = qkv.contiguous()
        state = state.clone()
        out, lse = hip_ext().flash_attn_varlen_drop_fwd(
            qkv, cu_seqlens, max_seqlen, heads, scale, state, p, site)
        ctx.save_for_backward(qkv, out, lse, cu_seqlens, state)
        ctx.scale, ctx.max_seqlen, ctx.p, ctx.site = scale, max_seqlen, p, site
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, cu_seqlens, state = ctx.saved_tensors
        dqkv = hip_ext().flash_attn_varlen_drop_bwd(
            qkv, out, dout.contiguous(), lse, cu_seqlens, ctx.max_seqlen,
            ctx.scale, state, ctx.p, ctx.site)
        return (dqkv,) + (None,) * 7


def flash_attention_varlen(qkv, cu_seqlens, max_seqlen, heads, scale,
                           p: float = 0.0, rng=None, site: int = 0):
    """Self-attention over a packed, unpadded batch: qkv [T, 3, H, 64] holds
    N sequences back to back, sequence n in rows cu_seqlens[n] ..
    cu_seqlens[n+1] − 1, each attending to itself only → ctx [T, H·64].

    cu_seqlens: int32 [N + 1] on qkv's device with cu[0] = 0, non-decreasing
    (an empty slot repeats a value) and cu[N] <= T; max_seqlen: a host int no
    sequence exceeds — it sizes the kernels' grid and keys the dropout
    masks. Neither is checked on the GPU, where nothing reads cu_seqlens on
    the host: shapes depend on T, N and max_seqlen only, so a captured call
    replays on other lengths written into cu_seqlens in place.
    Rows at or past cu[N] (the unused tail of a token budget) come back as
    zeros, and so do their gradients.
    CUDA bf16 runs the HIP kernels; anything else the fp32 reference.
    p > 0 (GPU bf16 only): sequence n draws the masks a dense
    [N, max_seqlen] batch draws for batch row n (reference.
    varlen_attn_dropout_keep)."""
    if p == 0:
        return FlashAttentionVarlenFn.apply(qkv, cu_seqlens, max_seqlen, heads,
                                            scale)
    _check_attn_dropout(qkv, p, rng)
    return FlashAttentionVarlenDropFn.apply(qkv, cu_seqlens, max_seqlen, heads,
                                            scale, p, rng.state, site)


class BertLayerFn(torch.autograd.Function):
    """One whole transformer encoder layer (fused QKV → attention →
    out-proj → LN-join → FFN(GELU) → LN-join) as a single autograd node,
    chaining the HIP primitives manually (the ResNet BottleneckFn pattern).

    What the composite buys over per-op autograd, per layer per step:
      - both residual-join backward adds (autograd CUDAFunctor_add over the
        [M, H] activation) fold into the dgrad GEMM epilogues
        (linear_dgrad_acc: dx_join += dy·W in place);
      - autograd bookkeeping for ~8 interior nodes disappears.
    GPU-only; requires S == 128 (fused attention backward) and head_dim 64.
    """

    @staticmethod
    def forward(ctx, x2d, b, s, heads, scale, eps,
                qkv_w, qkv_b, out_w, out_b, ln1_w, ln1_b,
                fc1_w, fc1_b, fc2_w, fc2_b, ln2_w, ln2_b):
        ext = hip_ext()
        qkv = ext.linear_fwd(x2d, qkv_w, qkv_b)
        qkv5 = qkv.view(b, s, 3, heads, 64)
        att, probs = ext.attn_fwd(qkv5, heads, scale, None, True)
        att2 = att.view(b * s, heads * 64)
        o = ext.linear_fwd(att2, out_w, out_b)
        y1, s1, mean1, rstd1 = ext.layernorm_add_fwd(x2d, o, ln1_w, ln1_b,
                                                     eps)
        g, deriv = ext.linear_gelu_fwd(y1, fc1_w, fc1_b)
        z = ext.linear_fwd(g, fc2_w, fc2_b)
        y2, s2, mean2, rstd2 = ext.layernorm_add_fwd(y1, z, ln2_w, ln2_b,
                                                     eps)
        ctx.save_for_backward(x2d, qkv5, probs, att2, s1, mean1, rstd1,
                              y1, g, deriv, s2, mean2, rstd2,
                              qkv_w, out_w, ln1_w, fc1_w, fc2_w, ln2_w)
        ctx.dims = (b, s, heads, scale)
        return y2

    @staticmethod
    def backward(ctx, dy2):
        (x2d, qkv5, probs, att2, s1, mean1, rstd1, y1, g, deriv,
         s2, mean2, rstd2, qkv_w, out_w, ln1_w, fc1_w, fc2_w,
         ln2_w) = ctx.saved_tensors
        b, s, heads, scale = ctx.dims
        ext = hip_ext()
        dy2 = dy2.contiguous()
        # LN2 join: dxs2 is the grad of (y1 + z) — it feeds BOTH the
        # residual (y1) and the FFN branch; the FFN dx accumulates into it
        dxs2, dg_ln2, db_ln2 = ext.layernorm_bwd(dy2, s2, ln2_w, mean2,
                                                 rstd2)
        dw2, db2 = ext.linear_wgrad_only(dxs2, g)
        dh = ext.linear_gelu_dgrad(dxs2, fc2_w, deriv)
        dw1, db1 = ext.linear_wgrad_only(dh, y1)
        dy1 = ext.linear_dgrad_acc(dh, fc1_w, dxs2)  # dxs2 += dh @ w1
        # LN1 join: same pattern with the attention branch
        dxs1, dg_ln1, db_ln1 = ext.layernorm_bwd(dy1, s1, ln1_w, mean1,
                                                 rstd1)
        dow, dob = ext.linear_wgrad_only(dxs1, att2)
        do_ = ext.linear_dgrad(dxs1, out_w)
        dqkv = ext.attn_bwd(qkv5, do_, probs, scale)
        dqkv2 = dqkv.view(b * s, -1)
        dqw, dqb = ext.linear_wgrad_only(dqkv2, x2d)
        dx = ext.linear_dgrad_acc(dqkv2, qkv_w, dxs1)  # dxs1 += dqkv @ Wqkv
        return (dx, None, None, None, None, None,
                dqw, dqb, dow, dob, dg_ln1, db_ln1,
                dw1, db1, dw2, db2, dg_ln2, db_ln2)


def bert_layer(x2d, b, s, heads, scale, eps, qkv_w, qkv_b, out_w, out_b,
               ln1_w, ln1_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_w, ln2_b):
    return BertLayerFn.apply(x2d, b, s, heads, scale, eps, qkv_w, qkv_b,
                             out_w, out_b, ln1_w, ln1_b, fc1_w, fc1_b,
                             fc2_w, fc2_b, ln2_w, ln2_b)


class LayerNormAddFn(torch.autograd.Function):
    """y = LN(a + b): the transformer residual join fused into the LN
    forward (the separate add was an extra full read+write of the [M, H]
    activation per join). Backward: dLN flows identically to both addends."""

    @staticmethod
    def forward(ctx, a, b, weight, bias, eps: float):
        y, s, mean, rstd = hip_ext().layernorm_add_fwd(a, b, weight, bias, eps)
        ctx.save_for_backward(s, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        s, weight, mean, rstd = ctx.saved_tensors
        dx, dg, db = hip_ext().layernorm_bwd(dy, s, weight, mean, rstd)
        return dx, dx, dg, db, None


def layer_norm_add(a, b, weight, bias, eps: float = 1e-12):
    return LayerNormAddFn.apply(a, b, weight, bias, eps)


class DropoutRng:
    """Device random-number state of the dropout kernels: an int64 tensor
    (seed, offset). The kernels read both from device memory on every
    launch and tick() advances offset with a one-thread kernel, so a train
    step captured into a graph draws fresh masks on each replay (a seed or
    offset passed as a launch argument would be frozen at capture) — the
    optimizers' device step state, applied to random numbers."""

    def __init__(self, seed: int, device):
        self.state = torch.tensor(self._signed(seed, 0), dtype=torch.int64,
                                  device=device)

    @staticmethod
    def _signed(seed: int, offset: int):
        # any Python int → the int64 bit pattern the kernels read as uint64
        return [((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)
                for v in (seed, offset)]

    def tick(self):
        """offset += 1 on the device, in stream order (capturable)."""
        hip_ext().rng_tick(self.state)

    def get_state(self):
        """(seed, offset) as unsigned 64-bit ints. Synchronizes: not for use
        under graph capture."""
        if self.state.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DropoutRng.get_state() synchronizes and must "
                               "not run under graph capture")
        seed, offset = (int(v) % (1 << 64) for v in self.state.tolist())
        return seed, offset

    def set_state(self, seed: int, offset: int):
        self.state.copy_(torch.tensor(self._signed(seed, offset),
                                      dtype=torch.int64))


def _check_p(p: float) -> None:
    ref.dropout_threshold(p)  # ValueError outside the kernels' contract


class DropoutFn(torch.autograd.Function):
    """Philox dropout of a contiguous bf16 tensor (csrc/dropout.hip). Saves
    the keep bitmask (one byte per 8 elements); the backward reads it and
    never regenerates it. Returns (y, mask)."""

    @staticmethod
    def forward(ctx, x, p: float, state, site: int):
        y, mask = hip_ext().dropout_fwd(x, state, p, site)
        ctx.save_for_backward(mask)
        ctx.p = p
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)
        return y, mask

    @staticmethod
    def backward(ctx, dy, _dmask=None):
        (mask,) = ctx.saved_tensors
        return hip_ext().dropout_bwd(dy.contiguous(), mask, ctx.p), None, None, None


def dropout_with_mask(x, p: float, rng: DropoutRng, site: int):
    """(y, mask): y = keep ? x / (1 - p_eff) : 0 and the uint8 keep bitmask
    [numel/8], bit j of byte o = element 8·o + j. p > 0, GPU bf16 only."""
    _check_p(p)
    return DropoutFn.apply(x.contiguous(), p, rng.state, site)


def dropout(x, p: float, rng: DropoutRng, site: int):
    """Dropout with masks from the device Philox state `rng` at call site
    `site` (distinct sites draw independent masks within a step; rng.tick()
    separates steps). p == 0 is the identity."""
    _check_p(p)
    if p == 0:
        return x
    return dropout_with_mask(x, p, rng, site)[0]


class LayerNormDropAddFn(torch.autograd.Function):
    """y = LN(a + dropout(b)): LayerNormAddFn with the branch's dropout
    drawn inside the join kernel (no separate pass over the [M, H]
    activation); backward writes da and db = da·keep/(1 - p_eff) from one
    dx kernel off the saved bitmask. Returns (y, mask)."""

    @staticmethod
    def forward(ctx, a, b, weight, bias, eps: float, p: float, state, site: int):
        y, s, mean, rstd, mask = hip_ext().layernorm_drop_add_fwd(
            a, b, weight, bias, eps, state, p, site)
        ctx.save_for_backward(s, weight, mean, rstd, mask)
        ctx.p = p
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)
        return y, mask

    @staticmethod
    def backward(ctx, dy, _dmask=None):
        s, weight, mean, rstd, mask = ctx.saved_tensors
        da, db, dg, dbeta = hip_ext().layernorm_drop_add_bwd(
            dy.contiguous(), s, weight, mean, rstd, mask, ctx.p)
        return da, db, dg, dbeta, None, None, None, None


def layer_norm_drop_add_with_mask(a, b, weight, bias, eps: float, p: float,
                                  rng: DropoutRng, site: int):
    """(y, mask) of LayerNormDropAddFn; mask is uint8 [M, N/8]. p > 0."""
    _check_p(p)
    return LayerNormDropAddFn.apply(a.contiguous(), b.contiguous(), weight,
                                    bias, eps, p, rng.state, site)


def layer_norm_drop_add(a, b, weight, bias, eps: float = 1e-12, p: float = 0.0,
                        rng: DropoutRng = None, site: int = 0):
    """y = LN(a + dropout(b, p)); p == 0 is layer_norm_add itself."""
    _check_p(p)
    if p == 0:
        return layer_norm_add(a, b, weight, bias, eps)
    return layer_norm_drop_add_with_mask(a, b, weight, bias, eps, p, rng,
                                         site)[0]
