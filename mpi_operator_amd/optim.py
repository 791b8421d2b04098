"""FusedSGD — momentum SGD with fp32 master weights and a single fused
multi-tensor HIP kernel per step on GPU (SURVEY.md §2.3 N7 'fused SGD-momentum
update'; the reference's workload used tf SGD inside the external image).

bf16 parameters keep an fp32 master + fp32 momentum in optimizer state; the
kernel updates master & momentum and refreshes the bf16 working copy in one
pass over HBM.

FusedAdamW / FusedLAMB follow the same conventions, and keep everything that
depends on the step number (step count, bias corrections, clip scale, and the
learning rate itself) in a per-group DEVICE scalar block that the kernels
read: a captured hipGraph of ``step()`` therefore replays correct steps,
where a host-computed ``1 - beta**t`` would be frozen at capture time."""
from __future__ import annotations

import torch

from .ops import adamw_step, lamb_step, sgd_momentum_step
from .ops import functional as _Fx
from .ops import reference as _ref


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr: float, momentum: float = 0.9,
                 weight_decay: float = 0.0, nesterov: bool = False):
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        # side-stream wgrad mode: grads may still be in flight on the side
        # stream — order them before the fused update (no-op otherwise)
        _Fx.join_wgrad_stream()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            masters, grads, momenta, outs = [], [], [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32)
                    if p.dtype != torch.float32:
                        st["master"] = p.detach().float().clone()
                if p.dtype != torch.float32:
                    masters.append(st["master"])
                    outs.append(p.data)
                else:
                    masters.append(p.data)
                    outs.append(None)
                grads.append(p.grad)
                momenta.append(st["momentum_buffer"])
            if masters:
                sgd_momentum_step(masters, grads, momenta, outs, group["lr"],
                                  group["momentum"], group["weight_decay"], group["nesterov"])
        return loss


class _FusedAdaptive(torch.optim.Optimizer):
    """Shared body of FusedAdamW / FusedLAMB.

    Per param: fp32 ``exp_avg`` / ``exp_avg_sq`` (+ fp32 ``master`` for
    non-fp32 params) in ``self.state``. Per group: one persistent scalar
    block (layout ``ops.reference.OPT_*``) owned by the optimizer, whose step
    slot is exposed as the int32 device tensor ``group["step"]`` so that
    ``state_dict()`` carries it. The block and the reduction scratch are
    allocated by the first ``step()``, which therefore must run eagerly —
    capture a graph only after one warm-up step."""

    _lamb = False

    def __init__(self, params, lr, betas, eps, weight_decay, adam_w_mode, max_grad_norm):
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid betas {betas}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        adam_w_mode=bool(adam_w_mode), max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        self._blocks = {}    # group index -> scalar block
        self._scratch = {}   # group index -> (partials, ratio)
        self._lr_dev = {}    # group index -> lr last written to the block

    # -- device step state --------------------------------------------------
    @staticmethod
    def _capturing(device) -> bool:
        return device.type == "cuda" and torch.cuda.is_current_stream_capturing()

    def _block(self, gi, group):
        blk = self._blocks.get(gi)
        if blk is None:
            device = group["params"][0].device
            if self._capturing(device):
                raise RuntimeError(
                    f"{type(self).__name__}: the first step() allocates optimizer state "
                    "and must not run under graph capture; run one eager step first")
            blk = torch.zeros(_ref.OPT_SCALARS, dtype=torch.float32, device=device)
            blk[_ref.OPT_CLIP] = 1.0
            self._blocks[gi] = blk
            params = [p for p in group["params"] if p.requires_grad]
            if device.type == "cuda":
                nb = _Fx.optim_block_count(params)
                self._scratch[gi] = (
                    torch.zeros(3 * nb if self._lamb else nb, dtype=torch.float32, device=device),
                    torch.ones(len(params), dtype=torch.float32, device=device))
            else:
                self._scratch[gi] = (None, None)
        group["step"] = blk.view(torch.int32)[_ref.OPT_STEP:_ref.OPT_STEP + 1]
        return blk

    def _refresh_group(self, gi, group):
        blk = self._blocks.get(gi)
        if blk is None:
            return
        lr = float(group["lr"])
        if self._lr_dev.get(gi) != lr and not self._capturing(blk.device):
            blk[_ref.OPT_LR:_ref.OPT_LR + 1].fill_(lr)
            self._lr_dev[gi] = lr

    def refresh_hyperparams(self):
        """Write each group's current ``lr`` to its device scalar block.
        ``step()`` does this itself when it runs eagerly; a loop that REPLAYS a
        captured graph calls this after changing ``group["lr"]`` so the
        schedule takes effect on the next replay."""
        for gi, group in enumerate(self.param_groups):
            self._refresh_group(gi, group)

    # -- checkpointing --------------------------------------------------------
    def load_state_dict(self, state_dict):
        old = {p: dict(st) for p, st in self.state.items()}
        super().load_state_dict(state_dict)
        # torch casts loaded per-param state to the PARAM's dtype (and may
        # alias the source tensors): take the fp32 moments and masters from
        # the saved values instead — INTO the tensors this optimizer already
        # owns where it has them (a captured graph holds their addresses),
        # into private copies otherwise
        saved_state = state_dict["state"]
        for gi, (group, sg) in enumerate(zip(self.param_groups, state_dict["param_groups"])):
            for p, pid in zip(group["params"], sg["params"]):
                src = saved_state.get(pid)
                if src is None:
                    continue
                for k in ("exp_avg", "exp_avg_sq", "master"):
                    if k not in src:
                        continue
                    dst = old.get(p, {}).get(k)
                    if dst is not None and dst.shape == src[k].shape:
                        dst.copy_(src[k])
                    else:
                        dst = src[k].detach().to(device=p.device, dtype=torch.float32, copy=True)
                    self.state[p][k] = dst
            # likewise the step count goes into the existing scalar block;
            # lr is rewritten by the next refresh
            step = sg.get("step")
            step = int(step) if step is not None else 0
            if step or gi in self._blocks:
                self._block(gi, group).view(torch.int32)[_ref.OPT_STEP] = step
            else:
                group.pop("step", None)
            self._lr_dev.pop(gi, None)

    # -- step -------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        # side-stream wgrad mode: grads may still be in flight on the side
        # stream — order them before the fused update (no-op otherwise)
        _Fx.join_wgrad_stream()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            masters, grads, exp_avgs, exp_avg_sqs, outs = [], [], [], [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                    if p.dtype != torch.float32:
                        st["master"] = p.detach().float().clone()
                if p.dtype != torch.float32:
                    masters.append(st["master"])
                    outs.append(p.data)
                else:
                    masters.append(p.data)
                    outs.append(None)
                grads.append(p.grad)
                exp_avgs.append(st["exp_avg"])
                exp_avg_sqs.append(st["exp_avg_sq"])
            if not masters:
                continue
            blk = self._block(gi, group)
            self._refresh_group(gi, group)
            partials, ratio = self._scratch[gi]
            beta1, beta2 = group["betas"]
            hyper = (beta1, beta2, group["eps"], group["weight_decay"],
                     group["adam_w_mode"], group["max_grad_norm"])
            if self._lamb:
                lamb_step(masters, grads, exp_avgs, exp_avg_sqs, outs, blk, partials, ratio, *hyper)
            else:
                adamw_step(masters, grads, exp_avgs, exp_avg_sqs, outs, blk, partials, *hyper)
        return loss


class FusedAdamW(_FusedAdaptive):
    """AdamW (``adam_w_mode=True``, decoupled decay — torch.optim.AdamW's
    algebra) or Adam with L2 decay (``adam_w_mode=False`` — torch.optim.Adam
    with weight_decay) as one fused multi-tensor HIP kernel per step plus a
    one-block step-state tick. ``max_grad_norm`` clips by the group's global
    grad norm (torch.nn.utils.clip_grad_norm_ semantics) inside the kernels."""

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, adam_w_mode: bool = True,
                 max_grad_norm: float | None = None):
        super().__init__(params, lr, betas, eps, weight_decay, adam_w_mode, max_grad_norm)


class FusedLAMB(_FusedAdaptive):
    """LAMB: Adam moments with a per-tensor trust ratio ||w|| / ||u||, as two
    fused multi-tensor passes and a per-tensor reduce. The update ``u`` is
    recomputed in the second pass rather than stored, and every norm is a
    fixed-order sum over a persistent partials slab (bit-reproducible)."""

    _lamb = True

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, adam_w_mode: bool = True,
                 max_grad_norm: float | None = None):
        super().__init__(params, lr, betas, eps, weight_decay, adam_w_mode, max_grad_norm)
