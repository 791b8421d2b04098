#!/usr/bin/env python3
"""Flagship benchmark: ResNet101 synthetic-ImageNet training images/sec —
the reference's headline metric (tf_cnn_benchmarks ResNet101,
bs=64/GPU, synthetic data, SGD, Horovod allreduce; 308.27 images/sec on two
2019-class GPUs).

Run (driver contract):
    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
For N>1 the driver launches this under torch.distributed.run with one rank
per GPU; ranks rendezvous over env:// and allreduce over RCCL/xGMI.

A plain run sets up, warms up, times exactly K steps and prints ONE JSON line
from rank 0 — nothing else. --dump-outputs DIR additionally writes what the
last timed step computed (see dump_outputs). --full is where any measurement
beyond the headline figure belongs; the flagship run has none today, so the
flag is accepted and changes nothing.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BASELINE_TOTAL_IMAGES_PER_SEC = 308.27  # reference README.md:211-213 (2 GPUs)

SEED = 1234                    # model init; SyntheticImageData seeds itself
PARAM_SAMPLE = 8 * 1024 * 1024  # dumped parameter elements (32 MiB as fp32)


def dump_outputs(out_dir, model, loss, logits):
    """Write what a caller of the timed training step receives after the
    last timed step, as float32 .npy files (well under 64 MB in total):

      loss.npy    the step's loss (scalar)
      logits.npy  the step's [batch, classes] logits
      params.npy  the updated model parameters, flattened in
                  model.parameters() order; when there are more than
                  PARAM_SAMPLE of them, a fixed sample drawn with SEED

    Inputs and initial weights are seeded, so two builds run with the same
    arguments can be compared file for file."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    with torch.no_grad():
        flat = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
        if flat.numel() > PARAM_SAMPLE:
            g = torch.Generator(device="cpu").manual_seed(SEED)
            idx = torch.randint(0, flat.numel(), (PARAM_SAMPLE,), generator=g)
            flat = flat[idx.to(flat.device)]
        arrays = {
            "loss": loss.detach().float().reshape(()),
            "logits": logits.detach().float(),
            "params": flat,
        }
        for name, t in arrays.items():
            np.save(os.path.join(out_dir, name + ".npy"),
                    t.cpu().numpy().astype(np.float32, copy=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # >=100 graph-replayed steps: a multi-second timed region that coarse
    # SMI samplers can't miss (the 20-step default produced a 0.38 s window)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="resnet101", choices=["resnet101", "resnet50"])
    ap.add_argument("--batch", type=int, default=64, help="per-GPU batch")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--impl", default="hip", choices=["hip", "torch"],
                    help="hip: hand-written CDNA4 kernels (default, the judged path); "
                         "torch: stock PyTorch-ROCm ops for A/B comparison")
    ap.add_argument("--bucket-mb", type=int, default=28)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's loss, logits "
                         "and updated parameters to DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline figure "
                         "(none for this workload today; a plain run stays lean)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    from mpi_operator_amd import parallel as hvd
    from mpi_operator_amd import models
    from mpi_operator_amd.trainer import SyntheticImageData, make_trainer, timed_steps

    hvd.init()
    use_cuda = torch.cuda.is_available()
    # --gpus N>1 REQUIRES an N-rank process group (the driver's torchrun
    # contract). A single process claiming N GPUs would multiply
    # global_batch by N while computing on one GPU — refuse to inflate.
    if use_cuda and args.gpus > 1 and hvd.size() != args.gpus:
        raise SystemExit(
            f"bench.py --gpus {args.gpus} requires world_size={args.gpus} "
            f"(got {hvd.size()}); launch via torch.distributed.run")
    n_gpus = hvd.size() if hvd.size() > 1 else args.gpus

    if args.impl == "torch":
        os.environ["MPIAMD_IMPL"] = "torch"
        from mpi_operator_amd.models import resnet_torch
        model_fn = getattr(resnet_torch, args.model)
    else:
        model_fn = getattr(models, args.model)

    batch, image = args.batch, args.image
    torch.manual_seed(SEED)  # identical initial weights from run to run
    if use_cuda:
        device = f"cuda:{hvd.local_rank()}"
        torch.cuda.set_device(device)
        model = model_fn()
        if args.impl == "hip":
            model = models.to_mi355x(model, device)
        else:
            # stock-PyTorch baseline: fp32 params + bf16 autocast (MIOpen path)
            model = model.to(device=device, memory_format=torch.channels_last)
            fwd = model.forward

            def autocast_fwd(x, _fwd=fwd):
                with torch.autocast("cuda", torch.bfloat16):
                    return _fwd(x)
            model.forward = autocast_fwd
        dtype = torch.bfloat16
    else:
        # CPU smoke mode (no GPU in the build container): tiny shapes, same path
        device, dtype = "cpu", torch.float32
        batch, image = 2, 64
        model = model_fn()
    model.train()

    p2p_busbw = None
    if use_cuda and hvd.size() > 1:
        # same-node P2P guard: fail loudly if RCCL fell back
        # to TCP for ranks sharing a node (multi-pod config 4)
        from mpi_operator_amd.parallel.p2p import verify_p2p
        p2p_busbw = verify_p2p().get("busbw_gb")

    data = SyntheticImageData(batch, image, 1000, device=device, dtype=dtype,
                              channels_last=use_cuda and args.impl == "hip")
    if use_cuda and args.impl == "torch":
        # the stock stem takes RGB, not the NHWC8-padded input of the hip path
        data.x = data.x.contiguous(memory_format=torch.channels_last)
    dopt = make_trainer(model, bucket_bytes=args.bucket_mb * 1024 * 1024)
    last = {}
    if args.dump_outputs:
        # keep the step's logits reachable: under graph replay this is the
        # static tensor, so after the run it holds the last timed step's
        # values. detach() is required — a reference to the attached output
        # keeps the previous step's autograd graph (and its AccumulateGrad
        # nodes, bound to the eager stream) alive into graph capture.
        model.register_forward_hook(
            lambda m, inp, out: last.__setitem__("logits", out.detach()))
    res = timed_steps(model, dopt, data, args.steps, args.warmup, device)
    if args.dump_outputs and hvd.rank() == 0:
        dump_outputs(args.dump_outputs, model, torch.tensor(res["loss"]), last["logits"])

    global_batch = batch * n_gpus
    images_per_sec = global_batch * args.steps / res["elapsed"]
    ms_per_step = res["elapsed"] / args.steps * 1000.0

    if hvd.rank() == 0:
        out = {
            "metric": "images/sec",
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(images_per_sec / BASELINE_TOTAL_IMAGES_PER_SEC, 3),
            "dtype": "bf16" if use_cuda else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": global_batch,
                "image": image,
                "parallelism": f"dp{n_gpus}",
                "impl": args.impl,
                "graph": res.get("graph", False),
                "loss": res["loss"],
                "p2p_busbw_gb": p2p_busbw,
            },
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
