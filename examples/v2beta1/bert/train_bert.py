#!/usr/bin/env python3
"""BERT-Large pretraining on the MI355X stack — BASELINE.json config 4:
2 worker pods × 4 GPUs each on one node (SSH hostfile + multi-pod
rendezvous; RCCL stays on xGMI across pods because both pods share
/dev/kfd). Synthetic MLM+NSP data, bf16, sequences/sec reported.

--varlen feeds ragged batches (lengths uniform in [--min-len, --seq]):
`padded` as [batch, seq] plus a key mask, `packed` as the same sequences
unpadded in one [1, batch*seq] token buffer with cu_seqlens (no work on
padding). Both report real (non-pad) tokens/sec."""
import argparse
import os
import sys
import time

import torch

# allow running straight from a source checkout (python examples/.../x.py)
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "..")))

from mpi_operator_amd import parallel as hvd
from mpi_operator_amd.models.bert import (bert_large, bert_base, bert_param_groups,
                                          pack_padded_batch, to_mi355x_bert)
from mpi_operator_amd.optim import FusedAdamW, FusedLAMB, FusedSGD


def synthetic_batch(batch, seq, vocab, device):
    ids = torch.randint(0, vocab, (batch, seq), device=device)
    type_ids = torch.zeros_like(ids)
    mlm_labels = torch.full_like(ids, -100)
    mask = torch.rand(batch, seq, device=device) < 0.15
    mlm_labels[mask] = ids[mask]
    nsp = torch.randint(0, 2, (batch,), device=device)
    return ids, type_ids, mlm_labels, nsp


def ragged_batches(n, batch, seq, min_len, vocab, device, seed, packed, max_seq):
    """n ragged batches as (model args, model kwargs, real tokens), built
    ahead of the timed loop the way a data pipeline runs ahead of the step
    (pack_padded_batch reads the lengths on the host). The lengths come from
    a seeded CPU generator, so `padded` and `packed` see the same ones."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        lens = torch.randint(min_len, seq + 1, (batch,), generator=g)
        ids, type_ids, mlm_labels, nsp = synthetic_batch(batch, seq, vocab, device)
        mask = (torch.arange(seq)[None] < lens[:, None]).to(device)
        mlm_labels = torch.where(mask, mlm_labels, torch.full_like(mlm_labels, -100))
        if packed:
            pk = pack_padded_batch(ids, type_ids, mask, mlm_labels,
                                   token_budget=batch * seq, max_sequences=batch,
                                   max_seq=max_seq)
            # max_seqlen = seq, not this batch's longest: every step has one shape
            out.append(((pk.ids, pk.type_ids, None, pk.mlm_labels, nsp),
                        dict(cu_seqlens=pk.cu_seqlens, max_seqlen=seq,
                             position_ids=pk.position_ids), int(lens.sum())))
        else:
            out.append(((ids, type_ids, mask.long(), mlm_labels, nsp), {},
                        int(lens.sum())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert_large", choices=["bert_large", "bert_base"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8, help="per-GPU sequences")
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "adamw", "lamb"])
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="hidden-state dropout (published recipes use 0.1)")
    ap.add_argument("--attn-dropout", type=float, default=0.0,
                    help="dropout on the attention probabilities (published "
                         "recipes use 0.1)")
    ap.add_argument("--seed", type=int, default=0,
                    help="dropout seed; each rank adds its rank")
    ap.add_argument("--varlen", default="off", choices=["off", "padded", "packed"],
                    help="ragged synthetic batches: padded to --seq with a key "
                         "mask, or packed without padding (cu_seqlens)")
    ap.add_argument("--min-len", type=int, default=64,
                    help="--varlen: lengths are uniform in [min-len, seq]")
    args = ap.parse_args()
    if args.varlen != "off" and not 1 <= args.min_len <= args.seq:
        ap.error("--min-len must be in [1, --seq]")

    hvd.init()
    use_cuda = torch.cuda.is_available()
    device = f"cuda:{hvd.local_rank()}" if use_cuda else "cpu"

    model = (bert_large if args.model == "bert_large" else bert_base)(
        args.dropout, args.attn_dropout)
    if use_cuda:
        model = to_mi355x_bert(model, device)
    model.train()
    # per-rank masks: the state is not a buffer, so broadcast_parameters
    # below leaves it alone
    model.seed_dropout(args.seed + hvd.rank())
    if args.optimizer == "sgd":
        opt = FusedSGD(model.parameters(), lr=1e-4, momentum=0.9)
    elif args.optimizer == "adamw":
        opt = FusedAdamW(bert_param_groups(model, 0.01), lr=1e-4)
    else:
        opt = FusedLAMB(bert_param_groups(model, 0.01), lr=2e-3)
    opt = hvd.DistributedOptimizer(opt, model.named_parameters())
    hvd.broadcast_parameters(model, 0)

    vocab = model.cfg.vocab_size

    def step():
        ids, type_ids, mlm_labels, nsp = synthetic_batch(args.batch, args.seq, vocab, device)
        opt.zero_grad()
        mlm_logits, nsp_logits = model(ids, type_ids)
        loss = model.loss(mlm_logits, nsp_logits, mlm_labels, nsp)
        loss.backward()
        opt.step()
        return loss

    real_tokens = 0
    if args.varlen != "off":
        batches = ragged_batches(args.warmup + args.steps, args.batch, args.seq,
                                 args.min_len, vocab, device, args.seed,
                                 args.varlen == "packed", model.cfg.max_seq)
        real_tokens = sum(b[2] for b in batches[args.warmup:])
        feed = iter(batches)

        def step():  # noqa: F811 — labels-in-forward: the fused MLM head
            a, kw, _ = next(feed)
            opt.zero_grad()
            loss = model(*a, **kw)
            loss.backward()
            opt.step()
            return loss

    for _ in range(args.warmup):
        step()
    if use_cuda:
        torch.cuda.synchronize()
    hvd.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    if use_cuda:
        torch.cuda.synchronize()
    hvd.barrier()
    dt = time.perf_counter() - t0

    seq_per_sec = args.batch * hvd.size() * args.steps / dt
    if hvd.rank() == 0:
        print(f"bert: {seq_per_sec:.1f} sequences/sec over {hvd.size()} GPUs "
              f"({dt / args.steps * 1000:.1f} ms/step, loss {float(loss):.3f})", flush=True)
        if args.varlen != "off":
            tok = real_tokens * hvd.size() / dt
            share = 1 - real_tokens / (args.batch * args.seq * args.steps)
            print(f"bert varlen={args.varlen}: {tok:.0f} real tokens/sec "
                  f"(rank 0's lengths; {share:.1%} of batch*seq is padding)",
                  flush=True)


if __name__ == "__main__":
    main()
