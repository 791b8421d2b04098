"""BERT-Large for MI355X — the config-4 workload of BASELINE.json
("BERT-Large Horovod, 2 worker pods × 4 GPUs each"). The reference ships no
BERT code (its workload layer is out-of-tree Horovod images); this is the
stack's own transformer family, built the same MI355X-first way as ResNet:

- every GEMM-shaped op (QKV projection, attention output, FFN in/out, MLM
  head) goes through the hand-written MFMA NT-GEMM HIP kernel
  (ops/csrc/gemm.hip) via ops.functional.linear;
- bf16 activations/params end-to-end (fp32 master weights live in FusedSGD);
- attention scores use torch.matmul (rocBLAS batched GEMM on ROCm) — the
  batched-GEMM shapes are library-friendly; fusing them by hand is a later
  optimization, and the dispatch seam is ops.functional.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import functional as Fx


import os as _os

# default ON since the LN-bwd split + per-channel reduce: 929 vs 893
# seq/s same-box (MPIAMD_FUSED_LN=0 reverts to torch-native LN)
_FUSED_LN = _os.environ.get("MPIAMD_FUSED_LN", "1") == "1"


# MPIAMD_FLASH_ATTN (read per call): route seq > 256 and key-masked
# attention through ops/csrc/flash_attention.hip instead of the eager chain.
# Default ON: 330 vs 230 seq/s and 6.9 vs 11.6 GiB peak at BERT-Large
# seq 512 bs 8, same box (profiles/BENCH_HISTORY.md)
_FLASH_ATTN_DEFAULT = "1"


class LayerNorm(nn.Module):
    """LayerNorm with fp32 statistics on the hand-written HIP kernel
    (ops/csrc/layernorm.hip). Default since round 2: the backward's dx
    pass was un-capped from the dgamma/dbeta slab grid (split kernels) and
    the slab reduce made per-channel — fused now measures 929 vs 893
    seq/s against torch-native on BERT-Large (MPIAMD_FUSED_LN=0 reverts)."""

    def __init__(self, n: int, eps: float = 1e-12):
        super().__init__()
        self.n, self.eps = n, eps
        self.weight = nn.Parameter(torch.ones(n))
        self.bias = nn.Parameter(torch.zeros(n))

    def forward(self, x):
        if _FUSED_LN and x.is_cuda and x.dtype == torch.bfloat16:
            return Fx.layer_norm(x, self.weight.float(), self.bias.float(),
                                 self.eps)
        return F.layer_norm(x.float(), (self.n,), self.weight.float(),
                            self.bias.float(), self.eps).to(x.dtype)


def _dropout(x, p, rng, site):
    """Hidden-state dropout at one call site: the Philox HIP kernel for GPU
    bf16 (masks from the model's DropoutRng), torch's generator otherwise —
    the same semantics without bit-compatibility."""
    if rng is not None and x.is_cuda and x.dtype == torch.bfloat16:
        return Fx.dropout(x, p, rng, site)
    return F.dropout(x, p, training=True)


@dataclass
class BertConfig:
    vocab_size: int = 30522
    hidden: int = 1024
    layers: int = 24
    heads: int = 16
    intermediate: int = 4096
    max_seq: int = 512
    type_vocab: int = 2
    # Hidden-state dropout, applied in train() at three kinds of site: after
    # the embedding LayerNorm, and on the attention-output and FFN-output
    # branches ahead of their residual joins.
    # 0.0 = none: benchmarks run dropout-free (synthetic data).
    dropout: float = 0.0
    # Dropout on the attention probabilities (the fourth site of the
    # published recipe), applied in train(): drawn inside the attention
    # kernels on GPU bf16, F.dropout on the eager chain's probs otherwise.
    attn_dropout: float = 0.0
    eps: float = 1e-12


def bert_large(dropout: float = 0.0,
               attn_dropout: float = 0.0) -> "BertForPreTraining":
    return BertForPreTraining(BertConfig(dropout=dropout,
                                         attn_dropout=attn_dropout))


def bert_base(dropout: float = 0.0,
              attn_dropout: float = 0.0) -> "BertForPreTraining":
    return BertForPreTraining(BertConfig(hidden=768, layers=12, heads=12, intermediate=3072,
                                         dropout=dropout,
                                         attn_dropout=attn_dropout))


class BertLinear(nn.Module):
    """Linear over the HIP NT-GEMM for (B·S, in) × (out, in)ᵀ shapes.

    Accepts (..., in_f); flattens leading dims for the 2-D kernel."""

    def __init__(self, in_f: int, out_f: int):
        super().__init__()
        w = torch.empty(out_f, in_f)
        nn.init.normal_(w, std=0.02)
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(out_f))

    def forward(self, x):
        lead = x.shape[:-1]
        y = Fx.linear(x.reshape(-1, x.shape[-1]).contiguous(), self.weight, self.bias)
        return y.reshape(*lead, -1)


class SelfAttention(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.heads = cfg.heads
        self.head_dim = cfg.hidden // cfg.heads
        # fused QKV: one big GEMM instead of three (3× fewer kernel launches,
        # one pass over the activations)
        self.qkv = BertLinear(cfg.hidden, 3 * cfg.hidden)
        self.out = BertLinear(cfg.hidden, cfg.hidden)
        self.scale = 1.0 / math.sqrt(self.head_dim)

    def _packed(self, qkv, cu_seqlens, max_seqlen, hip, p, rng, site):
        """Attention over a packed batch: qkv [1, T, 3, nh, hd], sequence n
        in rows cu_seqlens[n]..cu_seqlens[n+1]−1 → ctx [1, T, h], zeros at
        or past cu_seqlens[-1]."""
        _, t, _, nh, hd = qkv.shape
        if hip:
            # no host read of cu_seqlens: graph-safe
            ctx = Fx.flash_attention_varlen(
                qkv.view(t, 3, nh, hd), cu_seqlens, max_seqlen, nh, self.scale,
                p, rng, site)
            return ctx.view(1, t, nh * hd)
        # eager per-sequence chain (reads cu_seqlens on the host)
        cu = [int(c) for c in cu_seqlens.tolist()]
        parts = []
        for a, e in zip(cu, cu[1:]):
            if e == a:
                continue
            q, k, v = (qkv[0, a:e, i].transpose(0, 1) for i in range(3))
            scores = torch.matmul(q, k.transpose(-1, -2)) * self.scale
            probs = torch.softmax(scores.float(), dim=-1).to(v.dtype)
            if p > 0:
                probs = F.dropout(probs, p, training=True)
            parts.append(torch.matmul(probs, v).transpose(0, 1)
                         .reshape(e - a, nh * hd))
        if cu[-1] < t:
            parts.append(qkv.new_zeros(t - cu[-1], nh * hd))
        return torch.cat(parts, dim=0)[None]

    def forward(self, x, attn_mask=None, p=0.0, rng=None, site=0, *,
                cu_seqlens=None, max_seqlen=None):
        """p, rng, site: dropout on the attention probabilities (p = 0
        outside training). The HIP kernels draw it themselves from `rng` at
        `site`; without an rng (CPU, other dtypes) the eager chain applies
        F.dropout to probs.
        cu_seqlens (int32 [N + 1]), max_seqlen: x is a packed batch
        [1, T, hidden] of N sequences that attend to themselves only (see
        Fx.flash_attention_varlen); there is no attn_mask then."""
        b, s, h = x.shape
        qkv = self.qkv(x).view(b, s, 3, self.heads, self.head_dim)
        hip = (x.is_cuda and x.dtype == torch.bfloat16 and self.head_dim == 64
               and (p == 0 or rng is not None))
        if cu_seqlens is not None:
            if attn_mask is not None:
                raise ValueError("a packed batch (cu_seqlens) has no pad "
                                 "keys: attn_mask must be None")
            if b != 1:
                raise ValueError(f"a packed batch is [1, T, hidden], got "
                                 f"{tuple(x.shape)}")
            return self.out(self._packed(
                qkv, cu_seqlens, s if max_seqlen is None else max_seqlen, hip,
                p, rng, site))
        if hip and s <= 256 and attn_mask is None:
            # fused QKᵀ→softmax→PV kernel (one launch per step instead of
            # the batched-matmul + softmax chain); emits ctx in [b, s, h]
            # directly — no transpose/reshape passes
            return self.out(Fx.attention(qkv, self.heads, self.scale, None,
                                         p, rng, site))
        if (hip and (attn_mask is None or attn_mask.shape == (b, 1, 1, s))
                and _os.environ.get("MPIAMD_FLASH_ATTN",
                                    _FLASH_ATTN_DEFAULT) != "0"):
            # tiled online-softmax kernels: s > 256 and/or the additive key
            # mask BertModel builds; saves a per-row log-sum-exp instead of
            # [b, nh, s, s] probs. Other mask shapes keep the eager chain.
            return self.out(Fx.flash_attention(
                qkv, self.heads, self.scale,
                attn_mask.reshape(b, s) if attn_mask is not None else None,
                p, rng, site))
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))  # b, nh, s, hd
        scores = torch.matmul(q, k.transpose(-1, -2)) * self.scale
        if attn_mask is not None:
            scores = scores + attn_mask
        probs = torch.softmax(scores.float(), dim=-1).to(v.dtype)
        if p > 0:
            probs = F.dropout(probs, p, training=True)
        ctx = torch.matmul(probs, v)  # b, nh, s, hd
        ctx = ctx.transpose(1, 2).reshape(b, s, h)
        return self.out(ctx)


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.attn = SelfAttention(cfg)
        self.ln1 = LayerNorm(cfg.hidden, eps=cfg.eps)
        self.fc1 = BertLinear(cfg.hidden, cfg.intermediate)
        self.fc2 = BertLinear(cfg.intermediate, cfg.hidden)
        self.ln2 = LayerNorm(cfg.hidden, eps=cfg.eps)

    def _join_ln(self, ln, a, b, p=0.0, rng=None, site=0):
        """residual + LN; fused single-pass kernel when enabled. p > 0 drops
        out the branch b first: inside the join kernel on the fused path."""
        if p > 0:
            if (_FUSED_LN and rng is not None and a.is_cuda
                    and a.dtype == torch.bfloat16):
                return Fx.layer_norm_drop_add(a, b, ln.weight.float(),
                                              ln.bias.float(), ln.eps, p, rng,
                                              site)
            b = _dropout(b, p, rng, site)
        if _FUSED_LN and a.is_cuda and a.dtype == torch.bfloat16:
            return Fx.layer_norm_add(a, b, ln.weight.float(), ln.bias.float(),
                                     ln.eps)
        return ln(a + b)

    def forward(self, x, attn_mask=None, p=0.0, rng=None, site=0,
                attn_p=0.0, attn_site=0, *, cu_seqlens=None, max_seqlen=None):
        """p, rng, site: BertModel's hidden-state dropout for this call
        (p = 0 outside training); the attention-output join draws at `site`,
        the FFN-output join at `site + 1`. attn_p, attn_site: dropout on the
        attention probabilities, drawn from the same rng at `attn_site`.
        cu_seqlens, max_seqlen: x is a packed batch (SelfAttention.forward);
        everything but attention is token-major and takes it as it is."""
        if (x.is_cuda and x.dtype == torch.bfloat16 and attn_mask is None
                and cu_seqlens is None
                and self.attn.head_dim == 64 and x.shape[1] == 128 and p == 0
                and attn_p == 0
                and _os.environ.get("MPIAMD_LAYER_FUSED", "0") == "1"):
            # whole-layer composite Function (Fx.BertLayerFn): residual-join
            # backward adds fold into accumulate-dgrad GEMM epilogues.
            # Measured same-box 1400 vs 1461 seq/s AGAINST the per-op path
            # at BERT-Large bs32 — the unsplit acc-dgrad GEMM (no split-K,
            # extra C read in the epilogue) costs more than the two
            # CUDAFunctor_add joins it removes. Default OFF.
            b, s, h = x.shape
            y = Fx.bert_layer(
                x.reshape(-1, h).contiguous(), b, s, self.attn.heads,
                self.attn.scale, self.ln1.eps,
                self.attn.qkv.weight, self.attn.qkv.bias,
                self.attn.out.weight, self.attn.out.bias,
                self.ln1.weight.float(), self.ln1.bias.float(),
                self.fc1.weight, self.fc1.bias,
                self.fc2.weight, self.fc2.bias,
                self.ln2.weight.float(), self.ln2.bias.float())
            return y.view(b, s, h)
        # a padded batch calls the attention exactly as before
        pk = {} if cu_seqlens is None else {"cu_seqlens": cu_seqlens,
                                            "max_seqlen": max_seqlen}
        x = self._join_ln(
            self.ln1, x, self.attn(x, attn_mask, attn_p, rng, attn_site, **pk),
            p, rng, site)
        if x.is_cuda and x.dtype == torch.bfloat16:
            # fused FFN: GELU lives in the GEMM epilogues (fwd emits
            # h_pre + gelu(h); bwd's fc2-dx multiplies by gelu'(h_pre))
            b, s, h = x.shape
            y = Fx.ffn(x.reshape(-1, h).contiguous(),
                       self.fc1.weight, self.fc1.bias,
                       self.fc2.weight, self.fc2.bias).view(b, s, h)
        else:
            y = self.fc2(F.gelu(self.fc1(x), approximate="tanh"))
        return self._join_ln(self.ln2, x, y, p, rng, site + 1)


class BertEmbeddings(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.tok = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.pos = nn.Embedding(cfg.max_seq, cfg.hidden)
        self.typ = nn.Embedding(cfg.type_vocab, cfg.hidden)
        self.ln = LayerNorm(cfg.hidden, eps=cfg.eps)
        for e in (self.tok, self.pos, self.typ):
            nn.init.normal_(e.weight, std=0.02)

    def forward(self, ids, type_ids=None, p=0.0, rng=None, site=0, *,
                position_ids=None):
        """position_ids (ids' shape): each token's position, for a packed
        batch whose tokens count from 0 within their own sequence; default
        0..s−1 along dim 1."""
        s = ids.shape[1]
        if position_ids is None:
            pos = self.pos(torch.arange(s, device=ids.device))[None]
        else:
            pos = self.pos(position_ids)
        x = self.tok(ids) + pos
        if type_ids is not None:
            x = x + self.typ(type_ids)
        x = self.ln(x)
        return _dropout(x, p, rng, site) if p > 0 else x


class BertModel(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.cfg = cfg
        self.embeddings = BertEmbeddings(cfg)
        self.layers = nn.ModuleList(BertLayer(cfg) for _ in range(cfg.layers))
        # Device random-number state of the dropout kernels. A plain
        # attribute, NOT a buffer: broadcast_parameters would hand every rank
        # rank 0's seed, and a persistent buffer would change state_dict.
        self._dropout_rng = None
        self._dropout_seed = None

    def seed_dropout(self, seed: int):
        """(Re-)seed the dropout masks and restart their step counter; give
        each data-parallel rank its own seed. Without it the state is created
        on the first eager training forward from torch.initial_seed(). On
        the CPU (or in another dtype than bf16) dropout draws from torch's
        generator, which this leaves alone; the seed is kept for the GPU."""
        self._dropout_seed = int(seed)
        dev = self.embeddings.tok.weight.device
        rng = self._dropout_rng
        if rng is not None and rng.state.device == dev:
            rng.set_state(seed, 0)
        elif dev.type == "cuda":
            self._dropout_rng = Fx.DropoutRng(seed, dev)
        else:
            self._dropout_rng = None  # created once the model is on a GPU

    def _rng(self, device):
        rng = self._dropout_rng
        if rng is None or rng.state.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(
                    "BertModel: the first training forward with dropout allocates "
                    "the random-number state and must not run under graph "
                    "capture; run one eager step first")
            seed = self._dropout_seed
            rng = Fx.DropoutRng(torch.initial_seed() if seed is None else seed,
                                device)
            self._dropout_rng = rng
        return rng

    def forward(self, ids, type_ids=None, attn_mask=None, *, cu_seqlens=None,
                max_seqlen=None, position_ids=None):
        """cu_seqlens (int32 [N + 1] on ids' device): ids is a packed batch
        [1, T] of N sequence slots back to back (pack_padded_batch) instead
        of a padded [b, s] one; no attn_mask then. max_seqlen (host int,
        default cfg.max_seq) bounds the sequence lengths, and position_ids
        [1, T] gives each token its position within its own sequence. T, N
        and max_seqlen fix every shape; the lengths live in cu_seqlens'
        contents, so a captured step replays on another mix."""
        pk = {}
        if cu_seqlens is not None:
            if attn_mask is not None:
                raise ValueError("a packed batch (cu_seqlens) takes no "
                                 "attn_mask")
            if ids.dim() != 2 or ids.shape[0] != 1:
                raise ValueError(f"packed ids must be [1, T], got "
                                 f"{tuple(ids.shape)}")
            if max_seqlen is None:
                max_seqlen = self.cfg.max_seq
            if not 1 <= max_seqlen <= self.cfg.max_seq:
                raise ValueError(f"max_seqlen must be in [1, max_seq="
                                 f"{self.cfg.max_seq}], got {max_seqlen}")
            pk = {"cu_seqlens": cu_seqlens, "max_seqlen": int(max_seqlen)}
        if attn_mask is not None and attn_mask.dim() == 2:
            # (b, s) 1/0 mask → additive (b, 1, 1, s)
            attn_mask = (1.0 - attn_mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
        p = self.cfg.dropout if self.training else 0.0
        pa = self.cfg.attn_dropout if self.training else 0.0
        if not (p > 0 or pa > 0):
            x = self.embeddings(ids, type_ids, position_ids=position_ids)
            for layer in self.layers:
                x = layer(x, attn_mask, **pk)
            return x
        # static call sites: embeddings 0, layer i attention-output join
        # 1 + 2i, FFN-output join 2 + 2i, attention probabilities
        # 1 + 2·layers + i; one tick per forward separates steps
        rng = None
        w = self.embeddings.tok.weight
        if w.is_cuda and w.dtype == torch.bfloat16:
            rng = self._rng(w.device)
            rng.tick()
        n = len(self.layers)
        x = self.embeddings(ids, type_ids, p, rng, 0,
                            position_ids=position_ids)
        for i, layer in enumerate(self.layers):
            x = layer(x, attn_mask, p, rng, 1 + 2 * i, pa, 1 + 2 * n + i,
                      **pk)
        return x


class BertForPreTraining(nn.Module):
    """MLM + NSP heads, the standard pretraining objective."""

    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.cfg = cfg
        self.bert = BertModel(cfg)
        self.mlm_transform = BertLinear(cfg.hidden, cfg.hidden)
        self.mlm_ln = LayerNorm(cfg.hidden, eps=cfg.eps)
        # decoder tied to token embeddings (standard BERT weight tying)
        self.mlm_bias = nn.Parameter(torch.zeros(cfg.vocab_size))
        self.nsp = BertLinear(cfg.hidden, 2)

    def seed_dropout(self, seed: int):
        """BertModel.seed_dropout of the trunk."""
        self.bert.seed_dropout(seed)

    def _first_tokens(self, x, cu_seqlens):
        """The first token of every sequence (what NSP reads): x[:, 0] of a
        padded batch; row cu_seqlens[n] of a packed one. An empty slot reads
        a neighbour's row (clamped into the buffer) and carries nsp label
        −100, which the NSP loss ignores."""
        if cu_seqlens is None:
            return x[:, 0]
        return x[0, cu_seqlens[:-1].long().clamp(max=x.shape[1] - 1)]

    def forward(self, ids, type_ids=None, attn_mask=None, mlm_labels=None,
                nsp_labels=None, *, cu_seqlens=None, max_seqlen=None,
                position_ids=None):
        """cu_seqlens, max_seqlen, position_ids: a packed batch, as in
        BertModel.forward. mlm_labels is then [1, T] with −100 at the unused
        tail, nsp_labels / nsp_logits have one entry per sequence slot, and
        an empty slot's nsp label is −100."""
        x = self.bert(ids, type_ids, attn_mask, cu_seqlens=cu_seqlens,
                      max_seqlen=max_seqlen, position_ids=position_ids)
        h = self.mlm_ln(F.gelu(self.mlm_transform(x), approximate="tanh"))
        tok_w = self.bert.embeddings.tok.weight
        if mlm_labels is not None:
            # labels-in-forward (HF-style) training path: the fused MLM head
            # never materializes the unpadded [b·s, V] logits — decoder GEMM,
            # masked CE and its backward all work on one padded-vocab buffer
            if h.is_cuda and h.dtype == torch.bfloat16:
                b, s, hd = h.shape
                l_mlm = Fx.mlm_head_loss(h.reshape(-1, hd).contiguous(),
                                         tok_w, self.mlm_bias.float(),
                                         mlm_labels.view(-1))
            else:
                logits = torch.matmul(h, tok_w.t().to(h.dtype)) \
                    + self.mlm_bias.to(h.dtype)
                l_mlm = F.cross_entropy(
                    logits.float().view(-1, self.cfg.vocab_size),
                    mlm_labels.view(-1), ignore_index=-100)
            loss = l_mlm
            if nsp_labels is not None:
                nsp_logits = self.nsp(self._first_tokens(x, cu_seqlens))
                loss = loss + F.cross_entropy(nsp_logits.float(), nsp_labels,
                                              ignore_index=-100)
            return loss
        if h.is_cuda and h.dtype == torch.bfloat16:
            # decoder GEMM on the in-tree NT kernel with the bias folded
            # into the epilogue (weight tying: grads flow to tok.weight)
            b, s, hd = h.shape
            mlm_logits = Fx.linear(h.reshape(-1, hd).contiguous(), tok_w,
                                   self.mlm_bias).view(b, s, -1)
        else:
            mlm_logits = torch.matmul(h, tok_w.t().to(h.dtype)) + self.mlm_bias.to(h.dtype)
        nsp_logits = self.nsp(self._first_tokens(x, cu_seqlens))
        return mlm_logits, nsp_logits

    def loss(self, mlm_logits, nsp_logits, mlm_labels, nsp_labels):
        """mlm_labels: (b, s) with -100 at unmasked positions."""
        if mlm_logits.is_cuda and mlm_logits.dtype == torch.bfloat16:
            # fused masked CE: no fp32 logits cast, no fp32 probs — the
            # torch path moves ~1.5 GB extra HBM at bs32·seq128·vocab30k
            l_mlm = Fx.masked_softmax_cross_entropy(
                mlm_logits.view(-1, self.cfg.vocab_size), mlm_labels.view(-1))
        else:
            l_mlm = F.cross_entropy(
                mlm_logits.float().view(-1, self.cfg.vocab_size),
                mlm_labels.view(-1), ignore_index=-100)
        l_nsp = F.cross_entropy(nsp_logits.float(), nsp_labels)
        return l_mlm + l_nsp


class PackedBatch(NamedTuple):
    """pack_padded_batch's result; the fields are BertForPreTraining.forward's
    arguments of the same names."""
    ids: torch.Tensor                      # [1, T]
    type_ids: Optional[torch.Tensor]       # [1, T] or None
    position_ids: torch.Tensor             # [1, T]
    mlm_labels: Optional[torch.Tensor]     # [1, T] or None
    cu_seqlens: torch.Tensor               # int32 [max_sequences + 1]
    max_seqlen: int


def pack_padded_batch(ids, type_ids, attn_mask, mlm_labels, token_budget=None,
                      max_sequences=None, *, max_seq=None) -> PackedBatch:
    """Drop the padding of a [b, s] batch: its valid tokens (attn_mask 1/0,
    each row's valid tokens a prefix) back to back in one [1, T] row.

    T = token_budget (default: the number of valid tokens); the unused tail
    gets id 0, type 0, position 0 and label −100. cu_seqlens has
    max_sequences + 1 entries (default b + 1), the slots past b empty, so
    that batches of a data pipeline share one shape whatever their lengths.
    position_ids count from 0 within each sequence; max_seqlen is the
    longest length in this batch. type_ids and mlm_labels may be None.
    Raises ValueError if the tokens exceed token_budget, the sequences
    max_sequences, or a length max_seq (pass the model's cfg.max_seq).
    A host-side data-pipeline helper: it reads the mask on the host."""
    b, s = ids.shape
    valid = attn_mask.to(torch.bool)
    lens = valid.sum(dim=1)
    if not torch.equal(valid, torch.arange(s, device=ids.device)[None]
                       < lens[:, None]):
        raise ValueError("attn_mask must mark a prefix of each row as valid")
    lens_l = [int(n) for n in lens.tolist()]
    total = sum(lens_l)
    budget = total if token_budget is None else int(token_budget)
    slots = b if max_sequences is None else int(max_sequences)
    if total > budget:
        raise ValueError(f"{total} valid tokens do not fit token_budget="
                         f"{budget}")
    if b > slots:
        raise ValueError(f"{b} sequences do not fit max_sequences={slots}")
    if budget < 1:
        raise ValueError("token_budget must be at least 1")
    longest = max(lens_l)
    if max_seq is not None and longest > max_seq:
        raise ValueError(f"a sequence of {longest} tokens exceeds max_seq="
                         f"{max_seq}")

    def pack(t, fill):
        if t is None:
            return None
        out = t.new_full((1, budget), fill)
        out[0, :total] = t[valid]
        return out

    pos = torch.arange(s, device=ids.device)[None].expand(b, s)
    cu = [0]
    for n in lens_l:
        cu.append(cu[-1] + n)
    cu += [total] * (slots - b)
    return PackedBatch(
        pack(ids, 0), pack(type_ids, 0), pack(pos, 0), pack(mlm_labels, -100),
        torch.tensor(cu, dtype=torch.int32, device=ids.device),
        max(longest, 1))


def bert_param_groups(model: nn.Module, weight_decay: float = 0.01):
    """Optimizer param groups with the usual BERT exemption: no weight decay
    on biases and LayerNorm parameters."""
    no_decay = {id(p) for mod in model.modules() if isinstance(mod, LayerNorm)
                for p in mod.parameters(recurse=False)}
    decay, exempt = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if id(p) in no_decay or name.endswith("bias"):
            exempt.append(p)
        else:
            decay.append(p)
    return [{"params": decay, "weight_decay": weight_decay},
            {"params": exempt, "weight_decay": 0.0}]


def to_mi355x_bert(model: BertForPreTraining, device) -> BertForPreTraining:
    """bf16 working weights on the GPU, with LayerNorm params and linear
    biases kept fp32: the HIP kernels consume them as fp32 operands anyway
    (epilogue bias add, LN affine), so fp32 residency removes ~200 per-step
    dtype-cast kernels (.float() on entry + grad .to(bf16) on exit —
    ~2.6 ms/step on BERT-Large bs32, prof8 trace)."""
    model = model.to(device=device, dtype=torch.bfloat16)
    for mod in model.modules():
        if isinstance(mod, LayerNorm):
            mod.weight.data = mod.weight.data.float()
            mod.bias.data = mod.bias.data.float()
        elif isinstance(mod, BertLinear):
            mod.bias.data = mod.bias.data.float()
    model.mlm_bias.data = model.mlm_bias.data.float()
    return model
