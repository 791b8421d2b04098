"""Time the BN statistics bindings with the pipelined producers and the
coalesced finalize switched old/new in one process.

Each figure is the mean over `--iters` back-to-back launches (events around
the whole burst); all `--rounds` rounds are printed, old and new alternating
inside a round, as `tools/pipe_bench --epi` does. The burst is captured into
one graph and replayed, so the figure is GPU time: launched from Python, a
binding of two 5 us kernels is bound by the host at ~11 us a call and every
finalize looks the same.

  python tools/bn_bench.py                 # producers at ResNet101's classes
  python tools/bn_bench.py --finalize      # finalize alone, every slice width

The pipeline depth is a compile-time constant (MPIAMD_BN_PIPE_DEPTH in
batchnorm.hip): compare depths by running this against builds that differ in
it. The producers' figures include the finalize and apply passes of the
binding, which are the same kernels on both sides of a comparison.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS, MOM = 1e-5, 0.1
# ResNet101 at batch 64: rows x channels of the BN layers, per stage
CLASSES = [(200704, 64), (200704, 256), (50176, 128), (50176, 512),
           (12544, 256), (12544, 1024), (3136, 512), (3136, 2048)]


def rand_cl(M, C, seed, scale=1.0):
    torch.manual_seed(seed)
    t = ((torch.rand(1, C, M, 1, device="cuda") * 2 - 1) * scale)
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def burst_us(fn, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture stream
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    g.replay()
    t1.record()
    torch.cuda.synchronize()
    del g
    return t0.elapsed_time(t1) * 1e3 / iters


def ab(label, settings, apply, fn, iters, rounds):
    """settings: list of (name, value); apply(value) selects one."""
    cols = {name: [] for name, _ in settings}
    for _ in range(rounds):
        for name, value in settings:
            apply(value)
            cols[name].append(burst_us(fn, iters))
    line = f"{label:34s}"
    for name, _ in settings:
        v = cols[name]
        line += f"  {name} " + "/".join(f"{x:6.1f}" for x in v)
    base = sum(cols[settings[0][0]]) / rounds
    for name, _ in settings[1:]:
        line += f"  {name}/{settings[0][0]} {sum(cols[name]) / rounds / base:5.3f}"
    print(line, flush=True)


def producers(ext, iters, rounds):
    e = torch.empty(0)
    onoff = [("old", False), ("new", True)]
    for M, C in CLASSES:
        a, b = rand_cl(M, C, 1), rand_cl(M, C, 2)
        x, xd = rand_cl(M, C, 3, 3.0), rand_cl(M, C, 4, 3.0)
        torch.manual_seed(5)
        gamma = torch.rand(C, device="cuda") + 0.5
        beta = torch.randn(C, device="cuda") * 0.2
        jmask = torch.randint(0, 256, (M, C // 8), device="cuda",
                              dtype=torch.uint8)
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        y, mean, invstd, mask = ext.bn_fwd_train(x, gamma, beta, EPS, True, rm,
                                                 rv, MOM, e)
        _, mean_d, invstd_d, _ = ext.bn_fwd_train(xd, gamma, beta, EPS, False,
                                                  rm, rv, MOM, e)
        cases = [
            ("bn_fwd_train", lambda: ext.bn_fwd_train(
                x, gamma, beta, EPS, True, rm, rv, MOM, e)),
            ("bn_bwd mask", lambda: ext.bn_bwd(
                a, x, y, gamma, mean, invstd, True, mask)),
            ("bn_bwd norelu", lambda: ext.bn_bwd(
                a, x, y, gamma, mean, invstd, False, e)),
            ("join<1,1>", lambda: ext.join_bwd_stats(
                a, jmask, b, x, mean, invstd, mask, e, e, e)),
            ("join<0,1>", lambda: ext.join_bwd_stats(
                a, e, b, x, mean, invstd, mask, e, e, e)),
            ("join<1,2>", lambda: ext.join_bwd_stats(
                a, jmask, b, x, mean, invstd, mask, xd, mean_d, invstd_d)),
            ("join<0,2>", lambda: ext.join_bwd_stats(
                a, e, b, x, mean, invstd, mask, xd, mean_d, invstd_d)),
        ]
        for name, fn in cases:
            ab(f"{M}x{C} {name}", onoff, ext.set_bn_pipelined, fn, iters,
               rounds)
        del a, b, x, xd, jmask, y, mask
        torch.cuda.empty_cache()


def finalize(ext, iters, rounds):
    """bn_fwd_train_pre + bn_bwd_pre on a 64-row activation (the apply passes
    are a few hundred bytes), slabs of the partials grid (512 rows) and of the
    conv-epilogue bands (3136 rows)."""
    e = torch.empty(0)
    widths = [("bands", -1), ("ch8", 8), ("ch16", 16)]
    for C in sorted({c for _, c in CLASSES}):
        x, dy = rand_cl(64, C, 1, 3.0), rand_cl(64, C, 2)
        torch.manual_seed(5)
        gamma = torch.rand(C, device="cuda") + 0.5
        beta = torch.randn(C, device="cuda") * 0.2
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        y, mean, invstd, mask = ext.bn_fwd_train(x, gamma, beta, EPS, True, rm,
                                                 rv, MOM, e)
        for rows in (512, 3136):
            slab = torch.randn(rows, 2, C, device="cuda")
            slab[:, 1] = slab[:, 1].abs() + 1.0
            ab(f"C={C} rows={rows} fwd_pre", widths, ext.set_bn_finalize_ch,
               lambda: ext.bn_fwd_train_pre(x, slab, gamma, beta, EPS, True,
                                            rm, rv, MOM, e), iters, rounds)
            ab(f"C={C} rows={rows} bwd_pre", widths, ext.set_bn_finalize_ch,
               lambda: ext.bn_bwd_pre(dy, slab, x, y, gamma, mean, invstd,
                                      True, mask), iters, rounds)
    ext.set_bn_finalize_ch(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--finalize", action="store_true")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from mpi_operator_amd.ops import hip_ext
    ext = hip_ext()
    prev = ext.set_bn_pipelined(True), ext.set_bn_finalize_coalesced(True)
    try:
        if args.finalize:
            finalize(ext, args.iters, args.rounds)
        else:
            producers(ext, args.iters, args.rounds)
    finally:
        ext.set_bn_pipelined(prev[0])
        ext.set_bn_finalize_coalesced(prev[1])


if __name__ == "__main__":
    main()
