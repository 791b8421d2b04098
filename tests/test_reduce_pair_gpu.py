"""The paired split-K reduces after a conv backward pair (set_pair_reduce):
the dx reduce (with the consumer BN's backward statistics for
conv2d_dgrad_bn_wgrad, plain for conv2d_dgrad_wgrad) and the dw reduce run as
one grid. Every workgroup of that grid does what a workgroup of the separate
launch does, so dx, the slab and dw must be bit for bit what the two launches
give, in either workgroup order; every comparison here is torch.equal.

pair_reduce_count() counts the pair-reduce launches of this process. Each
case asserts that it rose by exactly 1 with the switch on and by 0 with it
off, so a shape that silently takes the two launches fails its test.

The pair kernel exists for the (dx splits, dw splits) combinations of
ResNet50/101 at batch 64: (2, 8), (2, runtime form), (4, 6), (5, 3), where
the runtime form of the dw reduce serves every count outside 2, 3, 4, 5, 6,
8, 16 (1 included). Shapes, (N, C, H, W, Kout, R, pad), are the smallest that
give those counts under conv_splits / conv_wgrad_splits:

  1x1-c64-s2-rt    2x64x7x7 -> 1024     dx 2, dw 1 (runtime form); C8 = 8, a
                   block owns 32 rows, M = 98 leaves the second row of the
                   two-row loop (r2 >= M) out; ReLU bitmask
  3x3-c64-s2-rt    2x64x7x7 -> 128 3x3  dx 2, dw 1; relu=False
  1x1-c64-s2-w8    1x64x64x64 -> 1024   dx 2, dw 8 (the wgrad needs M >= 4096
                   for 8 splits); 128 blocks, r2 >= M for every row; ReLU from
                   the BN output (no bitmask)
  1x1-c512-s4-w6   64x512x7x7 -> 2048   dx 4, dw 6: the wgrad splits 6 ways
                   only from M >= 3072, so this is the ResNet shape itself;
                   C8 = 64, 512 blocks, M = 3136 no multiple of 4096
  3x3-c512-s5-w3   64x512x7x7 -> 512 3x3  dx 5, dw 3; ResNet's, for the same
                   reason
  3x3-c512-s4-rt   2x512x7x7 -> 256 3x3  dx 4, dw 1: outside the table, the
                   two launches
"""
import functools

import pytest
import torch

import conv_refs as cr

gpu = pytest.mark.gpu
DEV = "cuda"
EPS, MOM = 1e-5, 0.1

# id -> ((N, C, H, W, Kout, R, pad), dx splits, dw splits, relu, bitmask)
CASES = {
    "1x1-c64-s2-rt": ((2, 64, 7, 7, 1024, 1, 0), 2, 1, True, True),
    "3x3-c64-s2-rt": ((2, 64, 7, 7, 128, 3, 1), 2, 1, False, False),
    "1x1-c64-s2-w8": ((1, 64, 64, 64, 1024, 1, 0), 2, 8, True, False),
    "1x1-c512-s4-w6": ((64, 512, 7, 7, 2048, 1, 0), 4, 6, True, True),
    "3x3-c512-s5-w3": ((64, 512, 7, 7, 512, 3, 1), 5, 3, True, True),
}
FALLBACK = ("3x3-c512-s4-rt", ((2, 512, 7, 7, 256, 3, 1), 4, 1, True, True))
PLAIN = ("1x1-c64-s2-rt", "1x1-c64-s2-w8", "3x3-c512-s5-w3")
ALL = dict(CASES, **{FALLBACK[0]: FALLBACK[1]})

# (on, stats_first) of set_pair_reduce
MODES = {"dw-first": (True, False), "dx-first": (True, True)}


@functools.lru_cache(maxsize=None)
def ext():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def restore(prev):
    """prev: the mode (0, 1 or 2) a set_pair_reduce call returned."""
    ext().set_pair_reduce(prev != 0, prev == 2)


class pair_reduce:
    def __init__(self, on, stats_first=False):
        self.mode = (on, stats_first)

    def __enter__(self):
        self.prev = ext().set_pair_reduce(*self.mode)

    def __exit__(self, *exc):
        restore(self.prev)


def default_heuristics():
    info = ext().route_info()
    return (info["conv_splits_force"] < 1 and info["wgrad_budget"] == 512
            and info["pipe8"] and info["pipemix"] and info["pipegather"]
            and info["pipegather_wgrad"])


def need_defaults():
    """The counter assertions hold where the conv pair runs (the 8-wave
    routes) at the heuristics' own split counts; a process whose MPIAMD_*
    knobs say otherwise does not assert them."""
    if not default_heuristics():
        pytest.skip("split counts or GEMM routes forced by MPIAMD_* knobs")
    prev = ext().set_pair_bwd(True)
    ext().set_pair_bwd(prev != 0, prev == 2)
    if prev == 0:
        pytest.skip("MPIAMD_PAIR_BWD=0: no conv pair, so no reduce pair")


def bn_call(c, relu, bitmask):
    (N, C, H, W, K, R, pad) = c["geom"]
    e = torch.empty(0)
    return ext().conv2d_dgrad_bn_wgrad(
        c["dy"], c["w"], c["x"], H, W, R, R, pad, c["a"],
        e if bitmask or not relu else c["by"], c["mean"], c["invstd"], relu,
        c["mask"] if bitmask and relu else e)


def plain_call(c):
    (N, C, H, W, K, R, pad) = c["geom"]
    return ext().conv2d_dgrad_wgrad(c["dy"], c["w"], c["x"], H, W, R, R, pad)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of one geometry and, with the pair reduce off, the results of
    both bindings and the counter's step; made once, never modified."""
    geom, ds, ws, relu, bitmask = ALL[name]
    N, C, H, W, K, R, pad = geom
    HO, WO = H + 2 * pad - R + 1, W + 2 * pad - R + 1
    x = cr.rand_bf16((N, C, H, W), 50, device=DEV)
    w = cr.rand_bf16((K, C, R, R), 51, scale=0.5, device=DEV)
    dy = cr.rand_bf16((N, K, HO, WO), 52, device=DEV)
    # the BN(+ReLU) layer that produced x and consumes dx as its dy
    a = cr.rand_bf16((N, C, H, W), 53, scale=3.0, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(54)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    by, mean, invstd, mask = ext().bn_fwd_train(
        a, gamma, beta, EPS, True, torch.zeros(C, device=DEV),
        torch.ones(C, device=DEV), MOM, torch.empty(0))
    c = dict(geom=geom, x=x, w=w, dy=dy, a=a, by=by, mean=mean,
             invstd=invstd, mask=mask)
    with pair_reduce(False):
        n0 = ext().pair_reduce_count()
        c["dx"], c["slab"], c["dw"] = bn_call(c, relu, bitmask)
        c["pdx"], c["pdw"] = plain_call(c)
        c["off_step"] = ext().pair_reduce_count() - n0
    torch.cuda.synchronize()
    return c


def poison_outputs(c):
    N, C, H, W, K, R, pad = c["geom"]
    cr.poison((N, C, H, W), c["x"])
    cr.poison((K, C, R, R), c["w"])
    cr.poison(tuple(c["slab"].shape), c["slab"])


@gpu
def test_shapes_reach_their_split_counts():
    """The split counts the table above claims (heuristics at their defaults)
    and the row geometry of the two small-channel cases."""
    if not default_heuristics():
        pytest.skip("split counts or GEMM routes forced by MPIAMD_* knobs")
    e = ext()
    for name, (geom, ds, ws, relu, bitmask) in ALL.items():
        N, C, H, W, K, R, pad = geom
        M = N * H * W
        assert e.conv_splits(M, C, R * R * K) == ds, name
        assert e.conv_wgrad_splits(K, R * R * C, M) == ws, name
        grid, rpb = case(name)["slab"].shape[0], 256 // (C // 8)
        assert M % (2 * grid * rpb) != 0, name  # the odd tail row is hit
    assert {ds for _, ds, *_ in CASES.values()} == {2, 4, 5}
    assert CASES["1x1-c64-s2-rt"][0][1] // 8 == 8
    assert CASES["1x1-c512-s4-w6"][0][1] // 8 >= 64


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_bn_pair_equals_two_launches(name, mode):
    need_defaults()
    geom, ds, ws, relu, bitmask = CASES[name]
    c = case(name)
    assert c["slab"].numel() > 0
    assert c["off_step"] == 0
    with pair_reduce(*MODES[mode]):
        poison_outputs(c)
        n0 = ext().pair_reduce_count()
        dx, slab, dw = bn_call(c, relu, bitmask)
        assert ext().pair_reduce_count() - n0 == 1
    assert slab.numel() > 0 and slab.shape == c["slab"].shape
    assert torch.equal(dx, c["dx"]), "dx"
    assert torch.equal(slab, c["slab"]), "slab"
    assert torch.equal(dw, c["dw"]), "dw"
    assert dw.is_contiguous(memory_format=torch.channels_last)


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", PLAIN)
def test_plain_pair_equals_two_launches(name, mode):
    """conv2d_dgrad_wgrad at a shape whose dgrad splits: the dx side is the
    plain split-K reduce."""
    need_defaults()
    c = case(name)
    assert c["off_step"] == 0
    with pair_reduce(*MODES[mode]):
        poison_outputs(c)
        n0 = ext().pair_reduce_count()
        dx, dw = plain_call(c)
        assert ext().pair_reduce_count() - n0 == 1
    assert torch.equal(dx, c["pdx"]), "dx"
    assert torch.equal(dw, c["pdw"]), "dw"
    # the reduce+stats kernel rounds the same sums once, as this one does
    assert torch.equal(dx, c["dx"])


@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_combination_outside_the_table_takes_two_launches(mode):
    name, (geom, ds, ws, relu, bitmask) = FALLBACK
    need_defaults()
    c = case(name)
    assert c["slab"].numel() > 0
    with pair_reduce(*MODES[mode]):
        n0 = ext().pair_reduce_count()
        dx, slab, dw = bn_call(c, relu, bitmask)
        pdx, pdw = plain_call(c)
        assert ext().pair_reduce_count() == n0
    assert torch.equal(dx, c["dx"]) and torch.equal(slab, c["slab"])
    assert torch.equal(dw, c["dw"])
    assert torch.equal(pdx, c["pdx"]) and torch.equal(pdw, c["pdw"])


@gpu
def test_set_pair_reduce_returns_previous():
    e = ext()
    prev = e.set_pair_reduce(False)
    try:
        assert prev in (0, 1, 2)
        assert e.set_pair_reduce(True) == 0
        assert e.set_pair_reduce(True, True) == 1
        assert e.set_pair_reduce(False, True) == 2  # off: the order is dropped
        assert e.set_pair_reduce(False) == 0
    finally:
        restore(prev)
    assert e.set_pair_reduce(prev != 0, prev == 2) == prev


@gpu
def test_paired_case_against_fp64():
    """dx and dw of one paired case per element against conv_refs' fp64
    references: one bf16 rounding plus the fp32 sum of n products in any
    order (conv_refs' bound, no wider than the 2^-23 of
    test_conv_pair_gpu.py)."""
    need_defaults()
    name = "3x3-c64-s2-rt"
    geom, ds, ws, relu, bitmask = CASES[name]
    N, C, H, W, K, R, pad = geom
    g9 = (N, C, H, W, K, R, R, 1, pad)
    c = case(name)
    with pair_reduce(True):
        n0 = ext().pair_reduce_count()
        dx, slab, dw = bn_call(c, relu, bitmask)
        assert ext().pair_reduce_count() - n0 == 1
    ref, bound = cr.dgrad_ref(c["dy"], c["w"], g9)
    cr.assert_close(dx, ref, cr.REL_BF16, bound, f"pair_reduce_dx[{name}]")
    ref, bound = cr.wgrad_ref(c["x"], c["dy"], g9)
    cr.assert_close(dw, ref, cr.REL_BF16, bound, f"pair_reduce_dw[{name}]")
