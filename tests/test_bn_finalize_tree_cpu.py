"""The BN finalize's summation tree, modelled in numpy fp32 in the two
associations the kernels use, without a GPU:

  bands     (bn_finalize_*_bands_k): thread t of 256 sums slab rows g = t,
            t + 256, ... in ascending order; each wave of 64 consecutive t
            runs the xor butterfly (offsets 32, 16, 8, 4, 2, 1); the four
            wave results are added as ((r0 + r1) + r2) + r3.
  coalesced (bn_finalize_*_co_k<CH>): thread (ch, rg) holds the chains
            t = rg + k·RG, RG = 256 / CH; the butterfly levels >= RG pair
            registers of one thread, the levels < RG pair row groups.

Both must give the same bits for every channel, and stay within 1e-5 relative
of the fp64 sum."""
import numpy as np
import pytest

ROWS = [1, 2, 255, 256, 257, 512, 513, 3136]
f32 = np.float32


def chains(p):
    """[256, C] fp32: chain t = p[t] + p[t + 256] + ... from 0, ascending."""
    rows, C = p.shape
    s = np.zeros((256, C), f32)
    for base in range(0, rows, 256):
        blk = p[base:base + 256]
        s[:blk.shape[0]] = s[:blk.shape[0]] + blk
    return s


def tree_bands(p):
    s = chains(p)
    r = []
    for w in range(4):
        v = s[64 * w:64 * w + 64].copy()
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):  # every lane: v += shfl_xor(v, off)
            v = v + v[lane ^ off]
        r.append(v[0])
    return ((r[0] + r[1]) + r[2]) + r[3]


def tree_coalesced(p, CH):
    RG, KK = 256 // CH, CH // 4
    s = chains(p)
    C = p.shape[1]
    # acc[rg][k] = chain rg + k·RG, as thread (ch, rg) holds them
    acc = np.stack([[s[rg + k * RG] for k in range(CH)] for rg in range(RG)])
    assert acc.shape == (RG, CH, C)
    red = np.zeros((4, RG, C), f32)
    for w in range(4):
        u = [acc[:, w * KK + kk].copy() for kk in range(KK)]
        off = KK // 2
        while off > 0:  # in-register levels 32 .. RG
            for kk in range(off):
                u[kk] = u[kk] + u[kk + off]
            off //= 2
        red[w] = u[0]
    r = []
    for w in range(4):
        v = [red[w, rg].copy() for rg in range(RG)]
        off = RG // 2
        while off > 0:  # the levels below RG, across row groups
            for rg in range(off):
                v[rg] = v[rg] + v[rg + off]
            off //= 2
        r.append(v[0])
    return ((r[0] + r[1]) + r[2]) + r[3]


@pytest.fixture(scope="module")
def slabs():
    rng = np.random.default_rng(0)
    full = rng.standard_normal((max(ROWS), 40)).astype(f32)
    full[:, 20:] = np.abs(full[:, 20:]) + f32(1)  # sums of squares: positive
    return full


@pytest.mark.parametrize("rows", ROWS)
def test_trees_are_bit_equal_and_close_to_fp64(slabs, rows):
    p = slabs[:rows]
    want = tree_bands(p)
    assert want.dtype == f32
    for CH in (8, 16):
        got = tree_coalesced(p, CH)
        assert got.dtype == f32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), CH
    ref = p.astype(np.float64).sum(0)
    err = np.abs(want.astype(np.float64) - ref)
    # the positive columns: 1e-5 relative to the fp64 sum itself
    assert np.all(err[20:] <= 1e-5 * np.abs(ref[20:]))
    # the signed columns can sum to nearly zero; there the bound is relative
    # to Σ|p|, the quantity an fp32 summation error scales with
    assert np.all(err <= 1e-5 * np.abs(p.astype(np.float64)).sum(0))


def test_model_is_sensitive_to_the_tree():
    """A different association (one running sum) gives different bits on the
    same data, so the equality above is not vacuous."""
    rng = np.random.default_rng(1)
    p = rng.standard_normal((3136, 64)).astype(f32)
    serial = np.zeros(64, f32)
    for g in range(p.shape[0]):
        serial = serial + p[g]
    assert not np.array_equal(serial.view(np.uint32),
                              tree_bands(p).view(np.uint32))
