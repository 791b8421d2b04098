"""Row-major 16-byte-store GEMM epilogue (pipe_mix8_k, pipe256x16_gemm_k)
against the one-element-per-lane epilogue of the same kernels.

The vector epilogue only moves data after the last MFMA — every element
keeps its value and its rounding — so each op, run once with
set_epilogue_vec(True) and once with set_epilogue_vec(False) on the same
inputs, must return bit-identical tensors. Accuracy against torch is the
business of the other GPU suites. Shapes are the smallest that reach each
hazard: ragged M, a partial column tile, the fp32 split-K slabs, the
stride-2 scatter writers with and without edge siblings, a caller-owned
output with guard elements, the 256² route, and a shape that must fall back
to the scalar stores."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def rand_cl(*shape, seed=0):
    torch.manual_seed(seed)
    return cl((torch.rand(*shape, device="cuda") * 2 - 1).to(torch.bfloat16))


def rand2d(m, k, seed):
    torch.manual_seed(seed)
    return (torch.rand(m, k, device="cuda") * 2 - 1).to(torch.bfloat16)


def conv_splits(M, ncols, K):
    """The bindings' split-K choice (bindings.cpp conv_splits)."""
    tiles = ((M + 127) // 128) * ((ncols + 127) // 128)
    nk = (K + 63) // 64
    if tiles >= 256 or nk < 16:
        return 1
    return max(1, min(512 // tiles, nk // 8, 16))


@pytest.fixture(scope="module")
def ext():
    from mpi_operator_amd.ops import hip_ext
    return hip_ext()


def both(ext, fn):
    """fn() under the vector and under the scalar epilogue; every output
    tensor must be bit-identical. Returns the vector run's outputs."""
    prev = ext.set_epilogue_vec(True)
    try:
        vec = fn()
        torch.cuda.synchronize()
        ext.set_epilogue_vec(False)
        sca = fn()
        torch.cuda.synchronize()
    finally:
        ext.set_epilogue_vec(prev)
    vec = vec if isinstance(vec, (list, tuple)) else [vec]
    sca = sca if isinstance(sca, (list, tuple)) else [sca]
    assert len(vec) == len(sca)
    for i, (v, s) in enumerate(zip(vec, sca)):
        assert v.shape == s.shape and v.dtype == s.dtype
        assert torch.equal(v, s), (
            i, (v.float() - s.float()).abs().max().item(),
            int((v != s).sum().item()))
    return vec


def test_setter_returns_previous(ext):
    prev = ext.set_epilogue_vec(False)
    try:
        assert ext.set_epilogue_vec(True) is False
        assert ext.set_epilogue_vec(True) is True
    finally:
        ext.set_epilogue_vec(prev)


def test_ragged_m_partial_column_tile(ext):
    # M = 50 rows of one 128-row tile; N = 136: second column tile 8 wide
    x, w = rand_cl(2, 40, 5, 5, seed=1), rand_cl(136, 40, 1, 1, seed=2)
    (y,) = both(ext, lambda: ext.conv2d_fwd(x, w, 1, 0))
    assert y.shape == (2, 136, 5, 5)


def test_gather_3x3_fwd_and_dgrad(ext):
    x, w = rand_cl(2, 16, 9, 9, seed=3), rand_cl(24, 16, 3, 3, seed=4)
    dy = rand_cl(2, 24, 9, 9, seed=5)
    both(ext, lambda: ext.conv2d_fwd(x, w, 1, 1))
    both(ext, lambda: ext.conv2d_dgrad(dy, w, 9, 9, 1, 1))


def test_split_k_fp32_slabs_fwd_and_dgrad(ext):
    # M = 128, K = 1024 (nk = 16), one tile: the heuristic gives 2 splits
    assert conv_splits(128, 64, 1024) == 2
    x, w = rand_cl(2, 1024, 8, 8, seed=6), rand_cl(64, 1024, 1, 1, seed=7)
    both(ext, lambda: ext.conv2d_fwd(x, w, 1, 0))
    # split-K-only fusion: a non-empty slab proves the route did split
    y, slab = both(ext, lambda: ext.conv2d_fwd_bn(x, w, 1, 0, True, False))
    assert slab.numel() > 0
    assert torch.equal(y, ext.conv2d_fwd(x, w, 1, 0))
    dy, wd = rand_cl(2, 1024, 8, 8, seed=8), rand_cl(1024, 64, 1, 1, seed=9)
    both(ext, lambda: ext.conv2d_dgrad(dy, wd, 8, 8, 1, 0))


@pytest.mark.parametrize("R,pad", [(1, 0), (3, 1)])
def test_wgrad_slabs(ext, R, pad):
    # M = 1024 pixels (nk = 16) -> 2 splits; RSC = 144 for the 3x3: the last
    # column tile is 16 wide
    x, dy = rand_cl(4, 16, 16, 16, seed=10), rand_cl(4, 24, 16, 16, seed=11)
    (dw,) = both(ext, lambda: ext.conv2d_wgrad(x, dy, R, R, 1, pad))
    assert dw.shape == (24, 16, R, R)


def test_stride2_writer_odd_input(ext):
    # 3x3 stride-2 dgrad onto 7x7: four parity sub-images of unequal size
    dy, w = rand_cl(2, 16, 4, 4, seed=12), rand_cl(16, 24, 3, 3, seed=13)
    (dx,) = both(ext, lambda: ext.conv2d_dgrad(dy, w, 7, 7, 2, 1))
    assert dx.shape == (2, 24, 7, 7)


@pytest.mark.parametrize("H", [7, 8])
def test_stride2_zero_writer(ext, H):
    # 1x1 stride-2 dgrad: the epilogue zeroes the three sibling pixels; on
    # 7x7 the last row/column has no siblings, on 8x8 every pixel has all
    dy, w = rand_cl(2, 16, 4, 4, seed=14), rand_cl(16, 24, 1, 1, seed=15)
    (dx,) = both(ext, lambda: ext.conv2d_dgrad(dy, w, H, H, 2, 0))
    # siblings are exactly zero, the parity pixels carry the values
    assert float(dx[:, :, 1::2, :].abs().max()) == 0.0
    assert float(dx[:, :, :, 1::2].abs().max()) == 0.0
    assert float(dx[:, :, 0::2, 0::2].abs().max()) > 0.0


@pytest.mark.parametrize("off", [64, 67])
def test_caller_owned_output_guards(ext, off):
    # dx_acc carved from the middle of a sentinel-filled buffer; off = 67
    # leaves the carve 2 bytes off a 16-byte boundary (scalar fallback)
    N, C, H, Kout = 2, 24, 5, 16
    n = N * H * H * C
    dy, w = rand_cl(N, Kout, H, H, seed=16), rand_cl(Kout, C, 1, 1, seed=17)
    torch.manual_seed(18)
    init = (torch.rand(n, device="cuda") * 2 - 1).to(torch.bfloat16)
    sentinel = 12288.0  # exact in bf16

    def run():
        buf = torch.full((n + 2 * 128,), sentinel, device="cuda",
                         dtype=torch.bfloat16)
        buf[off:off + n] = init
        dx = buf[off:off + n].view(N, H, H, C).permute(0, 3, 1, 2)
        ext.conv2d_dgrad_acc(dy, w, dx)
        return buf

    (buf,) = both(ext, run)
    assert bool((buf[:off].float() == sentinel).all())
    assert bool((buf[off + n:].float() == sentinel).all())
    assert not torch.equal(buf[off:off + n], init)


@pytest.mark.parametrize("c_f32", [False, True])
def test_pipe256_route(ext, c_f32):
    M, N, K = 8192, 1024, 64
    assert ext.nt_route(M, N, K) == "pipe256"
    a, b = rand2d(M, K, 19), rand2d(N, K, 20)
    both(ext, lambda: ext.gemm_nt(a, b, c_f32))


def test_pipe256_route_linear_fwd(ext):
    # the bias epilogue is not a vector writer: must agree trivially
    M, N, K = 8192, 1024, 64
    a, b = rand2d(M, K, 21), rand2d(N, K, 22)
    bias = torch.zeros(N, device="cuda", dtype=torch.float32)
    both(ext, lambda: ext.linear_fwd(a, b, bias))


@pytest.mark.parametrize("c_f32", [False, True])
def test_fallback_n_not_multiple_of_group(ext, c_f32):
    # N = 20: not a multiple of 8 (bf16); fp32's group of 4 divides it, so
    # the fp32 case takes the vector path at a partial tile instead
    a, b = rand2d(70, 64, 23), rand2d(20, 64, 24)
    both(ext, lambda: ext.gemm_nt(a, b, c_f32))
