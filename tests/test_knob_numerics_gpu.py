"""Kernel numerics under every C++ MPIAMD_* knob configuration.

No second set of references: each case runs a child pytest over existing
node ids of the kernel-numerics files with the knob environment set, so the
fp32/fp64 references and the tolerances are the ones the default route is
held to. The knobs are process-wide statics, hence one fresh child per
configuration. The first node of every child is
tests/test_knob_routes.py::test_this_process_matches_its_knobs, which
asserts in that process that the knobs resolved to the row of the route
table they name — a knob that does not select its route cannot pass here.

Children run one at a time (parent + one child = two GPU processes). A child
that ends abnormally (abort, segfault, time limit, or an illegal memory
access in its output) is terminal: the case fails and every later case in
this file fails at once without starting another process on the device.

Child time limit: with no knob set, the slowest child measured 8.2 s wall on
an MI355X (the pipe8_0 node list, 25 nodes, which ran first and so carried
the cold extension load; the other 21 took 3.8-5.7 s, of which about 3 s is
interpreter start and imports). CHILD_TIMEOUT_S is about ten times the
slowest, rounded up, to absorb a cold load and a busy machine. With the
test_conv_edges nodes added (3 to 15 tiny cases per conv configuration) the
slowest child measured 6.3 s (pipe8_0 again, now 40 nodes, first and cold);
the other 21 took 3.8-5.4 s, so the limit stands.
"""
import re
import subprocess
import sys

import pytest

from test_knob_routes import CONFIGS, ROOT, knob_env

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 90  # ~10 x the 8.2 s measured above

ROUTE_CHECK = "tests/test_knob_routes.py::test_this_process_matches_its_knobs"

_GEMM = "tests/test_gemm_gpu.py::test_gemm_nt_matches_matmul"
_OPS = "tests/test_ops_gpu.py::"
_BERT = "tests/test_bert_gpu.py::"
_FUSED = "tests/test_conv_bn_fused_gpu.py::"


def gemm(*idx):
    """Both output dtypes of the idx-th shapes of test_gemm_nt_matches_matmul:
    0 (128,128,64) 1 (256,256,256) 2 (64,1000,2048) 3 (200,72,136)
    4 (512,384,576) 5 (512,256,64) 6 (768,512,96) 7 (2048,1024,128)
    8 (8192,1024,128) 9 (8192,1024,192)."""
    return [f"{_GEMM}[{f32}-shape{i}]" for i in idx for f32 in (False, True)]


def ragged(*shapes):
    return [f"{_BERT}test_linear_bwd_ragged_shapes[{s}]" for s in shapes]


# test_conv_fwd_dgrad_wgrad: 0 1x1, 1 3x3 s1, 2 128x15x15 3x3 s2, 3 stem 7x7
# s2, 4 1x1 s2
CONV_ALL = [f"{_OPS}test_conv_fwd_dgrad_wgrad[geom{i}]" for i in range(5)]
CONV_S2 = CONV_ALL[2:]
WGRAD_GEMM = "tests/test_gemm_gpu.py::test_gemm_splitk_via_wgrad_path"
_EDGE = "tests/test_conv_edges_gpu.py::"


def edges(*names):
    return [f"{_EDGE}test_conv_edges[{n}]" for n in names]


# test_conv_edges (per-element fp64 bounds): every case that takes a gather
# (not a plain 1x1 GEMM) in fwd, dgrad or wgrad; the stride-2 dgrad cases;
# the cases whose fwd/dgrad k extent can split (2, 3 and 4 k-tiles, 18)
EDGE_GATHER = edges("nonsq-3x3", "nonsq-3x3-s2", "k1x3", "k3x1", "k5x5",
                    "k3x3-p0", "k3x3-p2", "k2x2-s2", "k1x3-s2", "splitk",
                    "c24-k136", "s3", "wgrad-8way", "one-pixel-3x3")
EDGE_S2 = edges("nonsq-3x3-s2", "k1x1-s2", "k1x1-s2-p1", "k2x2-s2", "k1x3-s2")
EDGE_SPLITK = edges("splitk", "nonsq-3x3", "c24-k136")
EDGE_ACC = _EDGE + "test_conv_dgrad_acc"
LINEAR = _OPS + "test_linear_fwd_bwd"
RAGGED_SMALL = ragged("512-1000-2048", "96-24-40", "256-3072-768", "32-2-768",
                      "64-10-64", "96-30-40")
RAGGED_ALL = RAGGED_SMALL + ragged("8192-256-512", "4096-1024-1024")
FFN = _BERT + "test_ffn_fused_gelu_matches_fp32"
FFN256 = _BERT + "test_ffn_fused_gelu_pipe256_route"
FFN256_BWD = _BERT + "test_ffn_fused_gelu_pipe256_route_bwd"
UNSPLIT5 = [f"{_FUSED}test_epilogue_stats_unsplit[geom{i}]" for i in range(5)]
UNSPLIT_256 = _FUSED + "test_epilogue_stats_unsplit[geom6]"  # (32,64,16,16,1024)
SPLIT_FWD_2 = _FUSED + "test_splitk_reduce_stats_fwd[geom0-2]"  # 2x1024x7x7
BN = ([f"{_OPS}test_bn_fwd_bwd[{r}-{c}]" for r in (True, False)
       for c in (8, 64, 2048)]
      # every 2 x .. x 7 x 7 geometry: the fwd ones all split; of the dgrad
      # ones geom0/geom1 do not (no slab: the unfused pair must come back
      # unchanged) and geom3/4/5 split 2, 2 and 4 ways
      + [f"{_FUSED}test_splitk_reduce_stats_fwd[{g}]"
         for g in ("geom0-2", "geom1-4", "geom3-9")]
      + [f"{_FUSED}test_splitk_reduce_stats_bwd[{g}-{r}]"
         for g in ("geom0-1", "geom1-1", "geom3-2", "geom4-2", "geom5-4")
         for r in (True, False)])
LN = ([f"{_BERT}test_layernorm_fwd_bwd_matches_fp32[{s}]"
       for s in ("4096-1024", "100-768", "7-2048", "5-1024")]
      + [_BERT + "test_layer_norm_add_matches_fp32"])

PIPE8_NODES = (gemm(3, 6, 7) + CONV_ALL + UNSPLIT5 + [SPLIT_FWD_2]
               + RAGGED_SMALL + [FFN])
BIG_GEMMS = gemm(8, 9)
NO_SPLIT_NODES = [LINEAR] + RAGGED_ALL + [CONV_ALL[2]]

# configuration (a key of test_knob_routes.CONFIGS) -> node ids
CASES = {
    "pipe8_0": PIPE8_NODES + EDGE_GATHER + [EDGE_ACC],
    "p256x16_0": BIG_GEMMS + [FFN256, UNSPLIT_256],
    "pipe_0": BIG_GEMMS,
    "gemm256_0": BIG_GEMMS,
    "pipent_0": gemm(2, 3) + [LINEAR],
    "pipemix_0": PIPE8_NODES + [WGRAD_GEMM] + EDGE_GATHER + [EDGE_ACC],
    "pipemix_0_glds_0": gemm(*range(8)) + [LINEAR],
    "pipemix_0_glds_0_onebuf": gemm(*range(8)) + [LINEAR],
    # split-major needs splits % 8 == 0: only the 16-slab linear dw engages
    # the swapped grid. The conv wgrad resolves to 2 splits here (2 tiles,
    # 16 k-tiles), so it checks that the knob leaves such a launch tile-major.
    "pipemix_0_splitmajor": ragged("8192-256-512") + [WGRAD_GEMM],
    "pipegather_0": CONV_ALL + [WGRAD_GEMM] + EDGE_GATHER,
    "pipegather_wgrad_0": CONV_ALL + [WGRAD_GEMM] + EDGE_GATHER,
    "pipes2_0": CONV_S2 + EDGE_S2,
    "no_splitk": NO_SPLIT_NODES + EDGE_SPLITK,
    "forced_splitk": NO_SPLIT_NODES + CONV_ALL[:2] + CONV_ALL[3:] + EDGE_SPLITK,
    "wgrad_budget_64": CONV_ALL + [WGRAD_GEMM] + EDGE_GATHER,
    "wgrad_budget_2048": CONV_ALL + [WGRAD_GEMM] + EDGE_GATHER,
    "bn_grids_64": BN,
    "bn_grid_1": BN,
    "gelu_deriv_0": [FFN, FFN256, FFN256_BWD],
    "gelubwd_wt": [FFN256_BWD],
    "ln_spec": LN,
    "ln2": LN,
}

ABNORMAL_RC = (134, 139, 124, 137, -6, -11)
_aborted = None  # set to the case that ended abnormally


def run_child(nodes, knobs):
    """(abnormal reason or None, return code, output) of one child pytest."""
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
           ROUTE_CHECK, *nodes]
    try:
        r = subprocess.run(cmd, env=knob_env(knobs), cwd=ROOT,
                           capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        out = e.stdout if isinstance(e.stdout, str) else \
            (e.stdout or b"").decode(errors="replace")
        return f"no exit within {CHILD_TIMEOUT_S} s", None, out
    out = r.stdout + r.stderr
    if r.returncode in ABNORMAL_RC:
        return f"return code {r.returncode}", r.returncode, out
    if "illegal memory access" in out:
        return "illegal memory access", r.returncode, out
    return None, r.returncode, out


@pytest.mark.parametrize("name", list(CASES))
def test_numerics_under_knobs(name):
    global _aborted
    if _aborted is not None:
        pytest.fail(f"not started: the child of case {_aborted!r} ended "
                    "abnormally, nothing more runs on the device")
    nodes = CASES[name]
    abnormal, rc, out = run_child(nodes, CONFIGS[name][0])
    tail = out[-6000:]
    if abnormal:
        _aborted = name
        pytest.fail(f"child ended abnormally ({abnormal}):\n{tail}")
    assert rc == 0, f"child pytest failed under {CONFIGS[name][0]}:\n{tail}"
    # every node ran and passed: no skip, no deselection, route check included
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) == len(nodes) + 1 and "skipped" not in out, tail
