"""Every C++ MPIAMD_* knob must select the route it names.

The knobs are read once per process into function-local statics, so each
configuration runs in a fresh child that imports the extension and prints
``route_info()`` plus a few ``nt_route(...)`` results as JSON; the parent
asserts the table below. Every knob is one inline function of
``csrc/knobs.h`` and ``route_info()`` calls the very functions the launchers
call, so a knob the dispatch ignores cannot pass. None of this touches the
device: the extension imports on a CPU-only machine, so these tests are
unmarked.

What is proved differs by knob. For the NT family (gemm256, pipe, pipent,
glds under pipemix) and for gelubwd_wt the chosen kernel itself is reported
(``nt_route`` / ``gelubwd_wt_route`` evaluate the dispatch predicate). For
bn_grid, bn_apply_grid, splitmajor, onebuf, sk_cpx and the other flags the
proof is the resolved value only: no launch property such as slab rows or
grid shape is observed. That value is what the launcher's own helper
returns, so it shows the knob reached the launcher, not what the launcher
then did with it; the numerics children cover the latter.

tests/test_knob_numerics_gpu.py imports CONFIGS and re-runs the kernel
numerics tests under each configuration; its children run
``test_this_process_matches_its_knobs`` first, in-process, so a knob that
did not take effect cannot pass the numerics vacuously.
"""
import glob
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi_operator_amd", "ops", "csrc")

# route_info() with nothing set: the production configuration
DEFAULT_INFO = {
    "pipemix": True, "pipegather": True, "pipegather_wgrad": True,
    "pipes2": True, "pipe8": True, "p256x16": True, "gemm256": True,
    "pipe": True, "pipent": True, "glds": True, "onebuf": False,
    "splitmajor": False, "sk_cpx": True, "fwd_sk": True, "dx_sk": -1,
    "linear_sk": True, "conv_splits_force": -1, "wgrad_budget": 512,
    "gelu_deriv": True, "gelubwd_wt": False, "ln_spec": False, "ln2": False,
    "bn_grid": 512, "bn_apply_grid": 2048,
}

# route_info key -> environment variable that drives it
KNOB_ENV = {k: "MPIAMD_" + k.upper() for k in DEFAULT_INFO}
KNOB_ENV["onebuf"] = "MPIAMD_GEMM_ONEBUF"
KNOB_ENV["conv_splits_force"] = "MPIAMD_CONV_SPLITS"

# (M, N, K, splits) probes of the dense NT dispatch and their default route
BIG = (8192, 1024, 128, 1)      # 128 full 256² tiles, K % 64 == 0
BIG_K32 = (8192, 1024, 96, 1)   # same grid, K % 64 == 32
RAGGED = (200, 72, 136, 1)      # every dim ragged
BIG_SK = (8192, 1024, 128, 2)   # split-K never takes a 256² kernel
DEFAULT_NT = {BIG: "pipe256", BIG_K32: "nt256", RAGGED: "pipemix",
              BIG_SK: "pipemix"}

GATHERS_OFF = {"pipegather": False, "pipegather_wgrad": False, "pipes2": False}
MIX_INFO = {"pipemix": False, **GATHERS_OFF}

# id -> (knobs, route_info values that differ from DEFAULT_INFO,
#        nt_route results that differ from DEFAULT_NT)
CONFIGS = {
    "default": ({}, {}, {}),
    "pipe8_0": ({"MPIAMD_PIPE8": "0"}, {"pipe8": False}, {}),
    "p256x16_0": ({"MPIAMD_P256X16": "0"}, {"p256x16": False}, {}),
    "pipe_0": ({"MPIAMD_PIPE": "0"}, {"pipe": False}, {BIG: "nt256"}),
    "gemm256_0": ({"MPIAMD_GEMM256": "0"}, {"gemm256": False},
                  {BIG: "pipemix", BIG_K32: "pipemix"}),
    # the NT fallback reverts; pipemix stays on, so TN and gathers keep the pipe
    "pipent_0": ({"MPIAMD_PIPENT": "0"}, {"pipent": False},
                 {RAGGED: "glds", BIG_SK: "glds"}),
    "pipemix_0": ({"MPIAMD_PIPEMIX": "0"}, MIX_INFO,
                  {RAGGED: "glds", BIG_SK: "glds"}),
    "pipemix_0_glds_0": ({"MPIAMD_PIPEMIX": "0", "MPIAMD_GLDS": "0"},
                         {**MIX_INFO, "glds": False},
                         {RAGGED: "reg", BIG_SK: "reg"}),
    "pipemix_0_glds_0_onebuf": (
        {"MPIAMD_PIPEMIX": "0", "MPIAMD_GLDS": "0", "MPIAMD_GEMM_ONEBUF": "1"},
        {**MIX_INFO, "glds": False, "onebuf": True},
        {RAGGED: "reg", BIG_SK: "reg"}),
    "pipemix_0_splitmajor": (
        {"MPIAMD_PIPEMIX": "0", "MPIAMD_SPLITMAJOR": "1"},
        {**MIX_INFO, "splitmajor": True}, {RAGGED: "glds", BIG_SK: "glds"}),
    # fwd, dgrad and wgrad gathers revert; 1x1 convs and linears keep the pipe
    "pipegather_0": ({"MPIAMD_PIPEGATHER": "0"}, GATHERS_OFF, {}),
    "pipegather_wgrad_0": ({"MPIAMD_PIPEGATHER_WGRAD": "0"},
                           {"pipegather_wgrad": False}, {}),
    "pipes2_0": ({"MPIAMD_PIPES2": "0"}, {"pipes2": False}, {}),
    "no_splitk": ({"MPIAMD_FWD_SK": "0", "MPIAMD_DX_SK": "0",
                   "MPIAMD_LINEAR_SK": "0", "MPIAMD_CONV_SPLITS": "1"},
                  {"fwd_sk": False, "dx_sk": 0, "linear_sk": False,
                   "conv_splits_force": 1}, {}),
    "forced_splitk": ({"MPIAMD_DX_SK": "1", "MPIAMD_CONV_SPLITS": "3",
                       "MPIAMD_SK_CPX": "0"},
                      {"dx_sk": 1, "conv_splits_force": 3, "sk_cpx": False},
                      {}),
    "wgrad_budget_64": ({"MPIAMD_WGRAD_BUDGET": "64"}, {"wgrad_budget": 64},
                        {}),
    "wgrad_budget_2048": ({"MPIAMD_WGRAD_BUDGET": "2048"},
                          {"wgrad_budget": 2048}, {}),
    "bn_grids_64": ({"MPIAMD_BN_GRID": "64", "MPIAMD_BN_APPLY_GRID": "64"},
                    {"bn_grid": 64, "bn_apply_grid": 64}, {}),
    "bn_grid_1": ({"MPIAMD_BN_GRID": "1"}, {"bn_grid": 1}, {}),
    "gelu_deriv_0": ({"MPIAMD_GELU_DERIV": "0"}, {"gelu_deriv": False}, {}),
    "gelubwd_wt": ({"MPIAMD_GELUBWD_WT": "1"}, {"gelubwd_wt": True}, {}),
    "ln_spec": ({"MPIAMD_LN_SPEC": "1"}, {"ln_spec": True}, {}),
    "ln2": ({"MPIAMD_LN2": "1"}, {"ln2": True}, {}),
}


def knob_env(knobs):
    """os.environ with every C++ knob cleared, then `knobs` set."""
    env = {k: v for k, v in os.environ.items()
           if k not in KNOB_ENV.values()}
    env.update(knobs)
    return env


def expected(name):
    _, info, nt = CONFIGS[name]
    return {**DEFAULT_INFO, **info}, {**DEFAULT_NT, **nt}


# fc2-dx problems dy [M][K] . w2 [K][N] as (M, N, K): the FFN shape of
# test_ffn_fused_gelu_pipe256_route_bwd (full 256² tiles, 256 workgroups)
# takes the transpose-plus-pipe256 route iff MPIAMD_GELUBWD_WT=1; a grid under
# the 128-workgroup floor never does
FC2DX_BIG = (4096, 4096, 256)
FC2DX_SMALL = (512, 1024, 256)


def check_routes(name, info, nt_of, wt_of):
    """Assert route_info() == the table row; nt_of(M, N, K, splits) -> str,
    wt_of(M, N, K) -> bool."""
    want_info, want_nt = expected(name)
    assert info == want_info, {k: (info.get(k), v) for k, v in want_info.items()
                               if info.get(k) != v}
    got_nt = {p: nt_of(*p) for p in want_nt}
    assert got_nt == want_nt, (got_nt, want_nt)
    assert wt_of(*FC2DX_BIG) == want_info["gelubwd_wt"]
    assert wt_of(*FC2DX_SMALL) is False


_CHILD = """
import json, sys
sys.path.insert(0, %r)
import torch  # the extension links against libtorch
from mpi_operator_amd.ops import hip_ext
ext = hip_ext()
probes = %r
print("ROUTES " + json.dumps({
    "info": ext.route_info(),
    "nt": [[list(p), ext.nt_route(*p)] for p in probes],
    "wt": [[list(p), ext.gelubwd_wt_route(*p)] for p in %r]}))
"""


def child_routes(knobs):
    code = _CHILD % (ROOT, sorted(DEFAULT_NT), [FC2DX_BIG, FC2DX_SMALL])
    r = subprocess.run([sys.executable, "-c", code], env=knob_env(knobs),
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ROUTES ")][-1]
    out = json.loads(line[len("ROUTES "):])
    return (out["info"], {tuple(p): route for p, route in out["nt"]},
            {tuple(p): wt for p, wt in out["wt"]})


@pytest.mark.parametrize("name", list(CONFIGS))
def test_knob_selects_route(name):
    info, nt, wt = child_routes(CONFIGS[name][0])
    check_routes(name, info, lambda *p: nt[p], lambda *p: wt[p])


def info_from_env(env):
    """route_info() as docs/tuning.md defines it for an arbitrary knob
    environment: default-on flags turn off at a leading '0', default-off
    flags turn on at a leading '1', the gather gates nest under PIPEMIX and
    PIPEGATHER, counts outside their documented range fall back."""
    def val(key):
        return env.get(KNOB_ENV[key])

    def ranged(key, lo, hi, dflt):
        try:
            v = int(val(key) or "")
        except ValueError:
            return dflt
        return v if lo <= v <= hi else dflt

    info = {}
    for key, dflt in DEFAULT_INFO.items():
        if dflt is True:
            info[key] = not (val(key) or "").startswith("0")
        elif dflt is False:
            info[key] = (val(key) or "").startswith("1")
    info["pipegather"] = info["pipegather"] and info["pipemix"]
    info["pipegather_wgrad"] = info["pipegather_wgrad"] and info["pipegather"]
    info["pipes2"] = info["pipes2"] and info["pipegather"]
    v = val("dx_sk")
    info["dx_sk"] = -1 if v is None else int(v.startswith("1"))
    info["conv_splits_force"] = ranged("conv_splits_force", 1, 2 ** 31 - 1, -1)
    info["wgrad_budget"] = ranged("wgrad_budget", 64, 2048, 512)
    info["bn_grid"] = ranged("bn_grid", 1, 8192, 512)
    info["bn_apply_grid"] = ranged("bn_apply_grid", 64, 16384, 2048)
    return info


def test_env_model_agrees_with_table():
    """info_from_env reproduces every explicit row of CONFIGS, so the
    fallback below checks untabled combinations to the same contract."""
    for name, (knobs, _, _) in CONFIGS.items():
        assert info_from_env(knobs) == expected(name)[0], name


def test_this_process_matches_its_knobs():
    """In-process: the knobs this process was started with resolved to the
    table row they name. With nothing set this is the default row; the
    children of tests/test_knob_numerics_gpu.py run it first. A combination
    outside the table (a suite run under an ad-hoc knob) is held to
    info_from_env instead — never skipped."""
    import torch  # noqa: F401
    from mpi_operator_amd.ops import hip_ext
    knobs = {k: v for k, v in os.environ.items() if k in KNOB_ENV.values()}
    names = [n for n, (kn, _, _) in CONFIGS.items() if kn == knobs]
    ext = hip_ext()
    if names:
        check_routes(names[0], dict(ext.route_info()), ext.nt_route,
                     ext.gelubwd_wt_route)
        return
    info, want = dict(ext.route_info()), info_from_env(knobs)
    assert info == want, {k: (info.get(k), v) for k, v in want.items()
                          if info.get(k) != v}
    assert ext.gelubwd_wt_route(*FC2DX_BIG) == want["gelubwd_wt"]


def test_knobs_documented():
    """Knob names read in knobs.h == route_info() keys, each in a docs table
    row; no other csrc file reads the environment."""
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        with open(path, encoding="utf-8") as f:
            text = f.read()
        if os.path.basename(path) == "knobs.h":
            names = set(re.findall(r'\bknob_\w+\(\s*"(MPIAMD_[A-Z0-9_]+)"',
                                   text))
        else:
            assert "getenv(" not in text, path
    info = child_routes({})[0]
    assert set(info) == set(DEFAULT_INFO)
    assert names == {KNOB_ENV[k] for k in info}, \
        names ^ {KNOB_ENV[k] for k in info}
    with open(os.path.join(ROOT, "docs", "tuning.md"), encoding="utf-8") as f:
        rows = [l for l in f if l.lstrip().startswith("|")]
    missing = sorted(n for n in names
                     if not any(re.search(r"`%s`" % n, l) for l in rows))
    assert not missing, f"no table row in docs/tuning.md for {missing}"
