"""The fused dropout kernels under the LayerNorm knobs. MPIAMD_LN_SPEC=1
selects the compile-time C8 = 128 / 96 instantiations of ln_fwd_drop_add_k and
ln_bwd_drop_dx_k (the default run only reaches the runtime-loop form), and
MPIAMD_LN2=1 the 2-row dx kernel of the dropout-free ln_bwd. The knobs are
read once per process, so each setting runs in a child pytest: the kernel
tests of test_dropout_gpu.py must pass there (masks bit-exact, fp64 bounds,
da / dgamma / dbeta equal to layernorm_bwd under the same knob), and every
output must carry the bits it carries in this process: the results do not
depend on either knob.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = {"ln_spec": {"MPIAMD_LN_SPEC": "1"}, "ln2": {"MPIAMD_LN2": "1"}}
SELECT = "fused_mask or fused_forward or fused_backward or print_digests"
CHILD_TIMEOUT_S = 240
ABNORMAL_RC = (134, 139, 124, 137, -6, -11)
_aborted = None  # the knob whose child ended abnormally


@pytest.mark.parametrize("name", list(KNOBS))
def test_fused_kernels_under_knob(name):
    global _aborted
    if _aborted is not None:
        pytest.fail(f"not started: the child of {_aborted!r} ended abnormally, "
                    "nothing more runs on the device")
    import test_dropout_gpu as t
    want = t.digests()
    env = dict(os.environ)
    for k in ("MPIAMD_LN_SPEC", "MPIAMD_LN2"):
        env.pop(k, None)
    env.update(KNOBS[name])
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider",
           os.path.join("tests", "test_dropout_gpu.py"), "-k", SELECT]
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _aborted = name
        pytest.fail(f"child did not exit within {CHILD_TIMEOUT_S} s")
    out = r.stdout + r.stderr
    tail = out[-6000:]
    if r.returncode in ABNORMAL_RC or "illegal memory access" in out:
        _aborted = name
        pytest.fail(f"child ended abnormally (rc {r.returncode}):\n{tail}")
    assert r.returncode == 0, f"child pytest failed under {KNOBS[name]}:\n{tail}"
    m = re.search(r"(\d+) passed", out)
    n_cases = len(t.SHAPES) * len(t.PS)
    assert m and int(m.group(1)) == 3 * n_cases + 1 and "skipped" not in out, tail
    got = dict(re.findall(r"^DIGEST (\S+) ([0-9a-f]{64})$", out, re.M))
    assert set(got) == set(want), (sorted(got), sorted(want))
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, f"outputs depend on {KNOBS[name]} at {differ}"
