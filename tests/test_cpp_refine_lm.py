"""RANSAC<T,S>::refineModelsLM of the C++ drop-in: tests/cpp/refineLMTest.cxx compiles and links on the CPU (against
lsqr_refine_lm of the C ABI, tests/test_refine_lm_abi.py); on the GPU it checks the call against the C ABI call on the
two-sphere scene, the radii it converges to, and the refusal of any other estimator."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "refineLMTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/refineLMTest"],
                          stdout=subprocess.DEVNULL)


@pytest.mark.gpu
def test_refine_models_lm_matches_the_c_abi_on_gpu():
    if not os.path.exists(PROG):
        _build()
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
