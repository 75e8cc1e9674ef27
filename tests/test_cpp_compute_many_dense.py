"""RANSAC<T,S>::computeMany of the C++ drop-in for DenseLinearEquationSystemParametersEstimator<double,n>:
tests/cpp/computeManyDenseTest.cxx compiles and links on the CPU; on the GPU it checks computeMany(...)[j] against
compute() with seed(seed() + j) for n = 3 and n = 20, and the round trace shows that the batched call
(lsqr_ransac_many_dense) ran rather than a loop over compute()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "computeManyDenseTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/computeManyDenseTest"],
                          stdout=subprocess.DEVNULL)


def test_compute_many_dense_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_compute_many_dense_matches_compute_on_gpu():
    if not os.path.exists(PROG):
        _build()
    env = dict(os.environ, LSQR_MANY_TRACE="1")
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
    assert "ransac_many round 0:" in r.stderr, r.stderr[-2000:]
