"""RANSAC<T,S>::computeManySequential of the C++ drop-in: tests/cpp/computeManySequentialTest.cxx compiles and links on
the CPU (against lsqr_ransac_many_sequential of the C ABI); on the GPU it checks computeManySequential against
computeSequential per problem for the plane and for a user-defined plugin estimator."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "computeManySequentialTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/computeManySequentialTest"],
                          stdout=subprocess.DEVNULL)


def test_compute_many_sequential_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_compute_many_sequential_matches_compute_sequential_on_gpu():
    if not os.path.exists(PROG):
        _build()
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
