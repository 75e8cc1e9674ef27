"""RANSAC<T,S>::computeGroupedSequential of the C++ drop-in: tests/cpp/computeGroupedSequentialTest.cxx compiles and
links on the CPU (against lsqr_ransac_grouped_sequential of the C ABI); on the GPU it checks computeGroupedSequential on
resident records against computeManySequential on the per-group vectors -- fractions, parameters and labels -- for the
plane (the one batched device call) and a user-defined plugin estimator (the fallback)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "computeGroupedSequentialTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/computeGroupedSequentialTest"],
                          stdout=subprocess.DEVNULL)


def test_compute_grouped_sequential_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_compute_grouped_sequential_matches_compute_many_sequential_on_gpu():
    if not os.path.exists(PROG):
        _build()
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
