"""RANSAC<T,S>::computeMany of the C++ drop-in for the estimators with record types of their own (absolute
orientation, pivot calibration, ray intersection, 2-D line): tests/cpp/computeManyRigidTest.cxx compiles and links
on the CPU; on the GPU it checks computeMany(...)[j] against compute() with seed(seed() + j)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "computeManyRigidTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/computeManyRigidTest"],
                          stdout=subprocess.DEVNULL)


def test_compute_many_rigid_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_compute_many_rigid_matches_compute_on_gpu():
    if not os.path.exists(PROG):
        _build()
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
