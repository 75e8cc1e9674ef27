"""RANSAC<T,S>::assignToModelsDenseGrouped / refineModelsDenseGrouped of the C++ drop-in:
tests/cpp/assignRefineDenseGroupedTest.cxx compiles and links on the CPU (against lsqr_assign_dense_grouped /
lsqr_refine_dense_grouped of the C ABI); on the GPU it checks both calls against the per-group loop of
assignToModelsDense / refineModelsDense on three groups, against the C ABI calls they wrap, and the refusal of any other
estimator."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "assignRefineDenseGroupedTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/assignRefineDenseGroupedTest"],
                          stdout=subprocess.DEVNULL)


def test_assign_refine_dense_grouped_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_assign_refine_dense_grouped_matches_the_per_group_loop_on_gpu():
    if not os.path.exists(PROG):
        _build()
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
