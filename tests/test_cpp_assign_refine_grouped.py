"""RANSAC<T,S>::assignToModelsGrouped / refineModelsGrouped of the C++ drop-in: tests/cpp/assignRefineGroupedTest.cxx
compiles and links on the CPU (against lsqr_assign_grouped / lsqr_refine_grouped of the C ABI); on the GPU it checks
both against the C ABI calls for the plane, and the host loop of forceHostLoop() and of a user-defined plugin estimator
against the loop over refineModels on the per-group gathers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "assignRefineGroupedTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/assignRefineGroupedTest"],
                          stdout=subprocess.DEVNULL)


def test_assign_refine_grouped_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_assign_refine_grouped_matches_the_c_abi_on_gpu():
    if not os.path.exists(PROG):
        _build()
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
