"""The exhaustive RANSAC<T,S>::computeMany of the C++ drop-in (the overload without a probability):
tests/cpp/computeManyExhaustiveTest.cxx compiles and links on the CPU; on the GPU it checks computeMany(...)[j]
against the exhaustive compute() on data[j] for the plane, the line and the default (geometric) sphere, and the trace
shows that the batched call (lsqr_ransac_many_exhaustive) ran rather than a loop over compute()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "computeManyExhaustiveTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/computeManyExhaustiveTest"],
                          stdout=subprocess.DEVNULL)


def test_compute_many_exhaustive_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_compute_many_exhaustive_matches_compute_on_gpu():
    if not os.path.exists(PROG):
        _build()
    env = dict(os.environ, LSQR_MANY_TRACE="1")
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
    # one batched call per device comparison (plane, line, sphere), none for the forced host loop
    assert r.stderr.count("ransac_many exhaustive: 62 problems") == 3, r.stderr[-2000:]
    assert "ransac_many lm round 0:" in r.stderr, r.stderr[-2000:]   # the sphere's batched LM stage
