"""RANSAC<T,S>::assignToModelsDense / refineModelsDense of the C++ drop-in: tests/cpp/refineDenseTest.cxx compiles and
links on the CPU (against lsqr_assign_dense / lsqr_refine_dense of the C ABI); on the GPU it runs refineModelsDense on a
planted mixture of three regressions with n = 3 and prints labels and parameters, which must equal
Context.refine_dense on the same rows bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "refineDenseTest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/refineDenseTest"],
                          stdout=subprocess.DEVNULL)


def test_refine_models_dense_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


@pytest.mark.gpu
def test_refine_models_dense_equals_context_refine_dense_on_gpu(tmp_path):
    from lsqrrecipes_amd.context import Context
    if not os.path.exists(PROG):
        _build()
    n, N, M, sigma = 3, 1200, 3, 0.01
    g = np.random.default_rng(31)
    X = g.normal(size=(M, n))
    rows = np.empty((N, n + 1))
    rows[:, :n] = g.normal(size=(N, n))
    rows[:, n] = np.einsum("ij,ij->i", rows[:, :n], X[g.integers(0, M, size=N)]) + sigma * g.normal(size=N)
    start = X + 0.5 * sigma * g.normal(size=X.shape)
    path = tmp_path / "mixture.bin"
    with open(path, "wb") as f:
        f.write(np.array([N, M], dtype=np.uint64).tobytes() + rows.tobytes() + start.tobytes())
    with Context(0) as ctx:
        ctx.set_model(L.DENSE, n, 4 * sigma).upload(rows)
        for max_rounds in (1, 8):
            want = ctx.refine_dense(start, max_rounds=max_rounds)
            r = subprocess.run([PROG, str(path), repr(4 * sigma), str(max_rounds)], capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
            out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if not ln.startswith("model")}
            models = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("model")]
            assert out["rounds"] == [str(want["rounds"]), "converged", str(int(want["converged"]))]
            assert want["rounds"] >= 1 and (max_rounds == 1 or want["converged"])
            labels = np.array(out["labels"], dtype=np.int32)
            assert np.array_equal(labels, want["labels"]) and set(np.unique(labels)) >= {0, 1, 2}
            assert out["assign"] == out["labels"]  # assignToModelsDense of the returned models
            got = np.array([[int(v, 16) for v in m] for m in models], dtype=np.uint64)
            assert np.array_equal(got, np.ascontiguousarray(want["params"]).view(np.uint64))
            assert out["refused"] == ["1"]
