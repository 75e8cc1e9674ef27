"""RANSAC<T,S>::assignToModelsRigid / refineModelsRigid of the C++ drop-in: tests/cpp/refineRigidTest.cxx compiles and
links on the CPU (against lsqr_refine_rigid of the C ABI) and, still on the CPU, turns every other estimator away with
std::invalid_argument; on the GPU it runs both calls for the absolute-orientation, pivot and ray estimators on planted
scenes of three models and prints labels and parameters, which must equal Context.refine_rigid on the same records bit
for bit."""
import os
import subprocess

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "examples", "build", "refineRigidTest")
AUX = 0.017453292519943295


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "build/refineRigidTest"],
                          stdout=subprocess.DEVNULL)


def test_refine_models_rigid_compiles_and_links():
    _build()
    assert os.access(PROG, os.X_OK)


def test_every_other_estimator_is_refused_without_a_device():
    _build()
    r = subprocess.run([PROG, "refuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.split() == ["refused", "1", "empty", "1"]


def _scene(kind, n):
    """three planted models of 30 % each plus clutter, shuffled -> records, start rows (the planted parameters, nudged)"""
    m = (3 * n) // 10
    if kind == "absor":
        made = [synth.absolute_orientation(m, 0.0, seed=0x58000 + j)[:2] for j in range(3)]
        clutter = synth.absolute_orientation(n - 3 * m, 1.0, seed=0x58099)[0]
    elif kind == "ray":
        made = [synth.rays(m, 0.0, seed=0x58100 + j)[:2] for j in range(3)]
        clutter = synth.rays(n - 3 * m, 1.0, seed=0x58199)[0]
    else:
        made = []
        for j, shift in enumerate(([0.0, 0.0, 0.0], [50.0, -45.0, 55.0], [-55.0, 50.0, -48.0])):
            rec, truth = synth.pivot(m, 0.0, seed=0x58200 + j)[:2]
            rec[:, 9:12] += shift
            made.append((rec, truth + np.r_[0.0, 0.0, 0.0, shift]))
        clutter = synth.pivot(n - 3 * m, 1.0, seed=0x58299)[0]
    data = np.vstack([p[0] for p in made] + [clutter])[np.random.default_rng(4321).permutation(n)]
    rows = np.array([p[1] for p in made])
    rows[:, -3:] += 0.05  # not the planted parameters themselves: the refit has something to move
    return np.ascontiguousarray(data), np.ascontiguousarray(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,model,delta", [("absor", L.ABSOR, 2.0), ("pivot", L.PIVOT, 1.0), ("ray", L.RAY, 2.0)])
def test_refine_models_rigid_equals_context_refine_rigid_on_gpu(tmp_path, kind, model, delta):
    from lsqrrecipes_amd.context import Context
    if not os.path.exists(PROG):
        _build()
    N = 2500  # more than one chunk of either size
    data, start = _scene(kind, N)
    path = tmp_path / "scene.bin"
    with open(path, "wb") as f:
        f.write(np.array([N, 3], dtype=np.uint64).tobytes() + data.tobytes() + start.tobytes())
    with Context(0) as ctx:
        ctx.set_model(model, 3, delta, 0, aux=AUX if kind == "ray" else 0.0).upload(data)
        for max_rounds in (0, 1, 8):
            want = ctx.refine_rigid(start, max_rounds=max_rounds)
            r = subprocess.run([PROG, kind, str(path), repr(delta), str(max_rounds)], capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
            out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if not ln.startswith("model")}
            models = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("model")]
            assert out["rounds"] == [str(want["rounds"]), "converged", str(int(want["converged"]))]
            assert want["rounds"] == min(max_rounds, 1) or (want["rounds"] >= 1 and want["converged"])
            labels = np.array(out["labels"], dtype=np.int32)
            assert np.array_equal(labels, want["labels"]) and set(np.unique(labels)) == {-1, 0, 1, 2}
            assert out["assign"] == out["labels"]  # assignToModelsRigid of the returned models
            assert np.array_equal(labels, ctx.assign_rigid(want["params"])["labels"])
            got = np.array([[int(v, 16) for v in m] for m in models], dtype=np.uint64)
            assert np.array_equal(got, np.ascontiguousarray(want["params"]).view(np.uint64))
            assert max_rounds == 0 or np.all(want["status"] == L.OK)
