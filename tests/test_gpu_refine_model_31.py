"""Refits with 32 or more models of which model 31 owns records.

The passes keep the set of models present in a chunk as a 64-bit mask and loop over its bits on the scalar unit.  A
scalar copy of that mask that sign-extends its low half turns "model 31 is present" into "models 31 .. 63 are present":
the moment step then writes a zero block for each of the models 32 .. 63, past the chunk's n_models blocks -- over the
next chunk's blocks of models 0 .. 31.  So three planted models are put at rows 3, 9 and 31 of 32, the other rows far
from every record, over several chunks of the pass, and the call is compared bit for bit with the call that is given the
three rows alone: a model's refit depends on its own records and row, not on the other rows of the call or on where it
sits among them (DESIGN.md sections 14 and 14.4)."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context

pytestmark = pytest.mark.gpu
WHERE = [3, 9, 31]
N = 3 * 2048 + 5  # the point models' chunk is 2048 records: three chunks and a short one


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def scene(gen):
    """three planted models of a third of the records each, shuffled -> records, their three rows"""
    parts, rows = [], []
    for j in range(3):
        pts, row, _ = gen(N // 3 + (j < N % 3), 0.0, seed=0x3100 + j, sigma=0.1)
        parts.append(pts)
        rows.append(row)
    data = np.vstack(parts)
    return np.ascontiguousarray(data[np.random.default_rng(31).permutation(len(data))]), np.array(rows)


def among_32(rows, far):
    """the three rows at WHERE among 32, the others copies moved `far` away from every record"""
    out = rows[np.arange(32) % 3] + far
    out[WHERE] = rows
    return out


def check(three, many):
    assert np.all(three["n_used"] > 500) and three["rounds"] >= 1
    assert np.array_equal(bits(many["params"][WHERE]), bits(three["params"]))
    assert np.array_equal(many["n_used"][WHERE], three["n_used"]) and many["rounds"] == three["rounds"]
    relabel = np.array(WHERE + [-1])  # label in the three-row call -> in the 32-row call; -1 stays
    assert np.array_equal(many["labels"], relabel[three["labels"]])
    assert np.all(many["status"][WHERE] == L.OK) and int(many["counts"][WHERE].sum()) == int(three["counts"][:3].sum())


def test_refine_plane(ctx):
    data, rows = scene(synth.plane)
    ctx.set_model(L.PLANE, 3, 0.5, L.LS_ALGEBRAIC).upload(data)
    start = rows + np.array([0, 0, 0, 0.05, -0.05, 0.05])  # the point moved off, inside the band
    far = np.array([0, 0, 0, 1e6, 1e6, 1e6])
    for max_rounds in (1, 4):
        check(ctx.refine(start, max_rounds=max_rounds), ctx.refine(among_32(start, far), max_rounds=max_rounds))


def test_refine_grouped_plane(ctx):
    """one group of all records through the grouped pass"""
    data, rows = scene(synth.plane)
    ctx.set_model(L.PLANE, 3, 0.5, L.LS_ALGEBRAIC).upload(data)
    start = rows + np.array([0, 0, 0, 0.05, -0.05, 0.05])
    many = among_32(start, np.array([0, 0, 0, 1e6, 1e6, 1e6]))
    groups = np.zeros(len(data), dtype=np.int32)
    three = ctx.refine(start, max_rounds=2)
    got = ctx.refine_grouped(groups, 1, many[None], max_rounds=2)
    assert np.array_equal(bits(got["params"][0, WHERE]), bits(three["params"]))
    assert np.array_equal(got["n_used"][0, WHERE], three["n_used"]) and got["rounds"][0] == three["rounds"]


def test_refine_lm_sphere(ctx):
    data, rows = scene(synth.sphere)
    ctx.set_model(L.SPHERE, 3, 0.5, L.LS_GEOMETRIC).upload(data)
    start = rows + np.array([0.05, -0.05, 0.05, 0.02])
    far = np.array([1e6, 1e6, 1e6, 0])
    three, many = ctx.refine_lm(start, max_rounds=2), ctx.refine_lm(among_32(start, far), max_rounds=2)
    check(three, many)
    assert np.array_equal(many["lm_nfev"][WHERE], three["lm_nfev"])
    groups = np.zeros(len(data), dtype=np.int32)
    got = ctx.refine_lm_grouped(groups, 1, among_32(start, far)[None], max_rounds=2)
    assert np.array_equal(bits(got["params"][0, WHERE]), bits(three["params"]))
    assert np.array_equal(got["lm_nfev"][0, WHERE], three["lm_nfev"])
