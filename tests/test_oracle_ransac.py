"""Pins oracle/ransac.c (restated RANSAC.hxx) against outputs of the REFERENCE's own
RANSAC.hxx: committed vectors (tests/golden/ransac_ref_vectors.npz, config1_ref_vectors.npz and
live_ref_vectors.npz, produced through oracle/_ref by tests/golden/make_golden.py) and, when oracle/_ref is present,
live runs."""
import os

import numpy as np
import pytest

from oracle import pyoracle as O
from lsqrrecipes_amd import synth

CASES = ["plane", "sphere", "circle", "line", "dense", "us", "usp"]


@pytest.fixture(scope="module")
def rv(golden_dir):
    return np.load(os.path.join(golden_dir, "ransac_ref_vectors.npz"))


def _cfg(v):
    return O.cfg(int(v[0]), int(v[1]), float(v[2]), int(v[3]))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_restatement_matches_reference_vectors(rv, name, seed):
    c = _cfg(rv[name + "_cfg"])
    data = rv[name + "_data"]
    p = 0.99 if name in ("us", "usp", "dense") else 0.999
    key = "%s_s%d_" % (name, seed)
    r = O.ransac(c, data, p, sampler="ref", seed=seed)
    assert r["fraction"] == rv[key + "fraction"][0]
    assert np.array_equal(r["consensus"], rv[key + "consensus"])  # bit-exact mask
    assert np.array_equal(r["params"], rv[key + "params"])        # same code path -> same bits
    counts = rv[key + "counts"]
    k = O.lib().orc_min_subset(c)
    assert r["iters"] * k == counts[3]                             # rand() calls consumed
    not_dup = r["status"] != 1
    assert not_dup.sum() == counts[0]                              # estimate() calls
    assert np.array_equal(r["subsets"][not_dup], rv[key + "subsets"])  # draw order preserved
    # full-scan variant (no early exit at RANSAC.hxx:94) gives the same answer
    r2 = O.ransac(c, data, p, sampler="ref", seed=seed, full_scan=True)
    assert np.array_equal(r2["consensus"], r["consensus"]) and r2["iters"] == r["iters"]
    # replaying the recorded subsets through the list sampler reproduces the run
    r3 = O.ransac(c, data, p, sampler="list", subsets=r["subsets"])
    assert np.array_equal(r3["consensus"], r["consensus"])
    assert np.array_equal(r3["params"], r["params"])


def test_exhaustive_matches_reference_vectors(rv):
    c = O.cfg(O.PLANE, 3, 0.5)
    r = O.ransac_exhaustive(c, rv["exh_data"])
    assert r["fraction"] == rv["exh_fraction"][0]
    assert np.array_equal(r["consensus"], rv["exh_consensus"])
    assert np.array_equal(r["params"], rv["exh_params"])
    assert rv["exh_subsets"].shape[0] == 14 * 13 * 12 // 6  # all C(14,3), lexicographic
    assert np.array_equal(rv["exh_subsets"][0], [0, 1, 2])
    assert np.array_equal(rv["exh_subsets"][-1], [11, 12, 13])


def test_choose():
    L = O.lib()
    assert L.orc_choose(10, 3) == 120
    assert L.orc_choose(100, 3) == 161700
    assert L.orc_choose(10_000_000, 3) == 0xFFFFFFFF  # saturates (RANSAC.hxx:274-277)
    assert L.orc_choose(2000, 3) == 1331334000


def test_invalid_input_conventions():
    """RANSAC.hxx:16-19: returns 0 and leaves `parameters` untouched."""
    c = O.cfg(O.PLANE, 3, 0.5)
    data = synth.plane(50, 0.2)[0]
    for p in (0.0, 1.0, -0.5, 1.5):
        r = O.ransac(c, data, p)
        assert r["fraction"] == 0 and r["iters"] == 0
    r = O.ransac(c, data[:2], 0.99)
    assert r["fraction"] == 0


@pytest.fixture(scope="module")
def lv(golden_dir):
    return np.load(os.path.join(golden_dir, "live_ref_vectors.npz"))


def _live_cases(seed):
    return (("plane", O.cfg(O.PLANE, 3, 0.5), synth.plane(3000, 0.5, seed=seed)[0], 0.999),
            ("sphere", O.cfg(O.SPHERE, 3, 0.5, O.LS_ALGEBRAIC), synth.sphere(1500, 0.4, seed=seed)[0], 0.99),
            ("line", O.cfg(O.LINE, 2, 0.5), synth.line(500, 0.5, seed=seed, dim=2)[0], 0.999))


@pytest.mark.parametrize("seed", [101, 202, 303, 404])
def test_live_against_reference(lv, seed):
    """the restated loop against the reference's RANSAC.hxx on the same rand() stream: the reference's outputs stored in
    tests/golden/live_ref_vectors.npz (tests/golden/make_golden.py), and a live run when oracle/_ref is present"""
    import hashlib
    for name, c, data, p in _live_cases(seed):
        key = "%s_s%d_" % (name, seed)
        assert np.array_equal(np.frombuffer(hashlib.sha256(data.tobytes()).digest(), dtype=np.uint8),
                              lv[key + "data_sha"])
        refs = [dict(fraction=lv[key + "fraction"][0], params=lv[key + "params"],
                     consensus=np.unpackbits(lv[key + "consensus_bits"])[:len(data)],
                     estimate_calls=lv[key + "estimate_calls"][0])]
        if O.ref_available():
            refs.append(O.ref_ransac(c, data, p, seed=seed, subsets_cap=4096))
        a = O.ransac(c, data, p, sampler="ref", seed=seed)
        for b in refs:
            assert a["fraction"] == b["fraction"]
            assert np.array_equal(a["consensus"], b["consensus"])
            assert np.array_equal(a["params"], b["params"])
            assert (a["status"] != 1).sum() == b["estimate_calls"]


def test_live_reference_invalid_input_untouched(lv):
    """RANSAC.hxx:16-19 leaves the caller's parameters untouched on invalid input; the exhaustive overload clears them
    first (RANSAC.hxx:165): the reference's outputs (stored, and live when oracle/_ref is present) and the restated
    loops', on parameters prefilled with [1, 2, 3]"""
    c = O.cfg(O.PLANE, 3, 0.5)
    data = synth.plane(50, 0.2)[0]
    pre = [1.0, 2.0, 3.0]
    for name, d, p, exh in (("p1", data, 1.0, False), ("n2", data[:2], 0.9, False), ("n2_exh", data[:2], 0.9, True)):
        ref = (lv["invalid_%s_fraction" % name][0], lv["invalid_%s_params" % name])
        assert ref[0] == 0 and np.array_equal(ref[1], [] if exh else pre)
        runs = [O.ransac_exhaustive(c, d, prefill=pre) if exh else O.ransac(c, d, p, prefill=pre)]
        if O.ref_available():
            runs.append(O.ref_ransac(c, d, p, exhaustive=exh, prefill=pre))
        for r in runs:
            assert r["fraction"] == ref[0] and np.array_equal(r["params"], ref[1])


def test_counter_sampler_properties():
    n, k = 1000, 64
    seen = set()
    for h in range(200):
        s = O.ctr_subset(42, h, n, k)
        assert len(set(s.tolist())) == k and s.max() < n
        seen.add(tuple(s.tolist()))
    assert len(seen) == 200
    assert np.array_equal(O.ctr_subset(42, 7, n, k), O.ctr_subset(42, 7, n, k))
    # n == k: a permutation
    s = O.ctr_subset(1, 0, 8, 8)
    assert sorted(s.tolist()) == list(range(8))
    # uniformity (loose): first index of k=3 over n=10
    cnt = np.zeros(10)
    for h in range(20000):
        for v in O.ctr_subset(5, h, 10, 3):
            cnt[v] += 1
    assert np.all(np.abs(cnt / cnt.sum() - 0.1) < 0.01)


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_config1_as_written_restatement_matches_the_reference(golden_dir, seed):
    """BASELINE.json configs[0]: plane, 10 k points, 30 % outliers, p = 0.999 -- the reference's own RANSAC.hxx run
    (tests/golden/config1_ref_vectors.npz) against the restated loop on the same rand() stream: same draws, same
    call counts, same consensus set and parameters, bit for bit; live against oracle/_ref when it is present"""
    import hashlib
    g = np.load(os.path.join(golden_dir, "config1_ref_vectors.npz"))
    data = synth.plane(10_000, 0.3)[0]
    assert np.array_equal(np.frombuffer(hashlib.sha256(data.tobytes()).digest(), dtype=np.uint8), g["data_sha"])
    c = O.cfg(O.PLANE, 3, 0.5)
    key = "s%d_" % seed
    want_mask = np.unpackbits(g[key + "consensus_bits"])[:len(data)]
    r = O.ransac(c, data, 0.999, sampler="ref", seed=seed)
    assert r["fraction"] == g[key + "fraction"][0]
    assert np.array_equal(r["consensus"], want_mask)
    assert np.array_equal(r["params"], g[key + "params"])
    not_dup = r["status"] != 1
    assert not_dup.sum() == g[key + "counts"][0] and r["iters"] * 3 == g[key + "counts"][3]
    assert np.array_equal(r["subsets"][not_dup], g[key + "subsets"])
    if O.ref_available():
        live = O.ref_ransac(c, data, 0.999, seed=seed, subsets_cap=4096)
        assert live["fraction"] == g[key + "fraction"][0] and np.array_equal(live["consensus"], want_mask)
        assert np.array_equal(live["params"], g[key + "params"]) and np.array_equal(live["subsets"], g[key + "subsets"])
