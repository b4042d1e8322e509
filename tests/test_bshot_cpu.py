"""B-SHOT without a GPU: the numpy restatement (bshot_ref.py) against answers derived by hand from features/features_bshot.cpp:109-157,
its vectorised form against its scalar form, the brute-force Hamming search on a case small enough to check by eye, and the host's
handling of a config with Features type "BSHOT"."""
import ctypes as C
import json

import numpy as np

import bshot_ref as br
import host_binding as hb
from test_host_layer import _cfg

f32 = np.float32
INF = np.inf

# (group, result, why). t = (double)sum * 0.9 throughout.
KNOWN = [
    ((0, 0, 0, 0), (0, 0, 0, 0), "case A: sum == 0"),
    ((10, 0.5, 0.25, 0.25), (1, 0, 0, 0), "case B: sum 11, t 9.9, only 10 > 9.9"),
    ((5, 5, 0.5, 0.5), (1, 1, 0, 0), "case C: sum 11, t 9.9, no single, 5 + 5 = 10 > 9.9, every other pair is 5.5 or 1"),
    ((4, 4, 4, 1), (1, 1, 1, 0), "case D: sum 13, t 11.7, pairs <= 8, 4 + 4 + 4 = 12 > 11.7, the other triples are 9"),
    ((1, 1, 1, 1), (1, 1, 1, 1), "case E: sum 4, t 3.6, every triple is 3"),
    # 10 * 0.9 is exactly 9.0 in double (0.9 = 0.9000000000000000222, the product rounds to 9.0), so the single test 9 > 9 FAILS and the
    # pair test 9 + 1 = 10 > 9 gives 1100. A threshold taken as sum * 0.9f = 8.9999998 would let 9 pass alone: case B, 1000. (The
    # single-element bit is what the double comparison decides; the group's result is 1100, not 0000: the first pair test passes.)
    ((9, 1, 0, 0), (1, 1, 0, 0), "the double comparison: 9 > 9.0 fails, the pair 10 > 9.0 passes"),
    # Two single tests pass and no pair test does. With finite sums this cannot happen (two singles above t and their pair at or below it
    # need t < 0, and then sum <= 3 t = 2.7 sum contradicts sum < 0); float overflow does it: sum = -inf, t = -inf, the two finite
    # elements pass alone, -inf > -inf fails, and every pair sum is -inf. The two bits of case B stand and count as case C.
    ((-3e38, -3e38, -INF, -INF), (1, 1, 0, 0), "two singles, no pair: the bits left by case B are case C"),
    ((6, 6, 6, -7), (0, 1, 1, 0), "sum 11, t 9.9: the pairs 01, 02 and 12 are 12 > 9.9, the last one written wins"),
    ((np.nan, 1, 2, 3), (1, 1, 1, 1), "NaN: sum != 0 is true, every comparison false, case E"),
    ((np.nan,) * 4, (1, 1, 1, 1), "a NaN SHOT row becomes ones"),
]


def test_known_answers_of_get_binary_vector():
    for vec, want, why in KNOWN:
        assert tuple(br.binary_vector(vec)) == want, (vec, why)
    rows = np.asarray([v for v, _, _ in KNOWN], f32).reshape(1, -1)
    want = np.asarray([w for _, w, _ in KNOWN], f32).reshape(1, -1)
    assert np.array_equal(br.binarize(rows), want)


def test_a_float_threshold_would_answer_differently():
    """what the (9, 1, 0, 0) group pins: with t = sum * 0.9f carried exactly the single test passes and the group is case B"""
    assert float(f32(10)) * 0.9 == 9.0 and float(f32(10)) * float(f32(0.9)) < 9.0


def mixed_rows(n, seed=5):
    """rows of 352 floats that mix SHOT-like non-negative values (sparse histograms of unit norm), negatives, zeros, -0.0, infinities and
    whole-NaN rows; every fourth group is built to sit near a decision (one, two or three dominant elements)"""
    rng = np.random.default_rng(seed)
    r = rng.random((n, br.DIM)).astype(f32) ** 4
    r[rng.random((n, br.DIM)) < 0.5] = 0
    g = r.reshape(n, -1, 4)
    near = rng.random(g.shape[:2]) < 0.25
    dom = rng.integers(1, 4, g.shape[:2])
    for k in (1, 2, 3):
        m = near & (dom == k)
        cnt = int(m.sum())
        vals = np.zeros((cnt, 4), f32)
        vals[:, :k] = f32(0.9) / k + rng.normal(scale=1e-3, size=(cnt, k)).astype(f32)
        vals[:, k:] = (f32(0.1) / (4 - k) + rng.normal(scale=1e-3, size=(cnt, 4 - k))).astype(f32)
        perm = np.argsort(rng.random((cnt, 4)), axis=1)
        g[m] = np.take_along_axis(vals, perm, axis=1)
    r = g.reshape(n, br.DIM)
    r /= np.maximum(np.linalg.norm(r, axis=1, keepdims=True), 1e-12).astype(f32)
    neg = rng.random(n) < 0.1
    r[neg] = rng.normal(size=(int(neg.sum()), br.DIM)).astype(f32)
    sel = rng.random((n, br.DIM))
    r[sel < 0.01] = -0.0
    r[(sel > 0.01) & (sel < 0.012)] = INF
    r[(sel > 0.012) & (sel < 0.014)] = -INF
    r[(sel > 0.014) & (sel < 0.015)] = f32(3e38)
    r[(sel > 0.015) & (sel < 0.016)] = f32(-3e38)
    r[rng.random(n) < 0.02] = np.nan
    r[0] = 0                                                        # the known answers ride at the start of the first row
    r[0, :4 * len(KNOWN)] = np.asarray([v for v, _, _ in KNOWN], f32).reshape(-1)
    return r


def test_vectorised_restatement_equals_the_scalar_one():
    rows = mixed_rows(64)
    want = np.asarray([br.binary_vector(g) for g in rows.reshape(-1, 4)], f32).reshape(rows.shape)
    got = br.binarize(rows)
    assert np.array_equal(got, want)
    counts = np.bincount(got.reshape(-1, 4).sum(1).astype(int), minlength=5)
    assert (counts > 0).all(), counts                               # zero to four bits all occur
    assert np.isnan(rows).all(1).any() and (got[np.isnan(rows).all(1)] == 1).all()


def test_brute_force_hamming_search():
    words = f32([[1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]])
    q = f32([[1, 1, 0, 0], [0, 0, 0, 1]])
    idx, dist = br.hamming_knn(words, q, 3)
    assert idx.tolist() == [[0, 2, 1], [1, 0, 2]]                  # ties to the lowest row
    assert dist.tolist() == [[0, 0, 2], [1, 3, 3]]
    idx, dist = br.hamming_knn(words[:2], q, 3)
    assert idx.tolist() == [[0, 1, -1], [1, 0, -1]] and np.isnan(dist[:, 2]).all()
    # both FLANN functors are this distance on such rows
    a, b = words[0], words[3]
    l2 = float(((a - b) ** 2).sum())
    s = a + b
    chi2 = float((((a - b) ** 2)[s > 0] / s[s > 0]).sum())
    assert l2 == chi2 == 2.0


def test_host_accepts_bshot_and_reports_its_length():
    """Features type "BSHOT" (refused before this descriptor was built): length 352, Radius 0.1 when the config gives none, the frame
    parameters of SHOT, and the config round-trips"""
    j = json.loads(_cfg(**{"Children/Features/Type": "BSHOT"}))
    del j["Children"]["Features"]["Parameters"]["Radius"]
    m = hb.Model()
    m.config_from_json(json.dumps(j))
    out = json.loads(m.config_to_json())["Children"]["Features"]
    assert out["Type"] == "BSHOT"
    assert abs(out["Parameters"]["Radius"] - 0.1) < 1e-7
    assert out["Parameters"]["ReferenceFrameType"] == "SHOT" and "ReferenceFrameRadius" in out["Parameters"]
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m.h.value)) == br.DIM
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())
    assert json.loads(m2.config_to_json())["Children"]["Features"] == out
    m.close(); m2.close()
