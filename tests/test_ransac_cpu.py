"""CPU tests of the RANSAC vote filter (Voting.RansacVoteFiltering): the host library reads and reports the four configuration keys and
refuses RansacRefineModel; known answers of the numpy restatement (tests/ransac_ref.py) of the definition in DESIGN.md §4.6."""
import json
import math
import os

import numpy as np
import pytest

import host_binding as hb
import ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")


def _cfg(**voting):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Voting"]["Parameters"].update(voting)
    return json.dumps(j)


def test_host_config_reads_and_reports_the_ransac_keys():
    m = hb.Model()
    m.config_from_json(_cfg(RansacVoteFiltering=True, RansacInlierThreshold=0.05, RansacInlierThresholdType="ObjectRadius"))
    p = json.loads(m.config_to_json())["Children"]["Voting"]["Parameters"]
    assert p["RansacVoteFiltering"] is True and p["RansacRefineModel"] is False
    assert p["RansacInlierThreshold"] == pytest.approx(0.05) and p["RansacInlierThresholdType"] == "ObjectRadius"
    m2 = hb.Model()
    m2.config_from_json(_cfg())                                   # keys absent: the reference's defaults (voting.cpp:47-50)
    p = json.loads(m2.config_to_json())["Children"]["Voting"]["Parameters"]
    assert p["RansacVoteFiltering"] is False and p["RansacRefineModel"] is False
    assert p["RansacInlierThreshold"] == pytest.approx(0.1) and p["RansacInlierThresholdType"] == "Fixed"


def test_host_config_refuses_refine_model_by_name():
    for extra in ({}, {"RansacVoteFiltering": True}):
        with pytest.raises(hb.HostError) as e:
            hb.Model().config_from_json(_cfg(RansacRefineModel=True, **extra))
        assert "RansacRefineModel" in str(e.value) and "not built" in str(e.value)


def test_python_config_has_the_four_fields(pkg):
    c = pkg.pipeline.IsmConfig()
    assert (c.ransac_vote_filtering, c.ransac_refine_model, c.ransac_inlier_threshold, c.ransac_inlier_threshold_type) == (False, False, 0.1, "Fixed")
    for name in ("ismhip_ransac_filter", "ismhip_find_maxima_ransac", "ismhip_hough3d_maxima_ransac", "ismhip_vote_keypoints", "ismhip_vote_keypoints_csr",
                 "ismhip_codebook_set_word_keypoint"):
        assert name in pkg.capi.EXPORTS


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q); w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _planted(rng, R, t, n_in=40, n_out=25, thr=0.1):
    S = rng.uniform(-1, 1, (n_in + n_out, 3))
    T = S @ R.T + t
    u = rng.normal(size=(n_out, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    T[n_in:] += u * rng.uniform(10 * thr, 20 * thr, (n_out, 1))
    return S, T


def test_ref_recovers_a_planted_motion():
    rng = np.random.default_rng(7)
    R = _rot(rng); t = np.array([0.3, -1.2, 0.7])
    S, T = _planted(rng, R, t)
    r = rr.ransac(S, T, 0.1)
    assert r["kept"] and r["n_inliers"] == 40
    assert np.array_equal(r["mask"], np.arange(65) < 40)
    assert np.abs(r["R"] - R).max() < 1e-6 and np.abs(r["t"] - t).max() < 1e-6
    assert 1 <= r["iterations"] <= 10001 and 0 <= r["best_i"] < r["iterations"]


def test_ref_drops_the_identity_pose_and_degenerate_clusters():
    rng = np.random.default_rng(8)
    S, T = _planted(rng, np.eye(3), np.zeros(3))
    r = rr.ransac(S, T, 0.1)
    assert not r["kept"] and not r["mask"].any() and r["best_i"] >= 0      # found, then dropped: the reference's isIdentity rule
    S2, T2 = _planted(rng, _rot(rng), np.ones(3), n_in=2, n_out=0)
    r = rr.ransac(S2, T2, 0.1)
    assert not r["kept"] and r["iterations"] == 0                          # n = 2
    S3 = np.tile(rng.uniform(-1, 1, (1, 3)), (30, 1)); T3 = rng.uniform(-1, 1, (30, 3))
    r = rr.ransac(S3, T3, 0.1)
    assert not r["kept"] and r["best_i"] == -1 and r["iterations"] == 0    # all training keypoints equal: no good sample
    S4, T4 = _planted(rng, _rot(rng), np.ones(3))
    assert not rr.ransac(S4, T4, 0.0)["kept"] and not rr.ransac(S4, T4, -1.0)["kept"]


def test_ref_sequential_stopping_rule_by_hand():
    # n = 10, counts 3, 3, 10: after i = 0: w = 0.3, k = ln 0.01 / ln(1 - 0.027) = 168.2...; i = 1 does not improve; i = 2: w = 1,
    # p clamps to DBL_EPSILON, k = ln 0.01 / ln 2.2e-16 = 0.1277...: the loop stops at i = 3
    assert rr.stopping_k(3, 10) == pytest.approx(math.log(0.01) / math.log(0.973), rel=1e-12)
    assert 168 < rr.stopping_k(3, 10) < 169 and 0.12 < rr.stopping_k(10, 10) < 0.13
    assert rr.sequential_stop([3, 3, 10] + [0] * 200, 10, 10000) == (10, 2, 3)
    # a constant count never improves again: 5 of 10 -> k = ln 0.01 / ln 0.875 = 34.49 -> hypotheses 0 .. 34
    assert rr.sequential_stop([5] * 200, 10, 10000) == (5, 0, 35)
    # ties keep the lowest index; max_iterations caps the loop at i <= max_iterations
    assert rr.sequential_stop([3] * 200, 10, 100) == (3, 0, 101)
    assert rr.sequential_stop([3] * 200, 10, 0) == (3, 0, 1)
    # no good sample ends the search where it happens
    assert rr.sequential_stop([3, 4, None, 10], 10, 10000) == (4, 1, 2)


def test_ref_draws_are_distinct_and_a_pure_function():
    for n in (3, 4, 7, 400):
        seen = set()
        for i in range(50):
            a, b, c = rr.draw(12345, i, 0, n)
            assert len({a, b, c}) == 3 and 0 <= min(a, b, c) and max(a, b, c) < n
            assert (a, b, c) == rr.draw(12345, i, 0, n)
            seen.add((a, b, c))
        assert n == 3 or len(seen) > 10
    assert rr.draw(12345, 5, 0, 400) != rr.draw(54321, 5, 0, 400)


def test_ref_identity_test_is_eigens():
    assert rr.is_identity(np.eye(3), np.zeros(3))
    assert rr.is_identity(np.eye(3), np.array([9e-5, 0, 0])) and not rr.is_identity(np.eye(3), np.array([2e-4, 0, 0]))
    c, s = math.cos(1e-3), math.sin(1e-3)
    assert not rr.is_identity(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), np.zeros(3))
