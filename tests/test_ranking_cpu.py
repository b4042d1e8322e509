"""Feature ranking without a GPU: the numpy transcription (ranking_ref.py) against answers derived by hand, the selection window at its
edges, and the FeatureRanking family of the C++ host mirror (factory, parameters, what is refused)."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
import ranking_ref as ref
import ranking_scenes as scenes

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")

# dim 1, chi2(x, y) = (x - y)^2 / (x + y): class 0 = {a = 1, b = 3}, class 1 = {c = 0, e = 8}
#   ab = 1, ac = 1, ae = 49/9, bc = 3, be = 25/11, ce = 8
LINE = np.asarray([[1.0], [3.0], [0.0], [8.0]], np.float32)
LINE_OFF = [0, 2, 4]
BE, AE = f32(25.0) / f32(11.0), f32(49.0) / f32(9.0)


def test_line_knn_activation(ora):
    # KSearch 2 -> 3 results, the first two score. a: (a, b, c) [b before c: the tie goes to the lower row]; b: (b, a, e); c: (c, a, b); e: (e, b, a)
    s = ref.scores(ora.knn, "KNNActivation", LINE, LINE_OFF, 2, increment_type=1)
    assert s.tolist() == [3.0, 3.0, 1.0, 1.0]
    assert np.array_equal(ref.scores(ora.knn, "KNNActivation", LINE, LINE_OFF, 2, increment_type=0), s)       # 0 means 1
    assert np.array_equal(ref.scores(ora.knn, "KNNActivation", LINE, LINE_OFF, 2, increment_type=7), s)       # invalid -> 1
    s2 = ref.scores(ora.knn, "KNNActivation", LINE, LINE_OFF, 2, increment_type=2)
    # a: from a (d 0), b (d 1), c (d 1); b: from a (d 1), b (d 0), e (d 25/11)
    want_b = f32(f32(f32(0.5) + f32(1.0)) + f32(1) / f32(BE + f32(1)))
    assert s2.tolist() == [2.0, float(want_b), 1.0, 1.0]
    # KSearch 1 -> 2 results, only the first scores: the self match
    assert ref.scores(ora.knn, "KNNActivation", LINE, LINE_OFF, 1, increment_type=1).tolist() == [1.0, 1.0, 1.0, 1.0]
    # more results asked than rows: the 4 valid ones, the last dropped
    assert ref.scores(ora.knn, "KNNActivation", LINE, LINE_OFF, 9, increment_type=1).tolist() == [4.0, 4.0, 2.0, 2.0]


def test_line_incremental(ora):
    s = ref.scores(ora.knn, "Incremental", LINE, LINE_OFF, 2)
    a = f32(f32(f32(0) + f32(-1)) + f32(f32(1) - BE)) + f32(-2)        # from a: 0 - 1; from b: 1 - 25/11; from c: 1 - 3
    b = f32(f32(f32(0) + f32(0)) + f32(-1)) + f32(BE - AE)            # from a: 1 - 1; from b: 0 - 1; from e: 25/11 - 49/9
    assert s.tolist() == [float(f32(a)), float(f32(b)), -1.0, float(-BE)]


def test_line_strangeness(ora):
    s = ref.scores(ora.knn, "Strangeness", LINE, LINE_OFF, 2)
    want = [f32(1) / f32(f32(1) + AE),           # a: own 0 + 1; other c 1 + e 49/9
            f32(1) / f32(BE + f32(3)),           # b: own 0 + 1; other e 25/11 + c 3
            f32(8) / f32(4),                     # c: own 0 + 8; other a 1 + b 3
            f32(8) / f32(BE + AE)]               # e: own 0 + 8; other b 25/11 + a 49/9
    assert s.tolist() == [float(w) for w in want]
    # three classes, one empty: its sum is 0 and the smallest of the others, every score x / 0
    s = ref.scores(ora.knn, "Strangeness", LINE, [0, 2, 2, 4], 2)
    assert np.isposinf(s).all()


def test_line_naive_bayes(ora):
    s = ref.scores(ora.knn, "NaiveBayes", LINE, LINE_OFF, 2, dist_threshold=1.5)
    # a: pos {a, b}, neg {c}; b: pos {b, a}, neg {}; c: pos {c}, neg {a}; e: pos {e}, neg {}
    want = [f32(1) / f32(f32(3) / f32(4)), f32(1) / f32(f32(2) / f32(4)), f32(0.5) / f32(f32(2) / f32(4)), f32(0.5) / f32(f32(1) / f32(4))]
    assert s.tolist() == [float(w) for w in want]
    # strictly below: a threshold equal to a distance does not count it
    s = ref.scores(ora.knn, "NaiveBayes", LINE, LINE_OFF, 2, dist_threshold=1.0)
    assert s[0] == f32(0.5) / f32(f32(1) / f32(4))           # a: pos {a}, neg {}


def test_plane_incremental(ora):
    # dim 2: (1,0), (0,1), (1,1): chi2 = 2, 1, 1. KSearch 1: every row's self match gets 0 - 1
    rows = np.asarray([[1, 0], [0, 1], [1, 1]], np.float32)
    assert ref.scores(ora.knn, "Incremental", rows, [0, 2, 3], 1).tolist() == [-1.0, -1.0, -1.0]
    # KSearch 2: (1,0): self 0 - 1, (1,1) 1 - 2; (0,1): self 0 - 1, (1,1) 1 - 2; (1,1): self 0 - 1, (1,0) 1 - 1
    assert ref.scores(ora.knn, "Incremental", rows, [0, 2, 3], 2).tolist() == [-1.0, -1.0, -3.0]


# ---- selection ------------------------------------------------------------------------------------------------------------------
def _kept(score, off, factor, offset):
    keep, n_keep = ref.select(np.asarray(score, np.float32), off, factor, offset)
    return np.nonzero(keep)[0].tolist(), n_keep.tolist()


def test_select_integer_ties():
    score = [3, 1, 2, 1, 3, 3, 0, 1, 2, 2, 1, 0]
    # ascending (score, index): 6 11 | 1 3 7 10 | 2 8 9 | 0 4 5; 0.75 of 12 keeps ranks 0 .. 8
    assert _kept(score, [0, 12], 0.75, 0.0) == ([1, 2, 3, 6, 7, 8, 9, 10, 11], [9])
    # ranks 6 .. 11 (offset 0.5, clamped at 12)
    assert _kept(score, [0, 12], 0.75, 0.5) == ([0, 2, 4, 5, 8, 9], [6])
    assert _kept(score, [0, 12], 0.25, 0.25) == ([3, 7, 10], [3])         # ranks 3 .. 5


def test_select_seven_at_factor_0_3():
    # 7 * 0.3 = 2.1: ranks 0, 1, 2 are below it
    kept, n = _kept([0.5, 0.1, 0.9, 0.3, 0.7, 0.2, 0.6], [0, 7], 0.3, 0.0)
    assert kept == [1, 3, 5] and n == [3]


def test_select_clamps_and_extremes():
    score = np.arange(8, dtype=np.float32)[::-1].copy()
    assert _kept(score, [0, 8], 0.5, -0.25) == ([6, 7], [2])              # min clamped at 0, max = 8 * 0.25
    assert _kept(score, [0, 8], 0.5, 0.75) == ([0, 1], [2])               # max clamped at 8
    assert _kept(score, [0, 8], 0.0, 0.0) == ([], [0])
    assert _kept(score, [0, 8], 1.0, 0.0) == (list(range(8)), [8])
    assert _kept(score, [0, 8], 0.5, 1.0) == ([], [0])                    # the window starts past the end


def test_select_signed_zero_inf_nan():
    # -0 == +0: the zeros rank by index, not by sign
    assert _kept([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -0.0, 0.0], [0, 8], 0.5, 0.0) == ([0, 1, 3, 5], [4])
    inf, nan = np.inf, np.nan
    assert ref.ranked_order(np.asarray([inf, 1.0, -inf, inf, 0.0, 2.0, -inf, inf], np.float32)).tolist() == [2, 6, 4, 1, 5, 0, 3, 7]
    # NaN after +inf, among themselves by index
    assert ref.ranked_order(np.asarray([nan, 1.0, inf, nan, -1.0, 0.5, nan, inf, 0.25], np.float32)).tolist() == [4, 8, 5, 1, 2, 7, 0, 3, 6]
    assert _kept([nan, 1.0, inf, nan, -1.0, 0.5, nan, inf, 0.25], [0, 9], 0.5, 0.0) == ([1, 2, 4, 5, 8], [5])        # 4.5: ranks 0 .. 4


def test_select_per_class_and_empty_class():
    name, score, off = scenes.score_vectors()[-1]
    keep, n_keep = ref.select(score, off, 0.5, 0.0)
    # class 0 (5): 2.5 -> ranks 0 .. 2 of (4:0, 2:1, 0:2, 1:2, 3:NaN); class 1 empty; class 2 (1): 0.5 -> rank 0; class 3 (8): ranks 0 .. 3 of
    # (8:-0, 9:0, 11:1, 12:1, 6:5, 7:5, 13:7, 10:inf)
    assert np.nonzero(keep)[0].tolist() == [0, 2, 4, 5, 8, 9, 11, 12] and n_keep.tolist() == [3, 0, 1, 4]


def test_select_nan_first_of_window():
    # rank 6 of the nan vector is index 0 (the first NaN): 0.75 of 9 = 6.75 keeps it
    keep, _ = ref.select(np.asarray([np.nan, 1.0, np.inf, np.nan, -1.0, 0.5, np.nan, np.inf, 0.25], np.float32), [0, 9], 0.75, 0.0)
    assert np.nonzero(keep)[0].tolist() == [0, 1, 2, 4, 5, 7, 8]


# ---- host mirror ----------------------------------------------------------------------------------------------------------------
def _cfg(fw):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["FeatureWeighting"] = fw
    return json.dumps(j)


def _round_trip(fw):
    m = hb.Model()
    m.config_from_json(_cfg(fw))
    out = json.loads(m.config_to_json())["Children"]["FeatureWeighting"]
    m.close()
    return out


@pytest.mark.parametrize("rank_type", ref.TYPES)
def test_host_accepts_ranking_types_and_round_trips(rank_type):
    params = {"KSearch": 7, "DistanceThreshold": 0.25, "Factor": 0.5, "ExtractOffset": 0.125}
    if rank_type == "KNNActivation":
        params.update({"UseFeaturePosition": False, "ScoreIncrementType": 2})
    out = _round_trip({"Type": rank_type, "Parameters": params})
    assert out["Type"] == rank_type
    for k, v in params.items():
        assert out["Parameters"][k] == v, k
    assert out["Parameters"]["ExtractFromList"] == "invalid"
    # defaults (feature_ranking.cpp:24-28, ranking_knn_activation.cpp:17-18)
    d = _round_trip({"Type": rank_type})["Parameters"]
    assert d["KSearch"] == 10 and d["DistanceThreshold"] == pytest.approx(0.1) and d["Factor"] == 0.75 and d["ExtractOffset"] == 0.0
    if rank_type == "KNNActivation":
        assert d["UseFeaturePosition"] is False and d["ScoreIncrementType"] == 0


def test_host_uniform_still_loads():
    assert _round_trip({"Type": "Uniform"})["Type"] == "Uniform"


def test_example_config_loads():
    m = hb.Model()
    m.config_from_json(json.dumps(json.load(open(os.path.join(ROOT, "config", "modelnet10_shot_knn_activation.ism")))["ObjectConfig"]))
    out = json.loads(m.config_to_json())["Children"]["FeatureWeighting"]
    m.close()
    assert out["Type"] == "KNNActivation" and out["Parameters"]["KSearch"] == 10 and out["Parameters"]["Factor"] == 0.75


@pytest.mark.parametrize("fw", [{"Type": "Similarity"}, {"Type": "Bogus"},
                                {"Type": "KNNActivation", "Parameters": {"UseFeaturePosition": True}}])
def test_host_refuses_what_is_not_built(fw):
    m = hb.Model()
    with pytest.raises(hb.HostError, match="built: Uniform, KNNActivation.*Incremental, Strangeness, NaiveBayes"):
        m.config_from_json(_cfg(fw))
    m.close()


def test_host_extract_from_list_is_converted():
    out = _round_trip({"Type": "Incremental", "Parameters": {"Factor": 0.75, "ExtractFromList": "center"}})["Parameters"]
    assert out["ExtractOffset"] == 0.125 == float(ref.extract_offset_from_list("center", 0.75))
    assert _round_trip({"Type": "Incremental", "Parameters": {"Factor": 0.75, "ExtractFromList": "back"}})["Parameters"]["ExtractOffset"] == 0.25
    assert _round_trip({"Type": "Incremental", "Parameters": {"Factor": 0.75, "ExtractFromList": "front", "ExtractOffset": 0.5}})["Parameters"]["ExtractOffset"] == 0.0
    assert _round_trip({"Type": "Incremental", "Parameters": {"Factor": 0.75, "ExtractOffset": 0.5}})["Parameters"]["ExtractOffset"] == 0.5
