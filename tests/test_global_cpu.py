"""Global-descriptor verification on the host (no GPU): the restatement global_ref.py against hand-derived answers -- the
SHORT_SHOT_GLOBAL histogram at its hard decisions, classifyWithKNN and the seven merge functions on hand-worked tables -- the scenes of
global_scenes.py against the undecided-point cap, and the bindings the GPU tests rely on."""
import math
import struct

import numpy as np
import pytest

import global_ref as gr
import global_scenes as gs

f32, f64 = np.float32, np.float64
I9 = f32([1, 0, 0, 0, 1, 0, 0, 0, 1])
ORIGIN = f32([0, 0, 0])


def polar(r, theta_deg, phi_deg):
    t, p = math.radians(theta_deg), math.radians(phi_deg)
    return [r * math.sin(t) * math.cos(p), r * math.sin(t) * math.sin(p), r * math.cos(t)]


def counts_of(pts, bins=(2, 2, 8), R=1.0, frame=I9, **kw):
    return gr.short_shot_global_counts(f32(pts).reshape(-1, 3), ORIGIN, f32(R), frame, bins, **kw)


def test_five_points_at_bin_centres():
    """identity frame, radius 1, (2, 2, 8): r 0.25 | 0.75 -> r bin 0 | 1, theta 45 | 135 -> 0 | 1, phi = -180 + 22.5 + 45 k -> k;
    index r + 2 theta + 4 phi; +1 each, no interpolation; the row is count / sqrt(5)"""
    spec = [(0.25, 45, 0), (0.75, 45, 3), (0.25, 135, 5), (0.75, 135, 7), (0.75, 45, 3)]
    pts = [polar(r, t, -180 + 22.5 + 45 * k) for r, t, k in spec]
    counts, lower, upper, und = counts_of(pts)
    want = np.zeros(32, np.int64)
    for r, t, k in spec:
        want[(r > 0.5) + 2 * (t > 90) + 4 * k] += 1
    assert want[1 + 0 + 12] == 2
    assert np.array_equal(counts, want) and np.array_equal(lower, want) and np.array_equal(upper, want) and und == 0
    row = gr.row_of_counts(counts)
    assert np.array_equal(row, (want / math.sqrt(7.0)).astype(f32))        # 1 + 1 + 1 + 4 = 7


def test_point_at_the_centroid_is_skipped_and_an_empty_histogram_is_nan():
    counts, *_ = counts_of([[0, 0, 0], [1e-8, 0, 0]])                     # d2 = 0 and 1e-16: neither is > 1e-15
    assert counts.sum() == 0 and np.isnan(gr.row_of_counts(counts)).all()
    counts, *_ = counts_of([[0, 0, 0], [4e-8, 0, 0]])                     # 1.6e-15 counts
    assert counts.sum() == 1


def test_point_on_the_z_axis_takes_atan2_of_zero():
    """(0, 0, 0.3): theta = 0 -> bin 0; phi = atan2(0, 0) = 0 -> raw 4 -> bin 4; r bin 0; (0, 0, -0.3): theta = 180.0000015 -> raw
    2.00000002 -> clamped to 1"""
    counts, *_ = counts_of([[0, 0, 0.3]])
    assert counts[0 + 0 + 4 * 4] == 1 and counts.sum() == 1
    counts, *_ = counts_of([[0, 0, -0.3]])
    assert counts[0 + 2 * 1 + 4 * 4] == 1


def test_phi_of_plus_and_minus_180_degrees():
    """y = +0: phi = pi * 57.29578 = 180.0000015, raw 8.00000003, clamped to 7. y = -1e-30 (a -0.0 does not survive the dot product's
    + 0): phi = -180.0000015, raw -3e-8, int() truncates towards zero: bin 0"""
    counts, *_ = counts_of([[-0.5, 0.0, 0.0]])
    assert counts[1 + 2 * 0 + 4 * 7] == 0 and counts[0 + 2 * 1 + 4 * 7] == 0
    assert counts.sum() == 1 and np.nonzero(counts)[0][0] // 4 == 7
    counts, *_ = counts_of([[-0.5, -1e-30, 0.0]])
    assert counts.sum() == 1 and np.nonzero(counts)[0][0] // 4 == 0


def test_r_equal_to_the_radius_is_clamped():
    """a neighbour needs the FLOAT d2 < r2, but r is taken in double from the float dot products: a point whose float d2 rounds below 1
    while its double r is >= 1 has raw_r >= r_bins and lands in the last bin by the clamp. Found by a seeded search on the unit sphere."""
    rng = np.random.default_rng(5)
    p = rng.normal(size=(200000, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(f32)
    d2 = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).astype(f32) + p[:, 2] * p[:, 2]).astype(f32)
    q = p.astype(f64)
    r = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
    hit = np.nonzero((d2 < f32(1)) & (r >= 1.0))[0]
    assert len(hit) > 0
    for i in hit[:20]:
        counts, *_ = counts_of([p[i]], bins=(4, 1, 1))
        assert counts[3] == 1


def test_log_radius_below_the_minimum_radius_clamps_to_bin_zero():
    """r = 0.01, min_radius 0.1, R = 1, 4 r-bins: 3 * (ln 0.01 - ln 0.1) / ln 10 + 1 = -2 -> int -2 -> clamped to 0; r = 0.1 -> 1;
    r = 0.5 -> 3 * 0.69897 + 1 = 3.097 -> 3. The minimum radius is the parameter itself and nothing is skipped below it."""
    counts, *_ = counts_of([[0.01, 0, 0], [0.1000001, 0, 0], [0.5, 0, 0]], bins=(4, 1, 1), min_radius=0.1, log_radius=True)
    assert counts.tolist() == [1, 1, 0, 1]


@pytest.mark.parametrize("dims", sorted(gr.AUTO_BINS))
def test_every_auto_size(pkg, dims):
    d, bins = gr.configure_spherical_grid(dims, "auto")
    assert d == dims == bins[0] * bins[1] * bins[2]
    assert pkg.capi.global_short_shot_grid(dims, "auto") == (d, bins)
    rng = np.random.default_rng(dims)
    p, _ = gs.blob(rng, 500)
    sel = gr.select(p)
    c, R = gr.centroid_radius(sel)
    counts, lower, upper, und = gr.short_shot_global_counts(sel, c, R, I9, bins)
    d2, _ = gr._sqdist(sel, c)
    assert counts.sum() == int(((d2 < gr.r2_of(R)) & (d2 > 0)).sum()) and len(counts) == dims
    assert (lower <= counts).all() and (counts <= upper).all()


def test_auto_64_differs_from_the_local_descriptor_and_unknown_sizes_fall_back(pkg):
    assert gr.configure_spherical_grid(64)[1] == (4, 2, 8) and pkg.capi.short_shot_grid(64)[1] == (2, 4, 8)
    assert gr.configure_spherical_grid(48) == (32, (2, 2, 8)) == pkg.capi.global_short_shot_grid(48)
    assert gr.configure_spherical_grid(32, "nonsense") == (32, (2, 2, 8)) == pkg.capi.global_short_shot_grid(32, "nonsense")


def test_manual_3_5_7(pkg):
    assert gr.configure_spherical_grid(32, "manual", (3, 5, 7)) == (105, (3, 5, 7)) == pkg.capi.global_short_shot_grid(32, "manual", (3, 5, 7))
    pts = [polar(0.5, 100, 10), polar(0.9, 179, -179), polar(0.1, 1, 179)]
    counts, *_ = counts_of(pts, bins=(3, 5, 7))
    # r 0.5 -> 1, theta 100 -> int(2.78) = 2, phi 10 -> int(7 * 190 / 360 = 3.69) = 3; r 0.9 -> 2, theta 179 -> 4, phi -179 -> 0;
    # r 0.1 -> 0, theta 1 -> 0, phi 179 -> int(6.98) = 6
    want = np.zeros(105, np.int64)
    for r, t, p in ((1, 2, 3), (2, 4, 0), (0, 0, 6)):
        want[r + 3 * t + 15 * p] += 1
    assert np.array_equal(counts, want)


def test_selection_rule_and_centroid_radius():
    """d2 < (float)((double)r * r), strictly: a point exactly on the radius is out; the centroid is the double mean, the radius the
    float norm's maximum"""
    p = f32([[0.5, 0, 0], [0, -0.5, 0], [0.25, 0, 0], [np.nan, 0, 0], [0, 0.4999999, 0]])
    sel = gr.select(p, (0, 0, 0), 0.5)
    assert len(sel) == 2
    c, R = gr.centroid_radius(sel)
    assert np.array_equal(c, (sel.astype(f64).sum(0) / 2).astype(f32))
    assert R == f32(np.sqrt(gr._sqdist(sel, c)[0].max()))
    assert len(gr.select(p)) == 4 and len(gr.select(p, (9, 9, 9), 0.1)) == 0
    c0, R0 = gr.centroid_radius(gr.select(p, (9, 9, 9), 0.1))
    assert np.isnan(c0).all() and R0 == 0


def test_undecided_points_open_the_interval():
    """a point 1e-12 below the r-bin edge of a (2, 1, 1) grid is undecided: lower leaves it out, upper has it in both bins"""
    counts, lower, upper, und = counts_of([[0.5, 0, 0], [0.2, 0, 0]], bins=(2, 1, 1))
    assert und == 1 and lower.tolist() == [1, 0] and upper.tolist() == [2, 1] and counts.tolist() == [1, 1]


def test_scenes_keep_within_the_undecided_cap(ora):
    """The GPU test allows at most 1 % of a scene's points undecided (summed over its regions, per grid): with the oracle's frame at the
    restatement's own centroid and radius, no scene comes near it. The usual undecided point is a region's farthest one, whose float d2
    EQUALS (float)(R * R): exact in float arithmetic, but within eps of the test all the same."""
    for case in gs.all_cases():
        total = {g: 0 for g in range(len(gs.GRIDS[case["name"]]))}
        n_scene = sum(len(gs.finite_points(case, o)[0]) for o in range(len(case["objs"])))
        for (o, centre, radius) in case["regions"]:
            p, _ = gs.finite_points(case, o)
            sel = gr.select(p, centre, -1.0 if radius is None else radius)
            if len(sel) < 5:
                continue
            c, R = gr.centroid_radius(sel)
            frame = ora.shot_lrf([0, len(sel)], sel[:, 0], sel[:, 1], sel[:, 2], [0, 1], c[0:1], c[1:2], c[2:3], float(R))[0]
            for g, (bins, min_radius, log_radius) in enumerate(gs.GRIDS[case["name"]]):
                counts, lower, upper, und = gr.short_shot_global_counts(sel, c, R, frame, bins, min_radius, log_radius)
                total[g] += und
                assert (lower <= counts).all() and (counts <= upper).all()
        assert max(total.values()) <= 0.01 * n_scene, (case["name"], total, n_scene)


def test_tie_scene_is_an_exact_tie(ora):
    """the dyadic mirror cloud: centroid exactly the origin, both sign sums exactly zero on the oracle's frame"""
    import frontend_scenes as fs
    case = gs.tie_case()
    p, _ = gs.finite_points(case, 0)
    c, R = gr.centroid_radius(p)
    assert np.array_equal(c, f32([0, 0, 0])) and len(p) > 16384
    frame = ora.shot_lrf([0, len(p)], p[:, 0], p[:, 1], p[:, 2], [0, 1], c[0:1], c[1:2], c[2:3], float(R))[0]
    d2, _ = gr._sqdist(p, c)
    assert fs.sign_sums(p[d2 < gr.r2_of(R)], frame) == (0, 0)


# ---- classifyWithKNN ------------------------------------------------------------------------------------------------------------------

def s(d):
    return float(gr.knn_score(d))


def test_knn_score_is_exp_of_minus_sqrt_in_float():
    assert abs(s(0.25) - math.exp(-0.5)) < 1e-7 and s(0.0) == 1.0


def test_classify_single_object_mode_majority_and_occurrence_tie():
    """neighbours (class, instance, d): (2, 7, .01) (1, 3, .04) (2, 8, .09) (1, 3, .16): classes 1 and 2 tie at two occurrences -> the
    lowest id, 1 (std::map order); weight = mean score of class 1; instance 3 with both occurrences"""
    cls, cw, inst, iw = gr.classify_with_knn([2, 1, 2, 1], [7, 3, 8, 3], [0.01, 0.04, 0.09, 0.16], max_class=9, single_object_mode=True)
    assert (cls, inst) == (1, 3)
    want = (s(0.04) + s(0.16)) / 2
    assert abs(cw - want) < 1e-6 and abs(iw - want) < 1e-6
    # a clear majority: class 2 three times; instances 8, 8, 7 -> 8
    cls, cw, inst, iw = gr.classify_with_knn([2, 1, 2, 2], [8, 3, 8, 7], [0.01, 0.04, 0.09, 0.16], 9, True)
    assert (cls, inst) == (2, 8)
    assert abs(cw - (s(0.01) + s(0.09) + s(0.16)) / 3) < 1e-6 and abs(iw - (s(0.01) + s(0.09)) / 2) < 1e-6
    # instance tie inside the class: 7 and 8 once each -> 7
    assert gr.classify_with_knn([2, 2], [8, 7], [0.01, 0.04], 9, True)[2] == 7


def test_classify_detection_mode_scores_the_maximums_own_class():
    """outside single-object mode the hypothesis keeps the maximum's class: its mean score among the neighbours, or weight 0 with
    instance 0 when the class is absent from them"""
    cls, cw, inst, iw = gr.classify_with_knn([2, 1, 2], [7, 3, 8], [0.01, 0.04, 0.09], max_class=1, single_object_mode=False)
    assert (cls, inst) == (1, 3) and abs(cw - s(0.04)) < 1e-6 and abs(iw - s(0.04)) < 1e-6
    assert gr.classify_with_knn([2, 1, 2], [7, 3, 8], [0.01, 0.04, 0.09], max_class=5, single_object_mode=False) == (5, 0, 0, 0)
    assert gr.zero_hypothesis(4, 11) == (4, 0, 11, 0)


# ---- the merge functions ---------------------------------------------------------------------------------------------------------------

def table(g=(1, 0.9, 30, 0.8)):
    """three maxima, weights 0.5 / 0.35 / 0.15 (classes 0, 1, 2; instances 10, 30, 20), all with the same hypothesis (single-object mode)"""
    M = gr.Maximum
    return [M(0, 0.5, 10, 0.5, g=g), M(1, 0.35, 30, 0.3, g=g), M(2, 0.15, 20, 0.2, g=g)]


def labels(ms):
    return [(m.cls, m.inst) for m in ms]


def weights(ms):
    return [float(m.weight) for m in ms]


def test_function_1_takes_a_confident_hypothesis_blindly():
    ms = table()
    gr.merge_hypotheses(1, ms, 1.0, min_svm_score=0.7)
    assert labels(ms) == [(1, 30), (1, 30), (2, 20)] and weights(ms) == weights(table())
    ms = table(g=(1, 0.7, 30, 0.8))                         # not ABOVE the score
    gr.merge_hypotheses(1, ms, 1.0, min_svm_score=0.7)
    assert labels(ms) == labels(table())


def test_functions_2_and_3_rate_limit_hit_and_missed():
    """class 1 sits at 0.35 >= 0.5 * 0.6 = 0.3: hit. With rate limit 0.8 (0.4) the walk stops at the second maximum: missed."""
    ms = table()
    gr.merge_hypotheses(3, ms, 1.0, rate_limit=0.6)
    assert labels(ms)[0] == (1, 30)
    ms = table()
    gr.merge_hypotheses(3, ms, 1.0, rate_limit=0.8)
    assert labels(ms)[0] == (0, 10)
    ms = table(g=(2, 0.9, 20, 0.8))                         # class 2 at 0.15 < 0.3: the walk breaks at it
    gr.merge_hypotheses(3, ms, 1.0, rate_limit=0.6)
    assert labels(ms)[0] == (0, 10)
    ms = table()
    gr.merge_hypotheses(2, ms, 1.0, min_svm_score=0.7, rate_limit=0.6)
    assert labels(ms)[0] == (1, 30)
    ms = table(g=(1, 0.6, 30, 0.8))                         # function 2 needs the score as well
    gr.merge_hypotheses(2, ms, 1.0, min_svm_score=0.7, rate_limit=0.6)
    assert labels(ms)[0] == (0, 10)


def test_function_4_upweights_and_zeroes():
    ms = table()
    gr.merge_hypotheses(4, ms, 1.0, weight_factor=1.5)
    assert weights(ms) == [0.5, float(f32(f32(0.35) * f32(1.5))), float(f32(0.15))]
    assert float(ms[1].inst_weight) == float(f32(f32(0.3) * f32(1.5))) and float(ms[0].inst_weight) == 0.5
    ms = table(g=(1, 0.0, 30, 0.0))                         # zero class weight: the consistent maximum is zeroed
    gr.merge_hypotheses(4, ms, 1.0)
    assert weights(ms)[1] == 0.0 and float(ms[1].inst_weight) == 0.0 and weights(ms)[0] == 0.5


def test_functions_5_6_7():
    ms = table()
    gr.merge_hypotheses(5, ms, 1.0)
    assert weights(ms)[1] == float(f32(f32(0.35) * f32(f32(1) + f32(0.9)))) and weights(ms)[0] == 0.5
    assert float(ms[1].inst_weight) == float(f32(f32(0.3) * f32(f32(1) + f32(0.8))))
    ms = table()
    gr.merge_hypotheses(6, ms, 1.0)
    assert weights(ms)[1] == float(f32(f32(0.35) * f32(0.9))) and float(ms[1].inst_weight) == float(f32(f32(0.3) * f32(0.8)))
    ms = table()
    gr.merge_hypotheses(7, ms, 1.0)
    w1, w2 = f32(0.35), f32(0.9)
    assert weights(ms)[1] == float(f32(f32(w1 + w2) - f32(w1 * w2))) and weights(ms)[0] == 0.5
    i1, i2 = f32(0.3), f32(0.8)
    assert float(ms[1].inst_weight) == float(f32(f32(i1 + i2) - f32(i1 * i2)))


def test_functions_4_5_7_keep_away_from_distant_regions():
    """detection mode: a maximum farther than radius / 2 from its region's centroid is left alone; one nearer is merged"""
    M = gr.Maximum
    for fn in (4, 5, 7):
        far = M(1, 0.5, 30, 0.5, pos=(1, 0, 0), g=(1, 0.9, 30, 0.8), roi_centroid=(0.2, 0, 0))
        near = M(1, 0.5, 30, 0.5, pos=(0.5, 0, 0), g=(1, 0.9, 30, 0.8), roi_centroid=(0.2, 0, 0))
        gr.merge_hypotheses(fn, [far, near], 1.0)
        assert float(far.weight) == 0.5 and float(near.weight) != 0.5


def test_merge_sequence_orders_erases_and_normalises():
    """function 4 with a zero hypothesis on the runner-up: it is zeroed, erased, and the rest renormalised; MinThreshold and BestK last"""
    M = gr.Maximum
    ms = [M(0, 0.5, 10, 0.5, g=(0, 0.9, 10, 0.8)), M(1, 0.35, 30, 0.3, g=(1, 0.0, 30, 0.0)), M(2, 0.15, 20, 0.2, g=(5, 0.5, 1, 0.5))]
    out = gr.merge_sequence(ms, 4, 1.0)
    assert labels(out) == [(0, 10), (2, 20)]
    assert abs(sum(weights(out)) - 1) < 1e-6 and abs(weights(out)[0] - 0.75 / 0.9) < 1e-6
    out = gr.merge_sequence([M(0, 0.5, 10, 0.5, g=(0, 0.9, 10, 0.8)), M(1, 0.35, 30, 0.3, g=(1, 0.0, 30, 0.0)), M(2, 0.15, 20, 0.2, g=(5, 0.5, 1, 0.5))],
                            4, 1.0, min_threshold=-0.5, best_k=1)
    assert labels(out) == [(0, 10)]
    assert gr.merge_sequence([], 3, 1.0) == []
    # function 7 can reorder: the runner-up overtakes
    out = gr.merge_sequence([M(0, 0.5, 10, 0.5, g=(0, 0.0, 10, 0.0)), M(1, 0.4, 30, 0.3, g=(1, 0.9, 30, 0.8))], 7, 1.0)
    assert labels(out)[0] == (1, 30)


# ---- the library's bindings -----------------------------------------------------------------------------------------------------------

def test_the_new_entries_are_exported_and_the_abi_version_stays(pkg):
    L = pkg.capi.lib()
    assert L.ismhip_abi_version() == 4
    for name in ("ismhip_global_short_shot", "ismhip_global_shot352"):
        assert name in pkg.capi.EXPORTS and getattr(L, name) is not None


# ---- the host library (no device) -----------------------------------------------------------------------------------------------------
import json      # noqa: E402
import os        # noqa: E402

import global_host as gh                                   # noqa: E402
import host_binding as hb                                  # noqa: E402
from test_host_layer import _BoostReader, _cfg, _toy_codebook      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSG = {"Type": "SHORT_SHOT_GLOBAL", "Parameters": {"ShortShotDims": 32, "ShortShotBinType": "auto"}}


def gcfg(global_features=SSG, **voting):
    j = json.loads(_cfg())
    if global_features is not None:
        j["Children"]["GlobalFeatures"] = global_features
    j["Children"]["Voting"]["Parameters"].update(voting)
    return json.dumps(j)


def test_config_with_global_verification_loads_and_keeps_the_reference_defaults():
    """UseGlobalFeatures with a built type loads, and Voting carries the eight parameters with the defaults of voting.cpp:39-45"""
    m = hb.Model()
    m.config_from_json(gcfg(UseGlobalFeatures=True))
    out = json.loads(m.config_to_json())
    v = out["Children"]["Voting"]["Parameters"]
    assert v["UseGlobalFeatures"] is True
    assert (v["GlobalFeaturesStrategy"], v["GlobalFeaturesK"], v["GlobalFeatureInfluenceType"], v["GlobalFeatureMinPoints"]) == ("KNN", 1, 3, 500)
    assert abs(v["GlobalParamMinSvmScore"] - 0.7) < 1e-6 and abs(v["GlobalParamRateLimit"] - 0.6) < 1e-6 and abs(v["GlobalParamWeightFactor"] - 1.5) < 1e-6
    assert out["Children"]["GlobalFeatures"] == SSG                                  # the child is written back as it was read
    m.config_from_json(gcfg({"Type": "SHOT_GLOBAL"}, UseGlobalFeatures=True, GlobalFeaturesK=5, GlobalFeatureInfluenceType=7))
    v = json.loads(m.config_to_json())["Children"]["Voting"]["Parameters"]
    assert (v["GlobalFeaturesK"], v["GlobalFeatureInfluenceType"]) == (5, 7)


def test_the_shipped_global_config_loads():
    path = os.path.join(ROOT, "config", "modelnet10_shot_global.ism")
    j = json.load(open(path))["ObjectConfig"]
    v = j["Children"]["Voting"]["Parameters"]
    assert v["UseGlobalFeatures"] is True and v["GlobalFeaturesK"] == 1 and v["GlobalFeatureInfluenceType"] == 3
    assert j["Children"]["GlobalFeatures"]["Type"] == "SHORT_SHOT_GLOBAL" and j["Children"]["GlobalFeatures"]["Parameters"]["ShortShotDims"] == 32
    hb.Model().config_from_json(json.dumps(j))


@pytest.mark.parametrize("gtype", ["CSHOT_GLOBAL", "USC_GLOBAL", "GRSD", "ESF", None])
def test_other_global_types_pass_through_and_are_refused_by_name_only_when_asked_for(gtype):
    child = None if gtype is None else {"Type": gtype, "Parameters": {"Anything": 1}}
    m = hb.Model()
    m.config_from_json(gcfg(child))                                                   # UseGlobalFeatures false: carried through
    if child is not None:
        assert json.loads(m.config_to_json())["Children"]["GlobalFeatures"] == child
    with pytest.raises(hb.HostError) as e:
        hb.Model().config_from_json(gcfg(child, UseGlobalFeatures=True))
    assert f'"{gtype or "Dummy"}"' in str(e.value) and "SHORT_SHOT_GLOBAL, SHOT_GLOBAL" in str(e.value)


def test_svm_strategy_is_refused_not_downgraded():
    with pytest.raises(hb.HostError, match="SVM"):
        hb.Model().config_from_json(gcfg(UseGlobalFeatures=True, GlobalFeaturesStrategy="SVM"))
    hb.Model().config_from_json(gcfg(GlobalFeaturesStrategy="SVM"))                 # unused: accepted as before


def test_bad_global_grids_are_refused():
    bad = {"Type": "SHORT_SHOT_GLOBAL", "Parameters": {"ShortShotBinType": "manual", "ShortShotRBins": 8, "ShortShotEBins": 8, "ShortShotABins": 8}}
    with pytest.raises(hb.HostError, match="512|8 x 8 x 8"):
        hb.Model().config_from_json(gcfg(bad))
    ok = {"Type": "SHORT_SHOT_GLOBAL", "Parameters": {"ShortShotBinType": "manual", "ShortShotRBins": 3, "ShortShotEBins": 5, "ShortShotABins": 7}}
    hb.Model().config_from_json(gcfg(ok, UseGlobalFeatures=True))


def test_stored_global_features_round_trip_in_the_reference_field_order(tmp_path):
    """write: Voting::iSaveData's order (voting.cpp:586-613) read back with struct.unpack; read: the loader keeps what it used to drop"""
    rng = np.random.default_rng(8)
    cb = _toy_codebook(rng)
    cls, inst = [0, 0, 2, 2, 2], [4, 5, 6, 7, 7]
    rf = rng.normal(size=(5, 9)).astype(f32); desc = rng.random((5, 32)).astype(f32); radius = rng.random(5).astype(f32)
    m = hb.Model()
    m.config_from_json(gcfg(UseGlobalFeatures=True))
    m.set_codebook(cb, 3)
    m.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    gh.set_global_features(m, cls, inst, rf, desc, radius)
    path = str(tmp_path / "g.ism")
    m.write(path)
    data = open(str(tmp_path / "g.ismd"), "rb").read()
    # a model without global features: the same bytes up to the count, which is then 0
    m0 = hb.Model()
    m0.config_from_json(gcfg({"Type": "GRSD"}))
    m0.set_codebook(cb, 3)
    m0.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    m0.write(str(tmp_path / "g0.ism"))
    data0 = open(str(tmp_path / "g0.ismd"), "rb").read()
    tail = struct.pack("<I", 0) + struct.pack("<I", 0)                               # no class labels, no instance labels
    assert data0.endswith(struct.pack("<I", 0) + tail)
    at = len(data0) - 12                                                              # where the global features start
    assert data[:at] == data0[:at]
    r = _BoostReader(data)
    r.o = at
    assert r.u() == 2
    k = 0
    for c, n_clouds in ((0, 2), (2, 3)):
        assert (r.u(), r.u()) == (c, n_clouds)
        for _ in range(n_clouds):
            assert r.u() == 1
            assert np.array_equal(np.asarray([r.f() for _ in range(9)], f32), rf[k]) and np.array_equal(r.vf(), desc[k])
            assert r.f() == radius[k] and r.u() == inst[k]
            k += 1
    assert (r.u(), r.u()) == (0, 0) and r.o == len(data)
    m2 = hb.Model()
    m2.read(path)
    g = gh.global_features(m2)
    assert g["n_clouds"] == 5 and g["cls"].tolist() == cls and g["inst"].tolist() == inst and g["cloud"].tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(g["rf"], rf) and np.array_equal(g["desc"], desc) and np.array_equal(g["radius"], radius)
    assert len(gh.global_features(m0)["cls"]) == 0



def test_the_host_exports_exist():
    L = hb.lib()
    for name in gh.EXPORTS:
        assert getattr(L, name) is not None


def test_host_classify_matches_the_restatement():
    rng = np.random.default_rng(12)
    for trial in range(200):
        k = int(rng.integers(1, 9))
        nc, ni, nd = rng.integers(0, 4, k), rng.integers(0, 5, k), (rng.random(k) * 2).astype(f32)
        for single in (True, False):
            mc = int(rng.integers(0, 5))
            got = gh.classify_knn(nc, ni, nd, mc, single)
            want = gr.classify_with_knn(nc, ni, nd, mc, single)
            assert (got[0], got[2]) == (want[0], want[2])
            assert abs(got[1] - want[1]) <= 1e-6 * max(1, abs(want[1])) and abs(got[3] - want[3]) <= 1e-6 * max(1, abs(want[3]))


@pytest.mark.parametrize("fn", [1, 2, 3, 4, 5, 6, 7, 9])
def test_host_merge_sequence_matches_the_restatement(fn):
    """hand tables and random ones: labels and order exact, weights to 1e-6 relative (the host compiler may fuse a * b + c)"""
    rng = np.random.default_rng(100 + fn)
    tables = [table(), table(g=(1, 0.0, 30, 0.0)), table(g=(2, 0.9, 20, 0.8)), table(g=(1, 0.7, 30, 0.8))]
    for _ in range(60):
        n = int(rng.integers(1, 7))
        w = np.sort(rng.random(n).astype(f32))[::-1]
        w = (w / w.sum()).astype(f32)
        single = rng.random() < 0.5
        g = (int(rng.integers(0, 3)), float(rng.random() * (rng.random() < 0.8)), int(rng.integers(0, 3)), float(rng.random() * (rng.random() < 0.8)))
        ms = []
        for i in range(n):
            gi = g if single else (int(rng.integers(0, 3)), float(rng.random() * (rng.random() < 0.8)), int(rng.integers(0, 3)), float(rng.random()))
            ms.append(gr.Maximum(int(rng.integers(0, 3)), w[i], int(rng.integers(0, 3)), rng.random(), pos=rng.normal(size=3) * 0.3, g=gi,
                                 roi_centroid=(0, 0, 0) if single else rng.normal(size=3) * 0.3))
        tables.append(ms)
    for ms in tables:
        kw = dict(min_threshold=float(rng.choice([0.0, 0.1, -0.5])), best_k=int(rng.choice([-1, 1, 2])), rate_limit=float(rng.choice([0.6, 0.8])))
        import copy
        want = gr.merge_sequence(copy.deepcopy(ms), fn, 0.5, **kw)
        got = gh.merge_sequence(fn, ms, 0.5, **kw)
        assert labels(got) == labels(want) and [(m.g_cls, m.g_inst) for m in got] == [(m.g_cls, m.g_inst) for m in want]
        for a, b in zip(got, want):
            for x, y in ((a.weight, b.weight), (a.inst_weight, b.inst_weight), (a.g_weight, b.g_weight), (a.g_inst_weight, b.g_inst_weight)):
                assert abs(float(x) - float(y)) <= 1e-6 * max(abs(float(y)), 1e-3), (fn, float(x), float(y))
