"""The float64 FPFH reference (fpfh_ref.py) and the scenes of fpfh_scenes.py, proven on the host (no GPU): the reference reproduces
the known-answer vectors, the CPU oracle -- one float32 evaluation order -- lies inside every interval with equal counts, the
margins are four times what the float32 mode measures, the scenes have the power the GPU test relies on and reach the decisions
they are named after. test_gpu_fpfh.py then holds the device to the same intervals."""
import numpy as np
import pytest

import fpfh_ref as fr
import fpfh_scenes as sc
import frontend_scenes as fs
import grid_model as gm
import kat_checks
import normals_ref as nr

f32 = np.float32
# float32 summation order and float32 weights / increments against the float64 intervals: largest excess of the oracle's row over
# [lo, hi] measured here 4.51e-5 (swap_tie, 83 neighbours; generic 3.5e-5; values up to 100, where one float32 ulp is 7.6e-6), x 8
TOL = 3.7e-4
MEASURED_EXCESS = 4.6e-5
POWER_SCENES = ("generic", "queue_counts", "sum_counts")


def oracle_rows(ora, name):
    po, P, N, ko, KP = sc.arrays(name)
    want, cnt = ora.fpfh33(po, *fs.cols(P), *fs.cols(N), ko, *fs.cols(KP), sc.scene(name)["radius"])
    return want, cnt.astype(np.int64)


def excess(ref, row):
    """how far finite values lie outside [lo, hi] (0 inside); exempt and NaN rows excluded"""
    ok = ~ref.nan & ~ref.exempt
    return np.maximum(ref.lo[ok] - row[ok], row[ok] - ref.hi[ok]).clip(min=0)


def one_object(points, normals, keypoint, radius):
    p = np.asarray(points, f32)
    return fr.fpfh33(np.array([0, len(p)]), p, np.asarray(normals, f32), np.array([0, 1]), np.asarray(keypoint, f32).reshape(1, 3), radius)


# ---------------------------------------------------------------------------------------------- the reference itself
def test_reference_reproduces_the_known_answer_vectors():
    k = kat_checks.KAT["fpfh_two_points"]                    # f2 = -1: the pole, f1 is undecided there; f2 and f3 are decided
    r = one_object(k["points"], k["normals"], k["keypoint"], k["radius"])
    exp = np.asarray(k["expected"])
    assert r.count[0] == 2 and r.undecided[0, fr.POLE_C] == 2 and not r.exempt[0]
    assert (exp >= r.lo[0] - k["tol"]).all() and (exp <= r.hi[0] + k["tol"]).all()
    assert np.array_equal(r.lo[0, 11:], r.hi[0, 11:]) and np.abs(r.lo[0, 11:] - exp[11:]).max() <= k["tol"]

    def decided(points, normals, keypoint, radius):
        r = one_object(points, normals, keypoint, radius)
        assert np.array_equal(r.lo, r.hi) and r.undecided.sum() == 0
        return r.lo[0]
    kat_checks.fpfh_three_points(decided)


def test_float32_mode_is_the_oracles_arithmetic(ora):
    """pairs32 against ismref_pair_features on every pair of the generic scene's second object: f2 and f3 bit for bit, f1 within one
    ulp of pi (numpy's arctan2 against the C library's atan2f), the same pairs skipped"""
    p, n, src, tgt = sc.object_pairs("generic", 1)
    src, tgt = src[:4000], tgt[:4000]
    b = fr.pairs32(p, n, src, tgt)
    for i in range(len(src)):
        ok, f = ora.pair_features(p[src[i]], n[src[i]], p[tgt[i]], n[tgt[i]])
        assert bool(ok) == (not b["skip"][i])
        if ok:
            assert f32(f[1]) == b["f"][i, 1] and f32(f[2]) == b["f"][i, 2], i
            assert abs(float(f[0]) - float(b["f"][i, 0])) <= 2.4e-7, i


def test_margins_are_four_times_the_measured_error():
    worst = dict(t=0.0, seam=0.0, swap=0.0)
    for name in sc.SCENES:
        m = fr.measure(*sc.arrays(name), sc.scene(name)["radius"])
        print(f"{name}: {m['pairs']} pairs, max |t32 - t64| {m['t']:.3g}, y/hypot {m['seam']:.3g}, |cos1| - |cos2| {m['swap']:.3g}")
        for k in worst:
            worst[k] = max(worst[k], m[k])
    print("largest:", worst)
    assert fr.EDGE >= 2e-5                                    # what the device's fast path documents as its difference in t
    assert 4 * worst["t"] <= fr.EDGE <= max(8 * worst["t"], 2e-5)
    assert 4 * worst["seam"] <= fr.SEAM <= 8 * worst["seam"]
    assert 4 * worst["swap"] <= fr.SWAP <= 8 * worst["swap"]
    assert worst["t"] <= 1.01 * fr.MEASURED_T and worst["seam"] <= 1.01 * fr.MEASURED_SEAM and worst["swap"] <= 1.01 * fr.MEASURED_SWAP


# ---------------------------------------------------------------------------------------------- the oracle inside the intervals
@pytest.mark.parametrize("name", list(sc.SCENES))
def test_oracle_lies_inside_the_intervals(ora, name):
    ref = sc.reference(name)
    want, cnt = oracle_rows(ora, name)
    assert np.array_equal(cnt, ref.count)
    assert np.array_equal(np.isnan(want).any(1), ref.nan) and np.array_equal(np.isnan(want).all(1), ref.nan)
    ex = excess(ref, want)
    print(f"{name}: largest excess of the oracle {ex.max(initial=0.0):.3g}, undecided {int(ref.undecided.sum())} of {int(ref.deposits.sum())} "
          f"deposits, exempt keypoints {int(ref.exempt.sum())}")
    assert ex.max(initial=0.0) <= MEASURED_EXCESS <= TOL / 8 * 1.0001
    fin = ~ref.nan & ~ref.exempt
    sums = want[fin].reshape(-1, 3, 11).sum(2)
    zero = (ref.hi[fin].reshape(-1, 3, 11).sum(2) == 0)
    assert (np.abs(sums - 100) <= 1e-3)[~zero].all() and (sums[zero] == 0).all()


@pytest.mark.parametrize("name", POWER_SCENES)
def test_one_wrong_pair_is_four_tolerances(name):
    ref = sc.reference(name)
    ok = ~ref.nan & ~ref.exempt
    print(f"{name}: smallest min_move {ref.min_move[ok].min():.3g}, largest in-ball count {int(ref.n_max.max())}")
    assert (TOL <= ref.min_move[ok] / 4).all()


def test_generic_scene_has_power():
    ref, s = sc.reference("generic"), sc.scene("generic")
    assert not ref.exempt.any() and not ref.nan.any()
    assert ref.undecided.sum() <= 0.02 * ref.deposits.sum()
    assert (((ref.lo == ref.hi) & (ref.lo > 0)).sum(1) >= 20).all()
    assert ref.count.max() <= 50 and ref.count.min() >= 20
    assert [len(k) for k in s["kps"]] == [16, 16, 0, 16, 16] and all(400 <= len(p) <= 1200 for p, _ in s["objs"])
    a, b = s["copy"]
    assert a < b and all(np.array_equal(x, y) for x, y in zip(s["objs"][a] + (s["kps"][a],), s["objs"][b] + (s["kps"][b],)))
    on = [nr.neighbour_mask(p, k, 1e-9, flip_equal=True).any(1) for (p, _), k in zip(s["objs"], s["kps"]) if len(k)]
    assert all(m[:8].all() and not m[8:].any() for m in on)                  # 8 keypoints on surface points, 8 off


# ---------------------------------------------------------------------------------------------- reach
@pytest.mark.parametrize("name", ["f1_edges", "f2_edges"])
def test_edge_scenes_sit_on_every_edge_from_both_sides(ora, name):
    s = sc.scene(name)
    f = s["feature"]
    seen = set()
    for o, (j, side, val) in enumerate(s["meta"]):
        p, n, src, tgt = sc.object_pairs(name, o)
        assert len(src) == 12
        a, b = fr.pairs64(p, n, src, tgt), fr.pairs32(p, n, src, tgt)
        centre = (src == 0) | (tgt == 0)
        assert centre.sum() == 6 and not (a["tie"] | a["pole"] | a["seam"] | a["deg"] | a["skip"]).any()
        assert (b["f"][centre, f] == f32(val)).all()                         # the float32 mode gives the chosen float, bit for bit
        assert (np.abs(a["t"][centre, f] - j) < 2e-6).all() and (a["cat"][centre, f] == fr.EDGE_C).all()
        others = np.ones((12, 3), bool)
        others[centre, f] = False
        frac = a["t"] - np.floor(a["t"])
        assert (np.minimum(frac, 1 - frac)[others] > 0.01).all() and (a["cat"][others] == -1).all()
        for i in np.nonzero(centre)[0]:                                      # the oracle's own value of the feature
            ok, fo = ora.pair_features(p[src[i]], n[src[i]], p[tgt[i]], n[tgt[i]])
            assert ok and (f32(fo[f]) == f32(val) if f == 1 else abs(float(fo[f]) - float(val)) <= 2.4e-7)
        seen.add((j, side))
    assert seen == {(j, side) for j in range(1, 11) for side in (-1, 0, 1)}
    edges = [np.float64(f32(2 * np.pi * j / 11 - np.pi)) if f == 0 else np.float64(f32(2.0 * j / 11 - 1)) for j in range(1, 11)]
    vals = np.array([float(m[2]) for m in s["meta"]]).reshape(10, 3)
    assert (vals[:, 0] < edges).all() and (vals[:, 1] == edges).all() and (vals[:, 2] > edges).all()
    assert (np.nextafter(vals[:, 1].astype(f32), f32(-9)) == vals[:, 0].astype(f32)).all()
    assert (np.nextafter(vals[:, 1].astype(f32), f32(9)) == vals[:, 2].astype(f32)).all()


def test_seam_scene_has_decided_and_undecided_pairs_and_the_signed_zero(ora):
    s = sc.scene("seam")
    for o, want_bin in zip(s["clear"], (10, 0)):                             # y = +-2^-12: decided, bins 10 and 0
        p, n, src, tgt = sc.object_pairs("seam", o)
        a = fr.pairs64(p, n, src, tgt)
        centre = (src == 0) | (tgt == 0)
        assert (a["x"][centre] < 0).all() and (np.abs(a["y"][centre]) == sc.SEAM_CLEAR).all()
        assert (a["masks"][centre, 0] == 1 << want_bin).all() and (a["cat"][centre] == -1).all()
    for o, sign in zip(s["tiny"], (1, -1)):                                  # y = +-2^-40: exact, but below the seam margin
        p, n, src, tgt = sc.object_pairs("seam", o)
        a, b = fr.pairs64(p, n, src, tgt), fr.pairs32(p, n, src, tgt)
        centre = (src == 0) | (tgt == 0)
        assert (a["y"][centre] == sign * sc.SEAM_TINY).all() and (b["y"][centre] == f32(sign * sc.SEAM_TINY)).all()
        assert (a["cat"][centre, 0] == fr.SEAM_C).all() and (a["masks"][centre, 0] == (1 << 10) | 1).all()
    for o in s["rotated"]:                                                   # y = 0 mathematically, rounding noise in float32
        p, n, src, tgt = sc.object_pairs("seam", o)
        a = fr.pairs64(p, n, src, tgt)
        centre = (src == 0) | (tgt == 0)
        assert (a["x"][centre] < 0).all() and (np.abs(a["y"][centre]) < 1e-6).all() and (a["cat"][centre, 0] == fr.SEAM_C).all()
    # the signed-zero probe: the oracle's own y is -0.0f with x < 0 for the pairs whose source is the centre, and its row has them in bin 0
    o = s["zero_probe"]
    p, n, src, tgt = sc.object_pairs("seam", o)
    b = fr.pairs32(p, n, src, tgt)
    neg_zero = (b["y"] == 0) & np.signbit(b["y"]) & (b["x"] < 0)
    assert neg_zero[src == 0].all() and neg_zero.sum() >= 3
    assert (np.floor(b["t"][neg_zero, 0]) < 0).all()                         # atan2(-0, x < 0) = -pi: below zero, clamped to bin 0
    want, _ = oracle_rows(ora, "seam")
    row = want[sc.arrays("seam")[3][o]]
    pos_zero = (b["y"] == 0) & ~np.signbit(b["y"]) & (b["x"] < 0)
    print("signed-zero probe: pairs with y = -0.0f", int(neg_zero.sum()), "with y = +0.0f", int(pos_zero.sum()), "oracle f1 block", row[:11])
    assert row[0] > 50.0 and (row[10] > 0) == bool(pos_zero.any())


def test_swap_tie_scene_has_exact_ties_and_one_ulp_gaps():
    s = sc.scene("swap_tie")
    for o in s["exact"]:
        p, n, src, tgt = sc.object_pairs("swap_tie", o)
        a, b = fr.pairs64(p, n, src, tgt), fr.pairs32(p, n, src, tgt)
        assert len(src) == 2 and (a["gap"] == 0).all() and (b["gap"] == 0).all() and not b["swap"].any()
    p, n, src, tgt = sc.object_pairs("swap_tie", 1)                          # a tie whose roles matter: f3 in bin 10 or bin 0
    a = fr.pairs64(p, n, src, tgt)
    assert (a["cat"][:, 2] == fr.SWAP_C).all() and (a["masks"][:, 2] == (1 << 10) | 1).all()
    gaps = []
    for o in s["ulp"]:
        p, n, src, tgt = sc.object_pairs("swap_tie", o)
        a, b = fr.pairs64(p, n, src, tgt), fr.pairs32(p, n, src, tgt)
        assert a["tie"].all() and (np.abs(np.abs(b["gap"]) - 2.0 ** -24) < 1e-12).all()
        assert np.array_equal(b["swap"], b["gap"] < 0)                       # one ulp of the cosine is enough for acosf to order them
        gaps += np.sign(b["gap"][src == 0]).tolist()
    assert sorted(gaps) == [-1, -1, 1, 1]
    p, n, src, tgt = sc.object_pairs("swap_tie", s["sphere"])
    a = fr.pairs64(p, n, src, tgt)
    assert a["tie"].mean() > 0.8 and (a["cat"][a["tie"]] != fr.SWAP_C).mean() > 0.99


def test_pole_and_degenerate_scene_reaches_its_cases(ora):
    s, ref = sc.scene("pole_and_degenerate"), sc.reference("pole_and_degenerate")
    ko = sc.arrays("pole_and_degenerate")[3]
    p, n, src, tgt = sc.object_pairs("pole_and_degenerate", s["pole"])
    a, b = fr.pairs64(p, n, src, tgt), fr.pairs32(p, n, src, tgt)
    polar = ((src == 0) & (tgt < 3)) | ((tgt == 0) & (src < 3))
    assert (a["hyp"][polar] == 0).all() and (np.abs(b["f"][polar, 1]) == 1).all() and (b["x"][polar] == 0).all() and (b["y"][polar] == 0).all()
    assert (a["cat"][polar, 0] == fr.POLE_C).all()
    for o in s["degenerate"]:
        pp, nn, src, tgt = sc.object_pairs("pole_and_degenerate", o)
        a, b = fr.pairs64(pp, nn, src, tgt), fr.pairs32(pp, nn, src, tgt)
        dg = (src + tgt == 1)
        assert (a["sin"][dg] == 0).all() and a["deg"][dg].all() and b["skip"][dg].all() and not a["deg"][~dg].any()
        assert ref.exempt[ko[o]]
    assert ref.exempt.sum() == len(s["degenerate"])
    want, cnt = oracle_rows(ora, "pole_and_degenerate")
    assert (want[ko[s["degenerate"][0]]] == 0).all() and cnt[ko[s["degenerate"][0]]] == 2
    k0 = ko[s["patch"]]
    assert ref.count[k0] >= 4 + 5 and ref.usable[k0] == ref.count[k0] - 4    # on the fourfold point
    assert ref.usable[k0 + 1] == ref.count[k0 + 1] >= 4 + 5                  # beside it
    assert ref.count[k0 + 2] == 1 and ref.usable[k0 + 2] == 1 and (ref.hi[k0 + 2] == 0).all()     # a point alone in its ball
    assert ref.count[k0 + 3] == 1 and ref.usable[k0 + 3] == 0 and (ref.hi[k0 + 3] == 0).all()     # only a coincident neighbour
    assert ref.nan[k0 + 4:k0 + 7].all() and (ref.count[k0 + 4:k0 + 7] == 0).all()
    g = gm.Grid(s["objs"][s["patch"]][0], s["cell"])
    kp = s["kps"][s["patch"]]
    assert g.ball_cells(kp[4], s["radius"]) is not None and g.ball_cells(kp[6], s["radius"]) is None   # inside / outside the grid


def test_queue_scene_hits_every_count():
    ref = sc.reference("queue_counts")
    assert ref.n_max.tolist() == sc.QUEUE_COUNTS == [2, 3, 64, 65, 66, 128, 129, 130, 193]
    assert (ref.count == 1).all() and (ref.usable == 1).all() and not ref.exempt.any()
    assert ref.min_move.min() >= 0.1


def test_sum_scene_hits_every_count_inside_one_row_step():
    s, ref = sc.scene("sum_counts"), sc.reference("sum_counts")
    n = len(sc.SUM_COUNTS)
    assert ref.usable[:n].tolist() == ref.count[:n].tolist() == sc.SUM_COUNTS == [1, 7, 8, 9, 15, 16, 17, 63, 64, 65]
    for o, c in enumerate(sc.SUM_COUNTS):
        sw = gm.Grid(s["objs"][o][0], s["cell"]).sweep(s["kps"][o][0], s["radius"])
        assert sw["candidates"] == sw["longest_row"] == c                    # one cell row: steps of 64 candidates, 65 = 64 + 1
    g = gm.Grid(s["objs"][s["spread"]][0], s["cell"])
    for q, u in zip(s["kps"][s["spread"]], ref.usable[n:]):
        sw = g.sweep(q, s["radius"])
        assert u >= 20 and sw["rows"] >= 4 and sw["longest_row"] < u         # the neighbours come from several rows, one step each
    assert not ref.exempt.any()


@pytest.mark.parametrize("name", ["exact_radius", "inexact_radius"])
def test_radius_scenes_have_probes_on_all_three_sides(name):
    s, ref = sc.scene(name), sc.reference(name)
    below, equal, above = s["probes"]
    r2 = nr.r2_of(s["radius"])
    for d, rel in ((below, np.less), (equal, np.equal), (above, np.greater)):
        assert rel(f32(d * d), r2) and abs(float(d) - s["radius"]) < 1e-6
    assert nr.sqdist3(f32([[below, 0, 0], [0, equal, 0], [0, 0, above]]), f32([0, 0, 0])).tolist() == [f32(below * below), f32(equal * equal), f32(above * above)]
    # the source point (object 0, point 0, at the origin) and the keypoint (object 1, at the origin) each see 'below' only
    p0, p1 = s["objs"][0][0], s["objs"][1][0]
    for pts, q, probes in ((p0, p0[0], p0[1:4]), (p1, s["kps"][1][0], p1[0:3])):
        assert (q == 0).all()
        assert nr.neighbour_mask(probes, q[None], s["radius"])[0].tolist() == [True, False, False]
        assert nr.neighbour_mask(probes, q[None], s["radius"], flip_equal=True)[0].tolist() == [True, True, False]
    assert nr.neighbour_mask(p0, s["kps"][0], s["radius"])[0, 0]            # the source point is flagged by its keypoint
    assert ref.count[1] == 1 + 2 + 3 and not ref.exempt.any() and ref.undecided.sum() == 0
    assert (s["radius"] == 0.25 and r2 == 0.0625) or f32(s["radius"]) * np.float64(f32(s["radius"])) != np.float64(r2)
