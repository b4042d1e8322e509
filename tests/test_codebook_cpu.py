"""The float64 codebook references (codebook_ref.py) and the scenes of codebook_scenes.py, proven on the host (no GPU): hand-derived
answers, the CPU oracle's float32 evaluation on every scene it can express, the tolerances, and the conditions under which a
tolerance cannot hide a wrong decision. test_gpu_codebook.py then holds the device to the same references.

Tolerances = 4 x the largest difference between the float32 oracle and the float64 reference over all scenes (the device may
contract multiply-adds where the oracle does not: a margin over a measurement). Measured here:
  vote weights   1.39e-07 (sigma-l2-1; ranks 1.09e-07, frames 7.99e-08)                  -> TOL_W     = 5.6e-07
  votes          2.30e-07 (csr-1024; frames 2.12e-07)                                      -> TOL_XYZ   = 9.2e-07
  cast positions 1.16e-07 (votes_edges, all 16 flag values)                                -> TOL_POS   = 4.7e-07
  cast weights   the oracle's bytes on every slot of every flag value (no matching term within 1e-12 of a rounding boundary)
  class sigma^2  2.93e-05 relative (sigma-l2-352: a small variance of large float32 sums; chi2-352 1.06e-05, dims <= 64 below 4e-06)
                                                                                           -> TOL_SIGMA = 1.2e-04
Smallest min_move: ranks 9.8e-05 (175 TOL_W), the 257 sampled medians of hub 6.04e-06 (10.8 TOL_W).
The oracle expresses a scene through ismref_activate when every feature activates one codeword (its own k = 1 search finds the
designed word); the variable lists of the sigma and csr scenes go through `float32_restatement`, the oracle's operation sequence
over ismref_rotate_into / ismref_rotate_back / ismref_distance. The hub scene (32768 votes of one word) is the reference's alone."""
from fractions import Fraction

import numpy as np
import pytest

import codebook_ref as cr
import codebook_scenes as sc

f32, f64 = np.float32, np.float64
TOL_W = 5.6e-7
TOL_XYZ = 9.2e-7
TOL_POS = 4.7e-7
TOL_SIGMA = 1.2e-4
ROUNDING_MARGIN = 1e-12  # cast weight: the matching term is a double-precision expression rounded once to float; two correct double evaluations
                         # differ by a few 2^-53, so they round to the same float unless the value lies this close to a rounding boundary
NEAR_TIE = 1e-6          # an LRF whose trace is nearer to 0 than a few float32 roundings of its diagonal may take either branch
TRAIN_SCENES = [n for n in sc.SCENES if n != "hub"]


# -------------------------------------------------------------------------------------- the oracle's float32 on a scene
def float32_restatement(ora, name):
    """ismref_activate's operation sequence (oracle/ism_oracle.cpp) for a CSR of activations: float32 votes, weights and sigma^2"""
    s, ref = sc.scene(name), sc.reference(name)
    vf = ref["vote_feature"].astype(np.int64); vo = ref["vote_offsets"].astype(np.int64)
    kp, centre, lrf = s["kp"], s["centre"], s["lrf"]
    xyz = np.stack([ora.rotate_into(lrf[f], centre[f] - kp[f]) for f in vf]) if len(vf) else np.zeros((0, 3), f32)
    w = np.empty(len(vf), f32)
    for e in range(len(vo) - 1):
        for vi in range(vo[e], vo[e + 1]):
            lst = []
            for vj in range(vo[e], vo[e + 1]):
                fj = vf[vj]
                r = ora.rotate_back(lrf[fj], xyz[vi])
                dx, dy, dz = (kp[fj] + r) - centre[vf[vi]]
                d = np.sqrt(f32(f32(dx * dx + dy * dy) + dz * dz))
                lst.append(f32(np.exp(f64(f32(f32(-1) * f32(d * d)) / f32(0.25)))))
            lst = np.sort(np.asarray(lst, f32)); m = len(lst)
            w[vi] = f32(f32(lst[m // 2 - 1] + lst[m // 2]) / f32(2)) if m % 2 == 0 else lst[m // 2]
    return dict(vote_xyz=xyz, vote_weight=w, class_sigma=sigma32(ora, s))


def sigma32(ora, s):
    """class sigma^2 as the oracle and the device take it: float32 functor values, summed one by one in float32"""
    words = s["desc"] if s["codewords"] is None else s["codewords"]
    out = np.full(s["n_classes"], np.nan, f32)
    with np.errstate(all="ignore"):
        for c, smp in enumerate(cr.sigma_samples(s["cls"], s["model"], s["act_off"], s["n_classes"])):
            if smp is None:
                continue
            sf, a0, nw = smp
            d = [f32(ora.distance(s["metric"], s["desc"][f], words[w])) for f in sf for w in s["act_idx"][a0:a0 + nw]]
            total = f32(0)
            for x in d:
                total = f32(total + x)
            mean = total / f32(len(d))
            var = f32(0)
            for x in d:
                diff = f32(x - mean)
                var = f32(var + f32(diff * diff))
            out[c] = var / f32(len(d) - 1)
    return out


def oracle_on(ora, name):
    """the oracle's float32 outputs of a training scene: ismref_activate where it can express the scene, else the restatement"""
    s = sc.scene(name)
    if s["oracle_k1"]:
        want = ora.activate(s["metric"], s["desc"], s["lrf"], s["kp"], s["cls"], s["model"], s["centre"], k=1, clean_up=s.get("clean_up", False),
                            n_classes=s["n_classes"], codewords=s["codewords"])
        ref = sc.reference(name)
        for key in ("word_src", "vote_offsets", "vote_feature"):
            assert np.array_equal(want[key], ref[key]), (name, key)
        return want
    return float32_restatement(ora, name)


def same_kind(a, b):
    """NaN where NaN, the same sign of zero"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[a == 0])) and np.array_equal(a == 0, b == 0)


def sigma_error(got, ref):
    """largest relative difference over the classes with a finite, non-zero sigma^2"""
    ok = np.isfinite(ref) & (ref != 0)
    return float(np.max(np.abs(np.asarray(got, f64)[ok] - ref[ok]) / np.abs(ref[ok]), initial=0.0))


# ----------------------------------------------------------------------------------------------------- hand-derived answers
def neighbour_at_rank(i, m, r):
    """the r-th nearest feature of vote i on the line of sc.line_positions (r = 0: itself), in closed form: the neighbour t places to
    the right lies a little further than the one t places to the left and nearer than the one t + 1 to the left, so the distances
    alternate left, right, left, ... until the shorter side ends, and go on along the longer side"""
    short = min(i, m - 1 - i)
    if r <= 2 * short:
        t = (r + 1) // 2
        return i - t if r % 2 else i + t
    return i + (r - short) if i == short else i - (r - short)


def test_medians_of_ranks_from_the_sorted_distances_on_the_line():
    """identity frames and one centre: the weight of vote i against feature j is exp(-4 (p_j - p_i)^2), p the abscissae. Ascending
    weight = descending distance, so the median of an odd m is the weight of the neighbour at distance rank m // 2 and that of an
    even m the mean over the ranks m / 2 - 1 and m / 2: no sorting, no median rule"""
    s, ref = sc.scene("ranks"), sc.reference("ranks")
    assert np.array_equal(np.diff(ref["vote_offsets"].astype(np.int64)), sc.RANKS_M) and ref["evaluated"].all()
    for e, m in enumerate(sc.RANKS_M):
        v0 = int(ref["vote_offsets"][e])
        p = s["kp"][ref["vote_feature"][v0:v0 + m], 0].astype(f64)
        w = lambda i, r: np.exp(-4 * (p[neighbour_at_rank(i, m, r)] - p[i]) ** 2)
        for i in range(m):
            want = w(i, m // 2) if m % 2 else (w(i, m // 2 - 1) + w(i, m // 2)) / 2
            assert abs(ref["vote_weight"][v0 + i] - want) <= 1e-13, (m, i)
        assert [neighbour_at_rank(0, m, r) for r in range(m)] == list(range(m))              # vote 0: monotone, neighbour m // 2 is the median
    assert ref["vote_weight"][0] == 1.0 and np.isinf(ref["min_move"][0])                       # m == 1
    d = float(s["kp"][2, 0]) - float(s["kp"][1, 0])                                             # m == 2
    assert np.allclose(ref["vote_weight"][1:3], (1 + np.exp(-4 * d * d)) / 2, rtol=0, atol=1e-15)
    assert np.allclose(ref["vote_xyz"], (sc.CENTRE.astype(f64) - s["kp"].astype(f64))[ref["vote_feature"]], rtol=0, atol=0)


def test_ties_give_the_tied_values():
    ref = sc.reference("ties")
    w = np.split(ref["vote_weight"], ref["vote_offsets"][1:-1].astype(np.int64))
    assert np.all(w[0] == 1.0) and np.all(w[1] == 1.0)
    assert np.allclose(w[2], np.exp(-1.0), atol=1e-7) and np.allclose(w[3], np.exp(-4 * 0.125), atol=1e-12)   # side 0.5; edge 0.125 sqrt(8)
    assert np.allclose(w[4], 0.5, atol=1e-40) and np.allclose(w[5], [1, 1, 1, 0, 0], atol=1e-40) and np.allclose(w[6], [0, 1, 1], atol=1e-40)
    assert np.all(w[7] > 1 - 2.0 ** -25) and np.all(w[8] > 1 - 2.0 ** -25)                   # round to exactly 1.0f
    assert np.all(w[7].astype(f32) == 1) and np.all(w[8].astype(f32) == 1)
    assert (ref["min_move"][:9] == 0).all()


def test_smallest_sigma_classes_by_hand():
    for name in ("sigma-l2-3", "sigma-chi2-3", "sigma-l2-33"):
        s, ref = sc.scene(name), sc.reference(name)
        smp = cr.sigma_samples(s["cls"], s["model"], s["act_off"], s["n_classes"])
        assert [None if x is None else (len(x[0]), x[2]) for x in smp] == [(1, 2), (1, 3), (3, 6), (3, 3), (4, 5), (6, 4), None, (2, 0), (1, 1)]
        d = lambda f, a: cr.distance64(s["metric"], s["desc"][f], s["codewords"][s["act_idx"][a]])
        d0, d1 = d(0, 0), d(0, 1)                                          # class 0: its one feature against its two words
        assert np.isclose(ref["class_sigma"][0], (d0 - d1) ** 2 / 2, rtol=1e-12)
        a = int(s["act_off"][2])                                           # class 1: feature 1 against the list of feature 2 (its own is empty)
        assert s["act_off"][2] == s["act_off"][1]
        assert np.isclose(ref["class_sigma"][1], np.var([d(1, a), d(1, a + 1), d(1, a + 2)], ddof=1), rtol=1e-12)
        sig = ref["class_sigma"]
        assert np.isnan(sig[6]) and np.isnan(sig[8]) and sig[7] == 0 and np.signbit(sig[7])
    s = sc.scene("sigma-chi2-3")                                            # x + y == 0 entries are skipped, not divided
    assert np.any((s["desc"][:, None, :] + s["codewords"][None, :, :]) == 0)
    assert cr.distance64(1, [0.0, 0.5, 0.0], [0.0, 0.25, 0.0]) == 0.0625 / 0.75


def test_term3_table_by_hand():
    s, ref = sc.scene("term3"), sc.reference("term3")
    words, cls = s["act_idx"], s["cls"]
    nf = [int(np.sum(cls == c)) for c in range(3)]
    share = lambda c, w: Fraction(int(np.sum((cls == c) & (words == w))), nf[c])
    total = [sum(share(c, w) for c in range(3)) for w in range(4)]
    for c in range(3):
        holding = [w for w in range(4) if share(c, w)]
        t3 = [share(c, w) / total[w] for w in holding]
        assert abs(ref["term3"][c] - float(t3[-1])) <= 1e-15
        assert t3[-1] != t3[0] and t3[-1] != max(t3)               # neither "first wins" nor "max wins"
    assert [float(x) for x in (Fraction(1, 3) / (Fraction(1, 3) + Fraction(1, 5)), Fraction(1, 4) / (Fraction(1, 4) + Fraction(3, 5)),
                               Fraction(1, 5) / (Fraction(1, 3) + Fraction(1, 5)))] == pytest.approx(list(ref["term3"]), abs=1e-15)
    e = 1                                                                   # word 1 holds classes 0, 1, 2 with 1, 2, 1 votes
    v0, v1 = int(ref["vote_offsets"][e]), int(ref["vote_offsets"][e + 1])
    assert v1 - v0 == 4 and np.allclose(ref["vote_class_weight"][v0], (1 / 3) * (1 / 4) * 0.625, atol=1e-15)


def test_cleanup_keeps_words_of_one_vote():
    ref = sc.reference("cleanup")
    assert ref["word_src"].tolist() == [0, 1, 2, 3, 4] and ref["vote_feature"].tolist() == [0, 1, 2, 3, 4]
    assert np.all(ref["vote_class_weight32"] == f32(1 / 5)) and not np.isnan(ref["class_sigma"]).any()


def test_boundary_votes_by_hand():
    s = sc.votes_scene()
    maxv = 4
    r0 = sc.votes_reference(0)
    live = r0["live"].reshape(-1, maxv)
    # activations 0, 1, 2 = word 1 at d = 1.0, one float above, one float below; votes of classes 0 (2 sigma = 1), 1 (NaN), 2 (0.5), 5 (2.0)
    assert live[0].tolist() == [True, True, False, True] and live[1].tolist() == [False, True, False, True] and live[2].tolist() == [True, True, False, True]
    assert live[3].tolist() == [True, True, True, True] and live[4].tolist() == [True, True, False, True] and live[5].tolist() == [True, True, True, True]
    assert live[7].tolist() == [False, True, False, True] and live[8].tolist() == [False, True, False, False] and live[9].tolist() == [False, True, False, True]
    assert not live[6].any() and not live[10].any() and not live[11].any() and not live[15].any()      # a word without votes, idx -1, idx n_words
    assert live[14].tolist() == [False, True, False, False]                                              # d = -1: fabs
    r2 = sc.votes_reference(cr.W_VOTE).copy()
    live2 = r2["live"].reshape(-1, maxv)
    assert live2[12, 0] and r2["weight"][12 * maxv] == f32(cr.FLT_EPSILON) and r2["margin_eps"][12 * maxv] == 0       # exactly FLT_EPSILON: kept
    assert not live2[13, 0] and r2["margin_eps"][13 * maxv] == float(np.nextafter(f32(cr.FLT_EPSILON), f32(0))) - cr.FLT_EPSILON
    r4 = sc.votes_reference(cr.W_MATCHING)
    assert r4["live"][1] and np.isnan(r4["weight"][1]) and r4["cls"][1] == 1                              # NaN sigma: kept, NaN weight
    g = (1 / np.sqrt(2 * np.pi * 0.5)) * np.exp(-1.0 / (2 * 0.5))
    assert r4["weight"][0] == f32(g)
    assert s["idx"].min() == -1 and s["idx"].max() == s["n_words"]


# ------------------------------------------------------------------------------------ the oracle, and the tolerances
def test_quaternions_and_distances_against_the_oracle(ora):
    lrf, n_perm = sc.frame_list()
    q, near, into, back = cr.frames(lrf)
    traces = sorted(set(int(round(np.trace(l.reshape(3, 3)))) for l in lrf[:n_perm]))
    assert traces == [-1, 0, 1, 3]
    v = np.array([0.5, -0.25, 0.125], f32)
    decided = (near == 0) | (near >= NEAR_TIE)                                               # a trace of exactly 0 is exact in float32 too
    assert decided[:n_perm].all() and (near[:n_perm] == 0).sum() == 8 and (~decided[n_perm:]).sum() <= 2
    diag = np.array([np.diag(l.reshape(3, 3)) for l in lrf[:n_perm]])
    assert sum(1 for d in diag if d.sum() <= 0 and (d[0] == d[1] or d[2] == max(d[0], d[1]))) >= 8 + 4      # ties of the diagonal
    for f in range(len(lrf)):
        qo = ora.rot_quaternion(lrf[f]).astype(f64)
        if decided[f]:
            assert np.abs(qo - q[f]).max() <= 2e-7, f                                         # the same branch
        assert np.abs(ora.rotate_into(lrf[f], v) - into[f] @ v).max() <= TOL_XYZ              # either branch: the same rotation
        assert np.abs(ora.rotate_back(lrf[f], v) - back[f] @ v).max() <= TOL_XYZ
    side = np.array([np.trace(l.reshape(3, 3).astype(f64)) for l in lrf[n_perm:n_perm + 32]])
    assert (side > 0).sum() >= 4 and (side < 0).sum() >= 4 and np.abs(side).max() < 3e-3
    # the 16 perturbed half turns: both sides of each diagonal comparison that is a tie in the unperturbed frame
    first, second = [], []
    for l in lrf[n_perm + 32:]:
        d = np.diag(l.reshape(3, 3).astype(f64))
        base = np.round(d)
        assert d.sum() < 0 and np.abs(d - base).max() < 3e-3
        if base[0] == base[1]:
            first.append(d[1] - d[0])                                   # `m11 > m00`
        else:
            i = 1 if d[1] > d[0] else 0
            assert base[2] == base[i]
            second.append(d[2] - d[i])                                  # `m22 > m[i][i]`
    assert len(first) + len(second) == 16
    for diffs in (first, second):
        assert sum(x > 0 for x in diffs) >= 1 and sum(x < 0 for x in diffs) >= 1 and all(x != 0 for x in diffs), diffs
    for name in ("sigma-l2-33", "sigma-chi2-35", "sigma-l2-1", "sigma-chi2-352"):
        s = sc.scene(name)
        for f in range(0, len(s["desc"]), 7):
            want = ora.distance(s["metric"], s["desc"][f], s["codewords"][f % 40])
            assert abs(want - cr.distance64(s["metric"], s["desc"][f], s["codewords"][f % 40])) <= 1e-6 * max(want, 1e-3)


def measure(ora):
    worst = dict(w=(0.0, ""), xyz=(0.0, ""), sigma=(0.0, ""))
    for name in TRAIN_SCENES:
        ref, want = sc.reference(name), oracle_on(ora, name)
        assert ref["evaluated"].all()
        assert same_kind(want["class_sigma"], ref["class_sigma"]), name
        assert np.array_equal(want["class_sigma"].view(np.uint32)[~np.isnan(want["class_sigma"])],
                              sigma32(ora, sc.scene(name)).view(np.uint32)[~np.isnan(want["class_sigma"])]), name
        s = sc.scene(name)
        if s["oracle_k1"]:                                           # one activation per feature: ismref_class_sigmas takes the scene too
            direct = ora.class_sigmas(s["metric"], s["desc"], s["cls"], s["model"], s["act_idx"], s["desc"] if s["codewords"] is None else s["codewords"],
                                      s["n_classes"])
            assert np.array_equal(direct.view(np.uint32), want["class_sigma"].view(np.uint32)), name
        if "vote_class_weight" in want:
            assert np.array_equal(want["vote_class_weight"].view(np.uint32), ref["vote_class_weight32"].view(np.uint32)), name
        got = dict(w=np.abs(want["vote_weight"] - ref["vote_weight"]).max(initial=0.0), xyz=np.abs(want["vote_xyz"] - ref["vote_xyz"]).max(initial=0.0),
                   sigma=sigma_error(want["class_sigma"], ref["class_sigma"]))
        print(f"{name}: weights {got['w']:.3g}, votes {got['xyz']:.3g}, sigma {got['sigma']:.3g} (relative)")
        for k in worst:
            if got[k] > worst[k][0]:
                worst[k] = (float(got[k]), name)
    return worst


def test_tolerances_are_four_times_the_measured_error(ora):
    worst = measure(ora)
    print("largest:", worst)
    for key, tol in (("w", TOL_W), ("xyz", TOL_XYZ), ("sigma", TOL_SIGMA)):
        assert 4 * worst[key][0] <= tol <= 4.2 * worst[key][0], (key, worst[key], tol)
    assert np.abs(sc.reference("term3")["vote_class_weight"] - sc.reference("term3")["vote_class_weight32"]).max() <= 2e-8


def oracle_votes(ora, flags):
    s = sc.votes_scene()
    got = ora.cast_votes(s["cb"], flags, s["lrf"], s["kp"][:, 0], s["kp"][:, 1], s["kp"][:, 2], s["dense_idx"], s["dense_dist"])
    slots = sc.dense_slots(s)
    return {k: v[slots] for k, v in got.items()}


def weight_close(got, want):
    """float32 cast weights: the bytes of the reference's float32, any NaN where it has a NaN"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    ok = ~np.isnan(want)
    return np.array_equal(np.isnan(got), ~ok) and np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def test_cast_reference_against_the_oracle_and_tol_pos(ora):
    worst = 0.0
    s = sc.votes_scene()
    for flags in range(16):
        ref, want = sc.votes_reference(flags), oracle_votes(ora, flags)
        assert np.array_equal(want["cls"] >= 0, ref["live"])
        for key in ("cls", "inst", "codeword"):
            assert np.array_equal(want[key], ref[key]), (flags, key)
        assert weight_close(want["weight"], ref["weight"]), flags
        assert np.array_equal(want["bbox_size"], ref["bbox_size"])
        assert np.abs(want["bbox_quat"] - ref["bbox_quat"]).max() <= TOL_POS
        worst = max(worst, float(np.abs(want["pos"] - ref["pos"]).max()))
        assert len(ref["live"]) == len(want["cls"]) == len(s["idx"]) * 4                          # n_act * max_votes slots, all of them compared
        assert np.all(ref["pos"][~ref["live"]] == 0) and np.all(want["pos"][~ref["live"]] == 0) and np.all(ref["weight"][~ref["live"]] == 0)
    print("cast positions:", worst)
    assert 4 * worst <= TOL_POS <= 4.2 * worst


# ------------------------------------------------------------------------------------------------------- cap conditions
def test_cast_scene_tells_strict_comparisons_from_lax_ones():
    """`trace >= 0` or `>=` on the diagonal give the same rotation but, at some frames, the NEGATED quaternion, which only the bbox
    quaternion b * q of a live vote shows. The scene must hold such votes for both: a 120-degree turn whose quaternion has w < 0, and
    a frame of trace -1 with a tied diagonal"""
    s, ref = sc.votes_scene(), sc.votes_reference(0)
    half_turn = False
    for variant in ("trace_ge", "diag_ge"):
        flipped = np.zeros(len(s["lrf"]), bool)
        for f, l in enumerate(s["lrf"]):
            q, _ = cr.rot_quaternion(l)
            alt, _ = cr.rot_quaternion(l, **{variant: True})
            same, negated = np.abs(alt - q).max() <= 1e-15, np.abs(alt + q).max() <= 1e-15
            assert same != negated
            flipped[f] = negated
            tr = np.trace(l.reshape(3, 3).astype(f64))
            assert not flipped[f] or (tr == 0 if variant == "trace_ge" else tr in (0, -1))        # a 120-degree turn has all of its diagonal tied
            if variant == "diag_ge" and flipped[f] and tr == -1 and np.diff(s["act_off"])[f] > 0:
                half_turn = True                                                                    # a half turn about a face diagonal casts a vote
        assert variant == "trace_ge" or half_turn
        slots = np.nonzero(ref["live"] & np.repeat(flipped[s["feat_of_act"]], 4))[0]
        print(f"{variant}: {int(flipped.sum())} frames flip, {len(slots)} live votes show it")
        assert flipped.sum() >= 3 and len(slots) >= 3
        b = s["cb"]["vote_bbox_quat"].astype(f64)
        assert np.all(np.abs(ref["bbox_quat"][slots]).max(1) * 2 >= 0.25) and np.all(np.abs(b).max(1) >= 0.25)      # a flip moves an entry by >> TOL_POS
    w = np.array([cr.rot_quaternion(l)[0][0] for l in s["lrf"]])
    tr = np.array([np.trace(l.reshape(3, 3).astype(f64)) for l in s["lrf"]])
    has_vote = np.diff(s["act_off"]) > 0
    assert np.any((tr == 0) & (w < 0) & has_vote) and np.any((tr == 0) & (w > 0) & has_vote)


def test_min_move_of_ranks_and_hub_is_eight_tolerances():
    for name in ("ranks", "hub"):
        ref = sc.reference(name)
        ev = ref["evaluated"]
        mm = ref["min_move"][ev]
        print(f"{name}: {int(ev.sum())} medians evaluated, smallest min_move {mm.min():.3g} = {mm.min() / TOL_W:.1f} TOL_W")
        assert mm.min() >= 8 * TOL_W
        if name == "hub":
            assert int(ev.sum()) >= 256 and ev[0] and ev[-1] and ev[len(ev) // 2] and ev[::cr.SAMPLE_STEP].all()
            assert np.isnan(ref["vote_weight"][~ev]).all() and len(ev) == sc.HUB_M
        else:
            assert ev.all()


def test_boundary_margins_are_zero_or_a_float_step():
    s = sc.votes_scene()
    eps = f32(cr.FLT_EPSILON)
    step_eps = float(eps - np.nextafter(eps, f32(0)))
    seen = dict(on=0, above=0, below=0, eps_on=0, eps_below=0)
    sig = np.array([0.5, np.nan, 0.25, 1.0])
    for flags in range(16):
        ref = sc.votes_reference(flags)
        ms = ref["margin_sigma"]; me = ref["margin_eps"]
        for slot in np.nonzero(~np.isnan(ms))[0]:
            a, v = divmod(int(slot), 4)
            c = int(s["cb"]["vote_class"][int(s["cb"]["vote_offsets"][s["idx"][a]]) + v])
            thr = f32(2 * sig[min(c, 3)])
            assert ms[slot] == 0 or abs(ms[slot]) >= float(thr - np.nextafter(thr, f32(0))), (flags, slot)
            if flags == 0:
                seen["on"] += ms[slot] == 0; seen["above"] += 0 < ms[slot] <= float(np.spacing(thr)); seen["below"] += 0 > ms[slot] >= -float(np.spacing(thr))
        fin = me[~np.isnan(me)]
        assert np.all((fin == 0) | (np.abs(fin) >= step_eps)), flags
        mm = ref["matching_margin"][~np.isnan(ref["matching_margin"])]
        assert (len(mm) > 0) == bool(flags & cr.W_MATCHING) and np.all(mm >= ROUNDING_MARGIN), (flags, mm.min(initial=1.0))
        if flags == cr.W_VOTE:
            seen["eps_on"] += int(np.sum(fin == 0)); seen["eps_below"] += int(np.sum(fin == -step_eps))
    assert seen["on"] >= 3 and seen["above"] >= 3 and seen["below"] >= 3 and seen["eps_on"] == 1 and seen["eps_below"] == 1, seen


def test_every_scene_states_what_it_pins_and_nothing_is_left_out():
    for name in sc.SCENES:
        assert len(sc.scene(name)["pins"]) > 20
    assert len(sc.votes_scene()["pins"]) > 20
    for name in TRAIN_SCENES:
        ref = sc.reference(name)
        assert ref["evaluated"].all() and not np.isnan(ref["vote_weight"]).any() and not np.isnan(ref["vote_xyz"]).any(), name
    # undecided frames are allowed only among the near-tie rotations of `frames`: there are none anywhere else
    for name in TRAIN_SCENES:
        near = sc.reference(name)["near_tie"]
        undecided = (near > 0) & (near < NEAR_TIE)
        assert not undecided.any() or name == "frames", name
        if name == "frames":
            assert not undecided[:sc.scene(name)["n_permutations"]].any()
    near = sc.votes_reference(0)["near_tie"]
    assert not ((near > 0) & (near < NEAR_TIE)).any()


def test_exact_quaternions_give_exact_votes_in_the_reference():
    s, ref = sc.scene("frames"), sc.reference("frames")
    exact = exact_frames(ref)
    assert exact[:24].sum() == 12 and exact[24:].sum() == 0              # identity, the eight 120-degree turns, three half turns about an axis
    xyz = ref["vote_xyz"][np.argsort(ref["vote_feature"])]
    assert np.array_equal(xyz[exact], xyz[exact].astype(f32).astype(f64))
    assert np.array_equal(xyz[exact] * 64, np.round(xyz[exact] * 64))


def exact_frames(ref):
    """frames whose quaternion is dyadic (entries multiples of 1/2, norm 1): the rotation of a dyadic vector is exact in float32"""
    q = ref["quat"]
    return np.all(q * 2 == np.round(q * 2), axis=1) & (np.abs((q * q).sum(1) - 1) == 0)
