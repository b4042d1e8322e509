"""CoSPAIR on the host (no GPU): the float64 interval reference cospair_ref.py against answers worked out by hand, the palette's
colour indices against a hand table, the margins against the measured float32 error, the cap on what the GPU test may leave
undecided, proof that every scene of cospair_scenes.py reaches its decision, and the host layer (header, binding, config, refusals)."""
import json
import os
import re

import numpy as np
import pytest

import cospair_ref as cr
import cospair_scenes as cs
import fpfh_ref as fr
import host_binding as hb
from test_host_layer import _cfg

f32 = np.float32
STEP = np.array([5.0, 0.0, 12.0]) / 128.0


def one(points, normals, rgba, kp, radius, rgb2lab):
    p = f32(points)
    return cr.cospair(rgb2lab, np.uint32([0, len(p)]), p, f32(normals), np.uint32(rgba), np.uint32([0, 1]), f32([kp]), radius)


# ------------------------------------------------------------------------------------------------ hand-derived answers
def test_worked_example(ora):
    """Centre at the origin with normal +z, radius 0.5 (r_l = l / 14), neighbours at k (5, 0, 12) / 128 (|d| = 13 k / 128), k = 1, 3:
    v = d x n / |d x n| = (0, -1, 0), w = n x v = (1, 0, 0), so f2 = -b_y, f1 = atan2(b_x, b_z), f3 = 12/13 (22.62 degrees: bin 1,
    entry 19) for a target normal b, and |cos2| = |5 b_x + 12 b_z| / 13 < 12/13 keeps the centre the source.
      k = 1, |d| = 0.1016: level 2.  b = (0.6, 0.8, 0):  f1 = 90 deg -> (90 + 180) / 40 = 6.75: entry 6; f2 = -0.8: 143.13 / 20 = 7.16: entry 16
      k = 3, |d| = 0.3047: level 5.  b = (-0.8, 0, 0.6): f1 = -53.13 deg -> 126.87 / 40 = 3.17: entry 3; f2 = 0: 90 / 20 = 4.5: entry 13
    Grey 0x808080 (L = 53.6, a = b = 0): l' = 0.536 -> 4, a' = 86.185 / 184.439 = 0.467 -> 4 (entry 13), b' = 107.863 / 202.345 = 0.533
    -> 4 (entry 22). One pair per level: every populated entry is (1 / 1) * l."""
    r = one([[0, 0, 0], STEP, 3 * STEP], [[0, 0, 1], [0.6, 0.8, 0], [-0.8, 0, 0.6]], [0, 0x808080, 0x808080], [0, 0, 0], 0.5, ora.rgb2lab)
    assert r.snap.tolist() == [0] and r.n.tolist() == [[0, 1, 0, 0, 1, 0, 0]] and r.decided_row.all()
    want = np.zeros(cr.DIM, f32)
    want[[54 + 6, 54 + 16, 54 + 19, 54 + 27 + 4, 54 + 27 + 13, 54 + 27 + 22]] = 2
    want[[216 + 3, 216 + 13, 216 + 19, 216 + 27 + 4, 216 + 27 + 13, 216 + 27 + 22]] = 5
    assert np.array_equal(r.want_lo[0], want) and np.array_equal(r.want_hi[0], want)


def test_level_scale():
    """3 pairs in level 2, two of them in one bin: (2 / 3) * 2 in float32; an empty level stays zero; values lie in [0, 7]"""
    assert cr.value(2, 3, 2) == f32(f32(2) / f32(3)) * f32(2) and cr.value(3, 3, 2) == 2 and cr.value(0, 0, 5) == 0
    assert cr.value(7, 7, 7) == 7
    r2 = cr.level_r2(0.875)
    assert r2.tolist() == [(l / 8) ** 2 for l in range(8)]              # r_l = l / 8: every r2_l exact


def test_spill_and_clamp():
    """bin 9 of f1 / f2 (L / a) lands on bin 0 of the next feature, as the reference writes it; bin 9 of f3 (b) and bin -1 of f1 (L)
    leave the 27-entry array and are clamped (deviation 1); bin -1 of the second and third feature stays inside, as written"""
    assert [cr.resolve(0, 9), cr.resolve(9, 9), cr.resolve(18, 9), cr.resolve(18, 10)] == [9, 18, 26, 26]
    assert [cr.resolve(0, -1), cr.resolve(0, -2), cr.resolve(9, -1), cr.resolve(18, -1)] == [0, 0, 8, 17]


# colour -> (L, a, b) of PCL's RGB2CIELAB through its two tables, and the three bins floor(9 x') by hand:
#   l' = L / 100, a' = (a + 86.185) / 184.439, b' = (b + 107.863) / 202.345
PALETTE_TABLE = {
    "black":   ((0.0, 0.0, 0.0), (0, 4, 4)),                # a' = 0.4673, b' = 0.5331
    "white":   ((99.99, 0.0, 0.0), (8, 4, 4)),              # the sXYZ table ends at index 3999: L = 99.99, l' = 0.9999: bin 8, NO spill
    "red":     ((53.226, 80.110, 67.176), (4, 8, 7)),       # a' = 0.9016, b' = 0.8651
    "green":   ((87.729, -86.211, 83.225), (7, -1, 8)),     # a' = -0.00014: bin -1 -> entry 8, L's bin 8, as the reference writes it
    "blue":    ((32.262, 79.308, -107.901), (2, 8, -1)),    # b' = -0.00019: bin -1 -> entry 17, a's bin 8, as the reference writes it
    "cyan":    ((91.111, -48.080, -14.119), (8, 1, 4)),     # a' = 0.2066, b' = 0.4633
    "magenta": ((60.319, 98.256, -60.815), (5, 9, 2)),      # a' = 1.00001: bin 9 -> entry 18, b's bin 0 (spill)
    "yellow":  ((97.136, -21.569, 94.525), (8, 3, 9)),      # b' = 1.00022: bin 9 -> entry 27, outside the array: CLAMPED to 26
    "grey":    ((53.577, 0.0, 0.0), (4, 4, 4)),
}
PALETTE_ENTRIES = {"black": (0, 13, 22), "white": (8, 13, 22), "red": (4, 17, 25), "green": (7, 8, 26), "blue": (2, 17, 17),
                   "cyan": (8, 10, 22), "magenta": (5, 18, 20), "yellow": (8, 12, 26), "grey": (4, 13, 22)}


def test_palette_table(ora):
    for name, rgba in cs.PALETTE:
        lab, bins = PALETTE_TABLE[name]
        assert np.abs(np.array(ora.rgb2lab(rgba)) - lab).max() < 2e-3, name
        by_hand = (int(np.floor(9 * lab[0] / 100)), int(np.floor(9 * (lab[1] + 86.185) / 184.439)), int(np.floor(9 * (lab[2] + 107.863) / 202.345)))
        assert by_hand == bins == cr.colour_bins(ora.rgb2lab, rgba), name
        assert tuple(cr.colour_indices(ora.rgb2lab, [rgba])[0]) == PALETTE_ENTRIES[name], name
    ref = cs.reference("palette", ora.rgb2lab)
    assert ref.n.tolist() == [[0, 0, 0, 0, 0, 0, 9]] and ref.decided_row.all()
    want = np.zeros(cr.BLOCK, np.int64)
    for e in PALETTE_ENTRIES.values():
        np.add.at(want, list(e), 1)
    assert ref.lo[0, 6 * cr.LEVEL + cr.BLOCK:].tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------ margins and the cap
def test_margins_are_four_to_eight_times_the_measured_error():
    worst = dict(c=0.0, ratio=0.0)
    for name in cs.SCENES:
        pt_off, p, n, _, kp_off, kp = cs.arrays(name)
        m = cr.measure(pt_off, p, n, kp_off, kp, cs.scene(name)["radius"])
        print(f"{name}: {m['pairs']} pairs, max |c32 - c64| {m['c']:.3g} at margin EDGE, largest share of a pair's own margin {m['ratio']:.3g}")
        worst = {k: max(worst[k], m[k]) for k in worst}
    assert 4 * worst["c"] <= cr.EDGE <= 8 * worst["c"], worst
    assert abs(worst["c"] - cr.MEASURED_C) <= 0.02 * cr.MEASURED_C
    assert worst["ratio"] < 1                                             # every measured pair lies inside its own margin
    assert (cr.ERR, cr.CATEGORIES) == (fr.ERR, fr.CATEGORIES)


@pytest.mark.parametrize("name", cs.CAPPED)
def test_cap_on_undecided_deposits(ora, name):
    """what the GPU test may leave undecided, from the reference alone: at least 90 % of the rows fully decided, no row with more than
    8 undecided deposits"""
    ref = cs.reference(name, ora.rgb2lab)
    live = ~ref.nan
    share = ref.decided_row[live].mean()
    print(f"{name}: {live.sum()} rows, {share:.3f} fully decided, at most {ref.undecided.max()} undecided deposits in a row, per category {ref.cats.sum(0).tolist()}")
    assert share >= 0.9 and ref.undecided.max() <= 8


# ------------------------------------------------------------------------------------------------ the scenes reach their decisions
def test_shells_scene(ora):
    s, ref = cs.scene("shells"), cs.reference("shells", ora.rgb2lab)
    assert ref.snap.tolist() == s["want_snap"] and ref.n[0].tolist() == s["want_levels"][0]
    p = s["objs"][0][0]
    d2 = (p.astype(np.float64) ** 2).sum(1)
    assert sorted(set(np.sqrt(d2[5:]) * 8)) == [1, 2, 4, 6, 7]          # exactly on r_1, r_2, r_4, r_6, r_7
    geo = ref.lo[0].reshape(cr.LEVELS, 2, cr.BLOCK)[:, 0]
    assert geo[0, 4] >= 2 and geo[0, 13] >= 2 and geo[0, 22] >= 2        # the two coincident duplicates: 4 / 4 / 4, decided
    assert not ref.want_hi[0, 3 * cr.LEVEL:4 * cr.LEVEL].any() and ref.want_lo[0, 4 * cr.LEVEL:5 * cr.LEVEL].any()   # the empty level 4


def test_queue_uniform_and_thin_scenes(ora):
    assert cs.reference("queue", ora.rgb2lab).n.sum(1).tolist() == cs.QUEUE_PAIRS
    u = cs.reference("uniform", ora.rgb2lab)
    assert u.n.sum() >= 4000 and len(set(cs.scene("uniform")["rgba"][0].tolist())) == 1
    col = u.lo[0].reshape(cr.LEVELS, 2, cr.BLOCK)[:, 1]
    assert ((col > 0).sum(1) == 3).all() and np.array_equal(col.sum(1), 3 * u.n[0])     # three counters per level take every colour deposit
    s, t = cs.scene("thin"), cs.reference("thin", ora.rgb2lab)
    assert len(s["objs"]) == 9 and [len(k) for k in s["kps"]] == [1, 6, 0, 1, 2, 3, 4, 7, 9]
    assert t.nan.nonzero()[0].tolist() == s["nan_rows"] and t.n[s["big_row"]].sum() >= 50000
    assert t.n[s["single_row"]].sum() == 0 and t.snap[s["single_row"]] == 0 and not t.want_hi[s["single_row"]].any()
    bp, bn = s["objs"][4]
    d2 = ((bp.astype(np.float64) - bp[8]) ** 2).sum(1)
    row = s["nan_neighbour_row"]
    assert t.snap[row] == 8 and d2[7] < (s["radius"] / 7) ** 2 and np.isnan(bn[7]).all()   # the NaN-normal point lies in level 1 of that row ...
    assert t.n[row, 0] == ((d2 < (s["radius"] / 7) ** 2).sum() - 2)                        # ... and is not counted (nor is the centre)


def test_hard_scenes(ora):
    """the hand-derived entries of `hard` are candidates of the reference, and the float32 sequence lands on them; the imported FPFH
    constructions reach the seam, swap-tie, pole and degenerate categories"""
    s, ref = cs.scene("hard"), cs.reference("hard", ora.rgb2lab)
    for (o, level), want in s["want"].items():
        hi = ref.hi[o].reshape(cr.LEVELS, 2, cr.BLOCK)[level, 0]
        assert all(hi[i] >= c for i, c in want.items()), (o, level)
    p, n = s["objs"][0]
    c32 = cr.c_float32(p, n, np.zeros(3, np.int64), np.arange(1, 4))["c"]
    assert np.floor(c32).astype(int).tolist() == [[9, 6, 1], [4, 9, 1], [4, 0, 1]]       # f1 = +pi and f2 = -1 reach bin 9: the spills
    cats = {name: cs.reference(name, ora.rgb2lab).cats.sum(0) for name in ("hard", "hard_seam", "hard_swap", "hard_pole")}
    assert cats["hard_seam"][fr.SEAM_C] > 0 and cats["hard_swap"][fr.SWAP_C] > 0
    assert cats["hard_pole"][fr.POLE_C] > 0 and cats["hard_pole"][fr.DEG_C] > 0 and cats["hard"][fr.DEG_C] > 0


# ------------------------------------------------------------------------------------------------ host layer
def test_header_and_binding(pkg):
    h = open(os.path.join(hb.ROOT, "include", "ismhip.h")).read()
    assert re.search(r"int\s+ismhip_cospair\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, const uint32_t\* kp_offsets_h,", h)
    for name, v in (("LEVELS", 7), ("BINS", 9), ("DIM", 378)):
        assert re.search(rf"#define ISMHIP_COSPAIR_{name}\s+{v}\b", h)
    assert "ismhip_cospair" in pkg.capi.EXPORTS and pkg.capi.COSPAIR_DIM == cr.DIM == cr.LEVELS * 2 * 3 * cr.BINS
    assert pkg.pipeline.IsmConfig(n_classes=3, feature="CoSPAIR").dim == 378


def _cospair_cfg(**params):
    p = {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}
    p.update(params)
    return _cfg(**{"Children/Features": {"Type": "CoSPAIR", "Parameters": p}})


def test_host_reads_the_example_config():
    src = json.load(open(os.path.join(hb.ROOT, "config", "kinect_cospair.ism")))["ObjectConfig"]
    m = hb.Model()
    m.config_from_json(json.dumps(src))
    out = json.loads(m.config_to_json())["Children"]["Features"]
    assert out["Type"] == "CoSPAIR" and out["Parameters"]["Radius"] == pytest.approx(0.05)
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())                        # what we write, we read
    assert json.loads(m2.config_to_json())["Children"]["Features"] == out
    m.close(); m2.close()
    other = json.load(open(os.path.join(hb.ROOT, "config", "kinect_cshot.ism")))["ObjectConfig"]
    for j in (src, other):                                         # the value set of kinect_cshot.ism, the feature type apart
        del j["Children"]["Features"]["Type"]
    assert src == other
    m = hb.Model()
    m.config_from_json(_cospair_cfg())                             # Radius not given: the reference's default 0.1
    assert json.loads(m.config_to_json())["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.1)
    m.close()


def test_host_refuses_a_colourless_cloud_and_still_refuses_pfh():
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(200, 3)).astype(f32)
    nrm = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(f32)
    m = hb.Model()
    m.config_from_json(_cospair_cfg(Radius=0.3))
    m.add_training(xyz, nrm, 0, 0)
    with pytest.raises(hb.HostError, match="CoSPAIR needs coloured point clouds"):
        m.train()
    with pytest.raises(hb.HostError, match="CoSPAIR needs coloured point clouds"):
        m.detect_batch(np.uint32([0, 200]), xyz, nrm, max_maxima=4)
    m.close()
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: .*CoSPAIR\)"):
        m.config_from_json(_cfg(**{"Children/Features/Type": "PFH"}))
    m.close()
