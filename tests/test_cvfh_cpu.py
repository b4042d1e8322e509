"""The CVFH global descriptor on the host (no GPU): the restatement cvfh_ref.py against hand-derived answers, the scenes of
cvfh_scenes.py against the zero-undecided condition and the 1 % cap, the host type "CVFH" with its three parameters, the declarations
and bindings, stored rows with SEVERAL rows per training cloud through the data file, and classifyWithKNN over the concatenated
neighbours of a two-row region.

Before the feature these fail: the host type (a pass-through child without a length: UseGlobalFeatures refuses it), the defaults, the
refusal's list, the shipped configuration, the header and the exports, the several-rows setter. The restatement's own tests and the
classifier test hold on either side: they pin the reference the GPU tests use."""
import json
import os

import numpy as np
import pytest

import cvfh_host as ch
import cvfh_ref as cr
import cvfh_scenes as cs
import global_host as gh
import host_binding as hb
from test_host_layer import _BoostReader, _cfg, _toy_codebook

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in cs.all_cases()}
DEFAULTS = {"CvfhClusterTolerance": 0.015, "CvfhNormalRadius": 0.015, "CvfhMinPoints": 50}


def gcfg(global_features, features=None, **voting):
    j = json.loads(_cfg())
    if global_features is not None:
        j["Children"]["GlobalFeatures"] = global_features
    if features is not None:
        j["Children"]["Features"] = features
    j["Children"]["Voting"]["Parameters"].update(voting)
    return json.dumps(j)


# ---- the restatement on the hand-derived scenes ----------------------------------------------------------------------------------------

def sizes(ref):
    return [(c["root"], c["size"]) for c in ref["clusters"]]


def test_hand_derived_clusters():
    """a lattice plane: one cluster; two coplanar patches further apart than the tolerance: two, in index order (the object is shuffled:
    the roots are the smallest original indices, 0 and 1 here by the seed); 29 points dropped, exactly 30 kept; sparse points and small
    patches: the fallback row over all selected points, NaN normals left out of its mean; an empty region: no row"""
    refs = cs.reference(CASES["hand"])
    assert sizes(refs[0]) == [(0, 120)] and (refs[0]["labels"] == 0).all()
    assert [s for _, s in sizes(refs[1])] == [64, 64] and refs[1]["clusters"][0]["root"] < refs[1]["clusters"][1]["root"]
    assert sizes(refs[2]) == [(0, 30), (59, 50)]
    lab = refs[2]["labels"]
    assert (lab[:30] == 0).all() and (lab[30:59] == 30).all() and (lab[59:] == 59).all()       # the 29 are a component, not a cluster
    assert refs[3]["fallback"] and sizes(refs[3]) == [(cr.NONE, 120)]
    fb = refs[3]["clusters"][0]
    assert np.array_equal(fb["normal"], [0, 0, -1]) and np.allclose(fb["centroid"], CASES["hand"]["objs"][3][0].astype(f64).mean(0))
    assert refs[3]["labels"][3] == 3 and refs[3]["labels"][17] == 17                            # a NaN normal: a component of its own
    assert [s for _, s in sizes(refs[4])] == [64]                                               # the ball holds one patch only
    assert refs[5]["fallback"] and len(refs[5]["sel"]) < cs.MIN_POINTS
    assert len(refs[6]["sel"]) == 0 and refs[6]["clusters"] == [] and not refs[6]["fallback"]
    assert refs[7]["fallback"] and len(refs[7]["sel"]) == 28


def test_cylinder_lattices():
    """6 degree steps: ONE cluster over 306 degrees although its ends' normals are 54 degrees from opposite (growing against a seed or
    a mean normal would split it); 14 degree steps: only axial neighbours link, every line of at least 30 points is a cluster, in the
    order of its smallest original index"""
    refs = cs.reference(CASES["cylinders"])
    assert sizes(refs[0]) == [(0, 312)]
    n = CASES["cylinders"]["objs"][0][1].astype(f64)
    assert (n @ n.T).min() < -0.99
    got = sizes(refs[1])
    assert sorted(s for _, s in got) == sorted(k for k in cs.CYL14_LENGTHS if k >= cs.MIN_POINTS) and len(got) == 7
    assert [r for r, _ in got] == sorted(r for r, _ in got)
    assert len(np.unique(refs[1]["labels"])) == len(cs.CYL14_LENGTHS)


def test_crease_and_many():
    """analytic normals: exactly the two planes; re-estimated normals: the points within the normal radius of the crease get mixed
    normals and fall out, two smaller clusters stay. Six patches against four row slots: six clusters"""
    assert [s for _, s in sizes(cs.reference(CASES["crease"])[0])] == [72, 64]
    est = cs.reference(CASES["crease-estimated"])[0]
    assert est["estimated"] and len(est["clusters"]) == 2 and sum(c["size"] for c in est["clusters"]) < 136
    assert est["clusters"][0]["size"] <= 72 and est["clusters"][1]["size"] <= 64
    assert [len(r["clusters"]) for r in cs.reference(CASES["many"])] == [6, 5, 4]
    assert CASES["many"]["max_rows"] == 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_scenes_have_no_undecided_link_and_every_scene_keeps_the_deposit_cap(name):
    case = CASES[name]
    deposits = undecided = 0
    for (o, c, r), ref in zip(case["regions"], cs.reference(case)):
        if case["exact"]:
            assert ref["n_undecided"] == 0 and np.array_equal(ref["labels"], ref["labels_loose"]), (name, o)
        P, N = case["objs"][o]
        for cl in ref["clusters"]:
            if not np.isfinite(cl["normal"]).all():
                continue
            out = cr.row_counts(P[ref["sel"]], N[ref["sel"]], cl["centroid"].astype(f32), cl["normal"].astype(f32))
            assert (out["lower"] <= out["counts"]).all() and (out["counts"] <= out["upper"]).all()
            deposits += out["m"]; undecided += out["undecided"]
    print(f"{name}: {deposits} depositing points over all rows, {undecided} undecided")
    assert undecided <= 0.01 * deposits


def test_the_batches_are_small_and_ragged():
    for case in CASES.values():
        n = [len(p) for p, _ in case["objs"]]
        assert 3 <= len(n) <= 4 and len(set(n)) > 1 and all(100 <= k <= 700 for k in n), (case["name"], n)


# ---- the host type -----------------------------------------------------------------------------------------------------------------------

def test_the_host_accepts_cvfh_with_global_features_and_reports_308():
    m = hb.Model()
    m.config_from_json(gcfg(ch.CVFH, UseGlobalFeatures=True))
    assert hb.lib().ism3d_global_descriptor_length(m.h) == 308
    out = json.loads(m.config_to_json())
    assert out["Children"]["GlobalFeatures"] == ch.CVFH and out["Children"]["Voting"]["Parameters"]["UseGlobalFeatures"] is True
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())
    assert json.loads(m2.config_to_json()) == out


def test_missing_parameters_get_pcls_defaults():
    m = hb.Model()
    m.config_from_json(gcfg({"Type": "CVFH"}, UseGlobalFeatures=True))
    assert json.loads(m.config_to_json())["Children"]["GlobalFeatures"] in ({"Type": "CVFH"}, {"Type": "CVFH", "Parameters": DEFAULTS})
    text = open(os.path.join(ROOT, "point-cloud-donkey_amd", "host", "ism3d.cpp")).read()
    for key, value in DEFAULTS.items():
        assert f'"{key}", {value}' in text


def test_ourcvfh_is_refused_and_the_message_lists_cvfh():
    with pytest.raises(hb.HostError) as e:
        hb.Model().config_from_json(gcfg({"Type": "OURCVFH"}, UseGlobalFeatures=True))
    assert '"OURCVFH"' in str(e.value) and "SHORT_SHOT_GLOBAL, SHOT_GLOBAL, VFH, GASD, CVFH" in str(e.value)
    hb.Model().config_from_json(gcfg({"Type": "OURCVFH"}))                              # without UseGlobalFeatures: a pass-through, as before


def test_cvfh_as_the_local_features_child_is_still_refused():
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path"):
        hb.Model().config_from_json(gcfg(None, features={"Type": "CVFH", "Parameters": {}}))


def test_the_shipped_config_loads_and_differs_from_the_vfh_one_in_the_child_only():
    j = json.load(open(os.path.join(ROOT, "config", "modelnet10_shot_cvfh.ism")))["ObjectConfig"]
    v = json.load(open(os.path.join(ROOT, "config", "modelnet10_shot_vfh.ism")))["ObjectConfig"]
    child = j["Children"]["GlobalFeatures"]
    assert child["Type"] == "CVFH" and set(child["Parameters"]) == set(DEFAULTS)
    v["Children"]["GlobalFeatures"] = child
    assert j == v
    m = hb.Model()
    m.config_from_json(json.dumps(j))
    assert hb.lib().ism3d_global_descriptor_length(m.h) == 308


def test_the_entry_is_declared_and_exported_and_the_abi_version_stays(pkg):
    text = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert "int  ismhip_global_cvfh(" in text and '"global_cvfh"' in text and "features/features_cvfh.cpp" in text
    assert "#define ISMHIP_ABI_VERSION 4" in text
    L = pkg.capi.lib()
    assert "ismhip_global_cvfh" in pkg.capi.EXPORTS and L.ismhip_global_cvfh is not None and callable(pkg.capi.global_cvfh)
    assert L.ismhip_abi_version() == 4


# ---- several rows per training cloud through the data file ---------------------------------------------------------------------------------

def test_two_and_three_rows_per_object_round_trip_through_the_data_file(tmp_path):
    """Voting::iSaveData's field order: classes; per class id and clouds; per cloud its rows; per row frame, descriptor, radius, instance"""
    rng = np.random.default_rng(25)
    cb = _toy_codebook(rng)
    cls, cloud, inst = [0, 0, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 2, 2], [4, 4, 5, 5, 5, 6, 6]      # clouds of 2, 3 and 2 rows
    rf = np.zeros((7, 9), f32); desc = (rng.integers(0, 2000, (7, 308)).astype(f32) / cr.NORM).astype(f32); radius = f32([.5, .5, .7, .7, .7, .9, .9])
    m = hb.Model()
    m.config_from_json(gcfg(ch.CVFH, UseGlobalFeatures=True))
    m.set_codebook(cb, 3)
    m.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    ch.set_global_features(m, cls, cloud, inst, rf, desc, radius)
    path = str(tmp_path / "g.ism")
    m.write(path)
    data = open(str(tmp_path / "g.ismd"), "rb").read()
    m0 = hb.Model()
    m0.config_from_json(gcfg(ch.CVFH))
    m0.set_codebook(cb, 3)
    m0.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    m0.write(str(tmp_path / "g0.ism"))
    at = len(open(str(tmp_path / "g0.ismd"), "rb").read()) - 12                    # where the global features start
    r = _BoostReader(data)
    r.o = at
    assert r.u() == 2
    k = 0
    for c, clouds in ((0, [2]), (1, [3, 2])):
        assert (r.u(), r.u()) == (c, len(clouds))
        for rows in clouds:
            assert r.u() == rows
            for _ in range(rows):
                assert [r.f() for _ in range(9)] == [0.0] * 9
                row = r.vf()
                assert len(row) == 308 and np.array_equal(row, desc[k])
                assert r.f() == radius[k] and r.u() == inst[k]
                k += 1
    assert k == 7
    m2 = hb.Model()
    m2.read(path)
    g = gh.global_features(m2)
    assert g["n_clouds"] == 3 and g["cloud"].tolist() == cloud and g["cls"].tolist() == cls and g["inst"].tolist() == inst
    assert np.array_equal(g["desc"], desc) and np.array_equal(g["radius"], radius)


# ---- the classifier over the concatenated neighbours of a two-row region ------------------------------------------------------------------------

@pytest.mark.parametrize("single", [True, False], ids=["single-object", "detection"])
def test_classify_with_knn_over_two_rows_equals_the_direct_restatement(single):
    """the host concatenates the neighbours of a region's rows in row order and calls classifyWithKNN once: the reference's loop feeds
    one accumulator row after row, so the float sums see the same sequence"""
    rng = np.random.default_rng(31)
    stored_cls = rng.integers(0, 3, 40).astype(np.uint32); stored_inst = (stored_cls * 10 + rng.integers(0, 3, 40)).astype(np.uint32)
    for trial in range(20):
        idx = rng.integers(0, 40, (2, 3))
        dist = np.sort(rng.random((2, 3)).astype(f32) * 4, axis=1)
        max_class = int(rng.integers(0, 4))
        want = ch.classify_rows(stored_cls, stored_inst, idx, dist, max_class, single)
        have = gh.classify_knn(stored_cls[idx.ravel()], stored_inst[idx.ravel()], dist.ravel(), max_class, single)
        assert have[0] == want[0], (trial, have, want)
        assert abs(have[1] - want[1]) <= 1e-6 * max(want[1], 1e-3)
        if want[1] > 0:
            assert have[2] == want[2] and abs(have[3] - want[3]) <= 1e-6 * max(want[3], 1e-3)
