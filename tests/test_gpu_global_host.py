"""Global verification through the C++ host (-m gpu): three classes x two small objects trained with SHORT_SHOT_GLOBAL (and once with
SHOT_GLOBAL), written, read back, then detectBatch with each of the seven merge functions in single-object and in detection mode.
What the host returns must equal global_ref.py's host sequence (classifyWithKNN, the merge sequence) applied to the DEVICE's own
maxima, rows and neighbours, which ism3d_last_global hands out: integers exactly, floats to 1e-6 relative (the host's expf, and a
compiler that may fuse a * b + c)."""
import json

import numpy as np
import pytest

import global_host as gh
import global_ref as gr
import host_binding as hb
from test_host_layer import _cfg

pytestmark = pytest.mark.gpu
N_CLASSES, N_TRAIN, N_TEST, N_POINTS = 3, 6, 4, 2048
BANDWIDTH = 0.6
SSG = {"Type": "SHORT_SHOT_GLOBAL", "Parameters": {"ShortShotDims": 32, "ShortShotBinType": "auto"}}
_state = {}


def config(global_features=SSG, **voting):
    j = json.loads(_cfg())
    j["Children"]["GlobalFeatures"] = global_features
    j["Children"]["Voting"]["Parameters"].update(dict(UseGlobalFeatures=True, GlobalFeaturesK=3, Bandwidth=BANDWIDTH))
    j["Children"]["Voting"]["Parameters"].update(voting)
    return j


def trained(pkg, tmp_path_factory, gtype="SHORT_SHOT_GLOBAL"):
    """train once per global type, write the model; -> (directory, training order, train set, test batch)"""
    if gtype not in _state:
        syn = pkg.synthetic
        train = syn.Dataset(N_CLASSES, N_TRAIN, split=0, n_points=N_POINTS, leaf=0.2)
        test = syn.Dataset(N_CLASSES, N_TEST, split=1, n_points=N_POINTS, leaf=0.2)
        order = sorted(range(N_TRAIN), key=lambda i: (train.label(i), i))
        m = hb.Model()
        m.config_from_json(json.dumps(config(SSG if gtype == "SHORT_SHOT_GLOBAL" else {"Type": gtype})))
        for i in order:
            o = train.get(i)
            m.add_training(o["xyz"], o["normals"], o["label"], i)
        m.train()
        d = tmp_path_factory.mktemp("global_" + gtype)
        m.write(str(d / "model.ism"))
        _state[gtype] = (d, order, train, test.batch(range(N_TEST)), gh.global_features(m))
    return _state[gtype]


def variant(d, name, gtype="SHORT_SHOT_GLOBAL", **voting):
    """the written model under other Voting parameters: a second .ism beside the same .ismd"""
    j = {"ObjectConfig": config(SSG if gtype == "SHORT_SHOT_GLOBAL" else {"Type": gtype}, **voting), "ObjectData": "model.ismd"}
    path = str(d / (name + ".ism"))
    open(path, "w").write(json.dumps(j))
    m = hb.Model()
    m.read(path)
    return m


def close(a, b):
    return abs(float(a) - float(b)) <= 1e-6 * max(abs(float(b)), 1e-3)


def check_against_the_restatement(m, nb, stored, fn, single, min_threshold=0.0, best_k=-1, **kw):
    """detect, then redo the host sequence with global_ref on what the device produced; returns (result, dump)"""
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16)
    g = gh.last_global(m)
    n_obj = len(nb["pt_off"]) - 1
    assert len(g["max_off"]) == n_obj + 1
    hyp = {}
    for r in range(len(g["region_obj"])):
        o, mi = int(g["region_obj"][r]), int(g["region_max"][r])
        live = single or int(g["n_sel"][r]) > kw.get("min_points", 500)
        live = live and not np.isnan(g["desc"][r]).any()
        max_cls = 0xffffffff if mi < 0 else int(g["max_cls"][g["max_off"][o] + mi])
        max_inst = 0xffffffff if mi < 0 else int(g["max_inst"][g["max_off"][o] + mi]) & 0xffffffff
        if live:
            idx = g["knn_idx"][r]
            assert (idx >= 0).all() and (np.diff(g["knn_dist"][r]) >= 0).all()
            want = gr.classify_with_knn(stored["cls"][idx], stored["inst"][idx], g["knn_dist"][r], max_cls, single)
        else:
            want = (max_cls, 0.0, max_inst, 0.0)
        have = (int(g["hyp_id"][r, 0]), g["hyp_w"][r, 0], int(g["hyp_id"][r, 1]), g["hyp_w"][r, 1])
        assert (have[0], have[2]) == (want[0] & 0xffffffff, want[2] & 0xffffffff), (r, have, want)
        assert close(have[1], want[1]) and close(have[3], want[3]), (r, have, want)
        hyp[(o, mi)] = (want, g["centroid"][r] if (not single and g["n_sel"][r] > 0) else np.zeros(3, np.float32), int(g["n_sel"][r]))
    for o in range(n_obj):
        a, b = int(g["max_off"][o]), int(g["max_off"][o + 1])
        ms = []
        for i in range(a, b):
            h, roi, _ = hyp[(o, -1)] if single else hyp[(o, i - a)]
            ms.append(gr.Maximum(int(g["max_cls"][i]), g["max_w"][i], int(g["max_inst"][i]), g["max_iw"][i], g["max_pos"][i], h, roi))
        if single and not ms and hyp[(o, -1)][2] > 0:
            h = hyp[(o, -1)][0]
            ms.append(gr.Maximum(h[0], h[1], h[2], 0.0, g["centroid"][[r for r in range(len(g["region_obj"])) if g["region_obj"][r] == o][0]], h))
        want = gr.merge_sequence(ms, fn, BANDWIDTH, min_threshold=min_threshold, best_k=best_k)
        assert int(got["n_total"][o]) == len(want), (fn, single, o)
        for i, w in enumerate(want[:16]):
            assert (int(got["cls"][o, i]), int(got["inst"][o, i])) == (w.cls, w.inst), (fn, single, o, i)
            assert close(got["weight"][o, i], w.weight), (fn, single, o, i, got["weight"][o, i], w.weight)
    return got, g


def test_training_stores_one_global_row_per_cloud(pkg, gpu, tmp_path_factory):
    """class-major, one cloud per training object, its instance id, the region radius and frame; the rows are those of the region entry
    on the same objects (a point on a bin edge may fall either way when the frame's last bits differ with the cloud's cell: 5e-3 of a
    unit row is three points of 2048); write -> read keeps them bit for bit"""
    ctx, dev = gpu
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    assert stored["n_clouds"] == N_TRAIN and stored["cls"].tolist() == [train.label(i) for i in order] and stored["inst"].tolist() == order
    assert stored["desc"].shape == (N_TRAIN, 32) and np.isfinite(stored["desc"]).all() and (stored["radius"] > 0).all()
    assert np.abs(np.linalg.norm(stored["desc"].astype(np.float64), axis=1) - 1).max() < 1e-6
    import torch
    b = train.batch(order)
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (b["xyz"], b["normals"]) for i in range(3)]
    cloud = pkg.capi.Cloud(ctx, b["pt_off"], *t, 0.16)
    try:
        out = pkg.capi.global_short_shot(ctx, cloud, dev, np.arange(N_TRAIN), bins=(2, 2, 8))
        assert np.abs(out["desc"].cpu().numpy() - stored["desc"]).max() < 5e-3
        assert np.array_equal(out["radius"].cpu().numpy(), stored["radius"])
        assert np.abs(out["lrf"].cpu().numpy() - stored["rf"]).max() < 1e-5
    finally:
        cloud.close()
    m2 = variant(d, "reread")
    again = gh.global_features(m2)
    for k in ("cls", "cloud", "inst", "rf", "desc", "radius"):
        assert np.array_equal(again[k], stored[k]), k


@pytest.mark.parametrize("single", [True, False], ids=["single-object", "detection"])
@pytest.mark.parametrize("fn", [1, 2, 3, 4, 5, 6, 7])
def test_detect_batch_matches_the_host_sequence(pkg, gpu, tmp_path_factory, fn, single):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, f"fn{fn}_{int(single)}", GlobalFeatureInfluenceType=fn, SingleObjectMode=single, GlobalFeatureMinPoints=50)
    got, g = check_against_the_restatement(m, nb, stored, fn, single, min_points=50)
    n_obj = len(nb["pt_off"]) - 1
    assert g["k"] == 3 and g["dim"] == 32
    if single:
        assert g["region_obj"].tolist() == list(range(n_obj)) and (g["region_max"] == -1).all()
        assert np.array_equal(g["n_sel"], np.diff(nb["pt_off"]))
    else:
        assert len(g["region_obj"]) == int(g["max_off"][-1]) and (g["region_max"] >= 0).all()
    assert (got["n"] >= 1).all()


def test_threshold_and_best_k_close_the_sequence(pkg, gpu, tmp_path_factory):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, "thr", GlobalFeatureInfluenceType=7, SingleObjectMode=True, MinThreshold=-0.5, BestK=2)
    got, _ = check_against_the_restatement(m, nb, stored, 7, True, min_threshold=-0.5, best_k=2)
    assert (got["n_total"] <= 2).all()


def test_an_object_without_maxima_returns_the_hypothesis(pkg, gpu, tmp_path_factory):
    """MinVotesThreshold above every cluster: no maximum survives, so single-object mode returns the hypothesis alone, at the centroid"""
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, "novotes", GlobalFeatureInfluenceType=3, SingleObjectMode=True, MinVotesThreshold=10000000)
    got, g = check_against_the_restatement(m, nb, stored, 3, True)
    assert int(g["max_off"][-1]) == 0 and (got["n_total"] == 1).all()
    assert got["cls"][:, 0].tolist() == g["hyp_id"][:, 0].tolist() and np.allclose(got["weight"][:, 0], 1.0)
    assert np.abs(got["pos"][:, 0] - g["centroid"]).max() == 0


def test_k_above_the_stored_rows_is_clamped_and_few_points_give_a_zero_hypothesis(pkg, gpu, tmp_path_factory):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, "bigk", GlobalFeaturesK=50, SingleObjectMode=True)
    _, g = check_against_the_restatement(m, nb, stored, 3, True)
    assert g["k"] == N_TRAIN and sorted(g["knn_idx"][0].tolist()) == list(range(N_TRAIN))
    m = variant(d, "fewpoints", GlobalFeatureInfluenceType=4, SingleObjectMode=False, GlobalFeatureMinPoints=1000000)
    got, g = check_against_the_restatement(m, nb, stored, 4, False, min_points=1000000)
    # function 4 zeroes every maximum that lies within Bandwidth / 2 of its region's centroid (the hypothesis keeps the maximum's own
    # class): those are erased, the distant ones stay
    assert (g["hyp_w"] == 0).all() and (got["n_total"] <= np.diff(g["max_off"])).all() and got["n_total"].sum() < int(g["max_off"][-1])


def test_shot_global_route(pkg, gpu, tmp_path_factory):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory, "SHOT_GLOBAL")
    assert stored["desc"].shape == (N_TRAIN, 352) and np.isfinite(stored["desc"]).all()
    m = variant(d, "shot", "SHOT_GLOBAL", GlobalFeatureInfluenceType=3, SingleObjectMode=True)
    _, g = check_against_the_restatement(m, nb, stored, 3, True)
    assert g["dim"] == 352
