"""Global verification with GlobalFeatures type "CVFH" through the C++ host (-m gpu): three classes x two objects of 2 048 points trained,
written, read back, then detectBatch in single-object and in detection mode. Training stores as many rows per object as the device
reports clusters; detection searches ALL rows of all regions at once and classifies each region on the concatenated neighbours of its
rows: the hypotheses must equal cvfh_host.classify_rows, a direct restatement of global_classifier.cpp:242-347, on the dumped
neighbours (integers exactly, floats to 1e-6 relative: the host's expf).

A model trained with CVFH is refused under another global type only if the row lengths differ. VFH's rows are 308 floats as well, so a
CVFH model RUNS under a VFH configuration; the last test states that."""
import json

import numpy as np
import pytest

import cvfh_host as ch
import global_host as gh
import host_binding as hb
from test_gpu_global_host import N_CLASSES, N_POINTS, N_TEST, N_TRAIN, close, config

pytestmark = pytest.mark.gpu
P = ch.CVFH["Parameters"]
_state = {}


def trained(pkg, tmp_path_factory):
    if not _state:
        syn = pkg.synthetic
        train = syn.Dataset(N_CLASSES, N_TRAIN, split=0, n_points=N_POINTS, leaf=0.2)
        test = syn.Dataset(N_CLASSES, N_TEST, split=1, n_points=N_POINTS, leaf=0.2)
        order = sorted(range(N_TRAIN), key=lambda i: (train.label(i), i))
        m = hb.Model()
        m.config_from_json(json.dumps(config(ch.CVFH)))
        for i in order:
            o = train.get(i)
            m.add_training(o["xyz"], o["normals"], o["label"], i)
        m.train()
        d = tmp_path_factory.mktemp("global_cvfh")
        m.write(str(d / "model.ism"))
        _state["v"] = (d, order, train, test.batch(range(N_TEST)), gh.global_features(m))
    return _state["v"]


def variant(d, name, child=ch.CVFH, **voting):
    path = str(d / (name + ".ism"))
    open(path, "w").write(json.dumps({"ObjectConfig": config(child, **voting), "ObjectData": "model.ismd"}))
    m = hb.Model()
    m.read(path)
    return m


def test_training_stores_as_many_rows_per_object_as_the_device_reports_clusters(pkg, gpu, tmp_path_factory):
    import torch
    ctx, dev = gpu
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    b = train.batch(order)
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (b["xyz"], b["normals"]) for i in range(3)]
    cloud = pkg.capi.Cloud(ctx, b["pt_off"], *t, 0.16)
    try:
        out = pkg.capi.global_cvfh(ctx, cloud, dev, np.arange(N_TRAIN), cluster_tolerance=P["CvfhClusterTolerance"], normal_radius=P["CvfhNormalRadius"],
                                   min_points=P["CvfhMinPoints"], max_rows=16)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        cloud.close()
    ncl = out["n_clusters"]
    print("rows per training object:", ncl.tolist())
    assert (ncl >= 1).all() and ncl.max() > 1 and ncl.max() <= 16
    assert stored["n_clouds"] == N_TRAIN and np.bincount(stored["cloud"], minlength=N_TRAIN).tolist() == ncl.tolist()
    assert stored["cls"].tolist() == [train.label(i) for i, n in zip(order, ncl) for _ in range(n)]
    assert stored["inst"].tolist() == [i for i, n in zip(order, ncl) for _ in range(n)]
    assert stored["desc"].shape == (int(ncl.sum()), 308) and np.isfinite(stored["desc"]).all() and (stored["rf"] == 0).all()
    assert np.array_equal(stored["radius"], np.repeat(out["radius"], ncl))                     # the cloud's radius on every row
    rows = np.concatenate([out["desc"][o, :ncl[o]] for o in range(N_TRAIN)])
    # the clusters do not depend on the cloud's cell size, the rows' deposits on the last bits of nothing but the points themselves:
    # the same counts; allow three deposits per bin as the other global types' host tests do
    assert np.abs(rows - stored["desc"]).max() <= 3.0 / 47278.0 + 1e-9
    again = gh.global_features(variant(d, "reread"))
    for k in ("cls", "cloud", "inst", "rf", "desc", "radius"):
        assert np.array_equal(again[k], stored[k]), k


@pytest.mark.parametrize("single", [True, False], ids=["single-object", "detection"])
def test_detect_batch_classifies_each_region_on_all_its_rows(pkg, gpu, tmp_path_factory, single):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, f"cvfh_{int(single)}", GlobalFeatureInfluenceType=3, SingleObjectMode=single, GlobalFeatureMinPoints=50)
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16)
    g = ch.last_global(m)
    n_obj = len(nb["pt_off"]) - 1
    R = len(g["region_obj"])
    assert g["k"] == 3 and g["dim"] == 308 and len(g["row_off"]) == R + 1 and g["row_off"][0] == 0 and (np.diff(g["row_off"].astype(np.int64)) >= 0).all()
    assert g["desc"].shape[0] == int(g["row_off"][-1])
    if single:
        assert g["region_obj"].tolist() == list(range(n_obj)) and (g["region_max"] == -1).all()
        assert (np.diff(g["row_off"].astype(np.int64)) >= 1).all() and np.diff(g["row_off"].astype(np.int64)).max() > 1
    else:
        assert R == int(g["max_off"][-1]) and (g["region_max"] >= 0).all()
    for r in range(R):
        o, mi = int(g["region_obj"][r]), int(g["region_max"][r])
        rows = np.arange(int(g["row_off"][r]), int(g["row_off"][r + 1]))
        enough = single or int(g["n_sel"][r]) > 50
        rows = [t for t in rows if enough and not np.isnan(g["desc"][t]).any()]
        max_cls = 0xffffffff if mi < 0 else int(g["max_cls"][g["max_off"][o] + mi])
        max_inst = 0xffffffff if mi < 0 else int(g["max_inst"][g["max_off"][o] + mi]) & 0xffffffff
        have = (int(g["hyp_id"][r, 0]), g["hyp_w"][r, 0], int(g["hyp_id"][r, 1]), g["hyp_w"][r, 1])
        if rows:
            assert (g["knn_idx"][rows] >= 0).all()
            want = ch.classify_rows(stored["cls"], stored["inst"], g["knn_idx"][rows], g["knn_dist"][rows], max_cls, single)
        else:
            want = (max_cls, 0.0, max_inst, 0.0)
        assert have[0] == want[0] & 0xffffffff and close(have[1], want[1]), (r, have, want)
        if want[1] > 0 or not rows:
            assert have[2] == want[2] & 0xffffffff and close(have[3], want[3]), (r, have, want)
    assert (got["n"] >= 1).all()


def test_a_cvfh_model_runs_under_a_vfh_config_because_the_lengths_are_equal(pkg, gpu, tmp_path_factory):
    """the host refuses stored rows under another global type only when their LENGTH differs from the configured type's; VFH and CVFH
    rows are 308 floats both, so this runs (every region then has one query row); under SHOT_GLOBAL (352) it is refused"""
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, "as_vfh", {"Type": "VFH"}, SingleObjectMode=True)
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16)
    g = ch.last_global(m)
    assert g["dim"] == 308 and np.diff(g["row_off"].astype(np.int64)).tolist() == [1] * (len(nb["pt_off"]) - 1) and (got["n"] >= 1).all()
    m = variant(d, "as_shot", {"Type": "SHOT_GLOBAL"}, SingleObjectMode=True)
    with pytest.raises(hb.HostError, match="308 dimensions, the configured GlobalFeatures type 352"):
        m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16)
