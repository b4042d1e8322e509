"""Feature ranking through the C++ host mirror (libism3d_amd.so): train() with a FeatureWeighting type keeps exactly the features the
numpy transcription of the reference (ranking_ref.py) keeps, computed from the features of a Uniform run on the same objects."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import host_binding as hb
import ranking_ref as ref
import ranking_scenes as scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
KEYS = ("desc", "lrf", "kp", "cls", "model", "center")
_cache = {}


def _last_features(m):
    """the host's features of its last train()"""
    L, P = m.L, hb._p
    dim, nobj = C.c_int(), C.c_int()
    n = L.ism3d_last_features(m.h, 0, C.byref(dim), C.byref(nobj), *([None] * 8))
    assert n >= 0
    d = dim.value
    out = dict(off=np.zeros(max(nobj.value, 0) + 1, np.uint32), desc=np.zeros((n, d), np.float32), lrf=np.zeros((n, 9), np.float32),
               kp=np.zeros((n, 3), np.float32), cls=np.zeros(n, np.uint32), model=np.zeros(n, np.uint32), center=np.zeros((n, 3), np.float32))
    assert L.ism3d_last_features(m.h, 0, None, None, *[P(out[k]) for k in ("off",) + KEYS]) == n
    return out


def _counter(m, name):
    v = C.c_double(-1.0)
    assert m.L.ism3d_device_timer(m.h, name.encode(), C.byref(v)) == 0
    return v.value


def _trained(pkg, fw):
    train = pkg.synthetic.Dataset(3, 6, split=0, n_points=2048, n_keypoints=128)
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["FeatureWeighting"] = fw
    j["Children"]["Clustering"] = {"Type": "None"}
    m = hb.Model()
    m.config_from_json(json.dumps(j))
    for i in sorted(range(6), key=lambda i: (train.label(i), i)):
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    return m


def _uniform(pkg):
    """the Uniform run, once: its training features, class ranges and counters"""
    if "uniform" not in _cache:
        m = _trained(pkg, {"Type": "Uniform"})
        tf = _last_features(m)
        off = np.concatenate([[0], np.cumsum(np.bincount(tf["cls"], minlength=3))]).astype(np.uint32)
        _cache["uniform"] = dict(tf=tf, off=off, size=m.codebook_size(), launches=_counter(m, "rank_launches"))
        m.close()
    return _cache["uniform"]


def test_uniform_launches_no_ranking(pkg, gpu):
    u = _uniform(pkg)
    assert u["launches"] == 0
    assert len(u["tf"]["desc"]) > 300 and (np.diff(u["off"]) > 20).all()
    assert u["size"] == len(u["tf"]["desc"])


@pytest.mark.parametrize("rank_type,params", [("KNNActivation", {"ScoreIncrementType": 2}), ("Incremental", {"ExtractOffset": 0.125}),
                                              ("Strangeness", {"Factor": 0.5}), ("NaiveBayes", {"ExtractFromList": "back"})],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_ranked_training_keeps_the_reference_rows(pkg, gpu, ora, rank_type, params):
    u = _uniform(pkg)
    tf, off = u["tf"], u["off"]
    params = dict({"KSearch": 10, "Factor": 0.75, "ExtractOffset": 0.0, "ExtractFromList": "invalid"}, **params)
    if rank_type == "NaiveBayes":
        _, dist = ora.knn(ref.CHI2, tf["desc"], tf["desc"], 11)
        params["DistanceThreshold"] = scenes.bayes_threshold(dist)
    m = _trained(pkg, {"Type": rank_type, "Parameters": params})
    rf = _last_features(m)
    # the reference's mask from the Uniform run's rows (chi-square searches although the model's DistanceType is Euclidean)
    score = ref.scores(ora.knn, rank_type, tf["desc"], off, params["KSearch"], params.get("DistanceThreshold", 0.1), params.get("ScoreIncrementType", 0))
    offset = ref.extract_offset_from_list(params["ExtractFromList"], params["Factor"], params["ExtractOffset"])
    keep, n_keep = ref.select(score, off, params["Factor"], offset)
    keep = keep.astype(bool)
    assert 0 < keep.sum() < len(keep)
    assert len(rf["desc"]) == keep.sum()
    for k in KEYS:
        assert np.array_equal(rf[k], tf[k][keep], equal_nan=True) if rf[k].dtype.kind == "f" else np.array_equal(rf[k], tf[k][keep]), k
    assert m.codebook_size() == int(n_keep.sum())
    assert _counter(m, "rank_launches") == 2
    m.close()
