"""ActivationStrategy "Threshold" in the C++ host mirror (libism3d_amd.so): the factory builds it and the configuration round-trips
on the CPU; on the GPU a Threshold model trains and detects end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import host_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")


def _threshold_cfg(threshold=None):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Codebook"]["Children"]["ActivationStrategy"] = {"Type": "Threshold", "Parameters": {} if threshold is None else {"Threshold": threshold}}
    return json.dumps(j)


def test_threshold_activation_config_loads_and_round_trips():
    m = hb.Model()
    m.config_from_json(_threshold_cfg(0.35))
    out = json.loads(m.config_to_json())["Children"]["Codebook"]["Children"]["ActivationStrategy"]
    assert out["Type"] == "Threshold"
    assert out["Parameters"]["Threshold"] == pytest.approx(0.35)
    assert out["Parameters"]["UseDistanceRatio"] is False            # inherited base parameters (activation_strategy.cpp:16-22)
    assert out["Parameters"]["DistanceRatioThreshold"] == pytest.approx(0.95)
    m.close()
    m = hb.Model()
    m.config_from_json(_threshold_cfg())
    assert json.loads(m.config_to_json())["Children"]["Codebook"]["Children"]["ActivationStrategy"]["Parameters"]["Threshold"] == pytest.approx(1.0)
    m.close()


def test_unknown_activation_strategy_lists_threshold_as_built():
    m = hb.Model()
    j = json.loads(_threshold_cfg())
    j["Children"]["Codebook"]["Children"]["ActivationStrategy"]["Type"] = "INN"
    with pytest.raises(Exception, match="built: KNN, KNNRule, Threshold"):
        m.config_from_json(json.dumps(j))
    m.close()


def _last_features(m, which, n_obj=None):
    """the host's features of its last train() (which = 0) / detectBatch() (which = 1)"""
    L, P = m.L, hb._p
    dim, nobj = C.c_int(), C.c_int()
    n = L.ism3d_last_features(m.h, which, C.byref(dim), C.byref(nobj), *([None] * 8))
    assert n >= 0, hb.Model.__name__
    d = dim.value
    out = dict(off=np.zeros(max(nobj.value, 0) + 1, np.uint32), desc=np.zeros((n, d), np.float32), lrf=np.zeros((n, 9), np.float32),
               kp=np.zeros((n, 3), np.float32), cls=np.zeros(n, np.uint32), model=np.zeros(n, np.uint32), center=np.zeros((n, 3), np.float32))
    assert L.ism3d_last_features(m.h, which, None, None, *[P(out[k]) for k in ("off", "desc", "lrf", "kp", "cls", "model", "center")]) == n
    return out


def _last_votes(m, n_obj):
    L, P = m.L, hb._p
    ns = L.ism3d_last_votes(m.h, None, None, None, None, None)
    assert ns >= 0
    v = dict(slot_off=np.zeros(n_obj + 1, np.uint32), pos=np.zeros((ns, 3), np.float32), weight=np.zeros(ns, np.float32),
             cls=np.zeros(ns, np.int32), inst=np.zeros(ns, np.int32))
    assert L.ism3d_last_votes(m.h, *[P(v[k]) for k in ("slot_off", "pos", "weight", "cls", "inst")]) == ns
    return v


@pytest.mark.gpu
def test_host_threshold_train_and_detect(pkg, gpu, ora):
    """Threshold through libism3d_amd.so against an independent path on the host's own inputs: the training features rebuilt through
    the C ABI (knn_threshold -> train_activate_lists) give the host's codebook; the detection features give the host's votes and
    vote-slot ranges (knn_threshold -> cast_votes_csr, slot range of object o = act_off[feature_off[o]] * max_votes); and the host's
    maxima equal the oracle's find_maxima on those votes."""
    import torch
    capi = pkg.capi
    ctx, dev = gpu
    syn = pkg.synthetic
    train = syn.Dataset(3, 9, split=0, n_points=4096, leaf=0.2)
    test = syn.Dataset(3, 6, split=1, n_points=4096, leaf=0.2)
    order = sorted(range(9), key=lambda i: (train.label(i), i))

    def trained(thr):
        m = hb.Model()
        m.config_from_json(_threshold_cfg(thr))
        for i in order:
            o = train.get(i)
            m.add_training(o["xyz"], o["normals"], o["label"], i)
        m.train()
        return m

    # a threshold with a few activations per training feature (squared L2 between the training descriptors)
    m0 = trained(0.25)
    tf = _last_features(m0, 0)
    m0.close()
    d = torch.as_tensor(tf["desc"]).to(dev)
    d2 = ((d * d).sum(1, keepdim=True) - 2 * d @ d.T + (d * d).sum(1)[None, :]).cpu().numpy()
    thr = float(np.quantile(d2, 6.0 / len(d2)))
    m = trained(thr)
    tf = _last_features(m, 0)
    n = len(tf["desc"])
    # ---- training: the host's codebook against the C ABI path on the host's training features
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    nf = len(tf["desc"])
    cbw = capi.Codebook(ctx, tf["desc"], np.arange(nf + 1, dtype=np.uint32), np.zeros((nf, 3), np.float32), np.zeros(nf, np.uint32),
                        np.zeros(nf, np.uint32), 1, np.ones(1, np.float32))
    off, idx, _ = capi.knn_threshold(ctx, cbw, 0, T(tf["desc"]), thr)
    cbw.close()
    assert len(np.unique(np.diff(off))) > 2
    kp = tf["kp"]
    want = capi.train_activate_lists(ctx, 0, T(tf["desc"]), T(tf["lrf"]), T(kp[:, 0]), T(kp[:, 1]), T(kp[:, 2]), tf["cls"], tf["model"],
                                     tf["center"], off, idx, n_classes=3)
    cb = m.codebook_all()
    ws = want["word_src"].astype(np.int64)
    assert np.array_equal(cb["words"], tf["desc"][ws])
    assert np.array_equal(cb["vote_offsets"], want["vote_offsets"])
    assert np.array_equal(cb["vote_class"], tf["cls"][want["vote_feature"]])
    for k in ("vote_xyz", "vote_weight", "vote_class_weight", "class_sigma"):
        assert np.allclose(cb[k], want[k], rtol=1e-6, atol=1e-7, equal_nan=True), k
    # ---- detection
    nb = test.batch(range(6))
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16)
    df = _last_features(m, 1)
    votes = _last_votes(m, 6)
    assert len(df["off"]) == 7
    dcb = capi.Codebook(ctx, cb["words"], cb["vote_offsets"], cb["vote_xyz"], cb["vote_class"], cb["vote_instance"], 3, cb["class_sigma"],
                        word_weight=cb["word_weight"], vote_weight=cb["vote_weight"], vote_class_weight=cb["vote_class_weight"])
    off_d, idx_d, dist_d = capi.knn_threshold(ctx, dcb, 0, T(df["desc"]), thr)
    kq = df["kp"]
    mine = capi.cast_votes_csr(ctx, dcb, 0, T(df["lrf"]), T(kq[:, 0]), T(kq[:, 1]), T(kq[:, 2]), off_d, idx_d, dist_d)
    maxv = dcb.max_votes
    dcb.close()
    assert np.array_equal(votes["slot_off"], off_d[df["off"].astype(np.int64)] * maxv)
    assert np.array_equal(votes["cls"], mine["cls"].cpu().numpy())
    assert np.array_equal(votes["inst"], mine["inst"].cpu().numpy())
    assert np.array_equal(votes["weight"], mine["weight"].cpu().numpy())
    assert np.array_equal(votes["pos"], mine["pos"].cpu().numpy())
    # ---- the host's maxima = the oracle's mean shift on the host's votes (Voting: MeanShift, Bandwidth 0.6, single-object mode "None")
    mx = ora.find_maxima(votes["slot_off"], votes, 3, 0.6, max_maxima=16)
    assert np.array_equal(got["n"], mx["n"])
    assert (got["n"] > 0).all()
    for o in range(6):
        k = int(got["n"][o])
        assert np.array_equal(got["cls"][o, :k], mx["cls"][o, :k])
        assert np.abs(got["weight"][o, :k] - mx["weight"][o, :k]).max() <= 1e-4
        # positions: the mean shift stops once a step is below Voting.Threshold (1e-3), so the two agree to that, not to 1e-4
        assert np.abs(got["pos"][o, :k] - mx["pos"][o, :k]).max() <= 1e-3
    m.close()
