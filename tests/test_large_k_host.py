"""KNN activation with K > 16 in the C++ host mirror (libism3d_amd.so): a K = 24 model trains and detects end to end against the
Python harness with the same K and the CPU oracle's detection; a K above ISMHIP_KNN_LARGE_K_MAX is refused by name before anything runs on the device."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
import oracle_pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")


def _knn_cfg(k):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Codebook"]["Children"]["ActivationStrategy"] = {"Type": "KNN", "Parameters": {"K": k}}
    return json.dumps(j)


def _dataset(pkg):
    syn = pkg.synthetic
    return (syn.Dataset(3, 9, split=0, n_points=4096, leaf=0.2), syn.Dataset(3, 6, split=1, n_points=4096, leaf=0.2))


@pytest.mark.gpu
def test_host_knn_k2000_refused_by_name(pkg, gpu):
    train, _ = _dataset(pkg)
    m = hb.Model()
    m.config_from_json(_knn_cfg(2000))
    for i in range(3):
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    with pytest.raises(Exception, match="ISMHIP_KNN_LARGE_K_MAX"):
        m.train()
    m.close()


@pytest.mark.gpu
def test_host_knn_k24_train_and_detect_matches_python_harness_and_oracle(pkg, gpu, ora):
    ctx, dev = gpu
    train, test = _dataset(pkg)
    order = sorted(range(9), key=lambda i: (train.label(i), i))
    m = hb.Model()
    m.config_from_json(_knn_cfg(24))
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    cfg = pkg.pipeline.IsmConfig(n_classes=3, k=24)
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(train.batch(order), dev)], instance_ids=order)
    got_cb = m.codebook_all()                                      # (sized by the vote count: K votes per feature)
    words, vxyz, vcls = got_cb["words"], got_cb["vote_xyz"], got_cb["vote_class"]
    assert words.shape == cb["words"].shape
    np.testing.assert_allclose(words, cb["words"], atol=2e-5)      # keypoints differ by an ulp between the hosts (test_host_layer.py)
    np.testing.assert_allclose(vxyz, cb["vote_xyz"], atol=1e-4)
    assert np.array_equal(vcls, cb["vote_class"])
    assert len(vcls) >= 24 * len(words) - 24 * 24                  # every feature cast K votes
    nb = test.batch(range(6))
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    assert np.array_equal(got["n"], np.minimum(want["n"].cpu().numpy(), 8))
    k = 4
    assert np.array_equal(got["cls"][:, :k], want["cls"][:, :k].cpu().numpy())
    np.testing.assert_allclose(got["weight"][:, :k], want["weight"][:, :k].cpu().numpy(), atol=1e-4)
    np.testing.assert_allclose(got["pos"][:, :k], want["pos"][:, :k].cpu().numpy(), atol=2e-3)
    # the CPU oracle's detection (its own exact 24-NN, vote casting and mean shift) on the harness's codebook and keypoints
    ref = oracle_pipeline.detect(ora, cfg, cb, nb, cfg.n_classes)
    assert ref["idx"].shape[1] == 24
    assert np.array_equal(want["cls"][:, :k].cpu().numpy(), ref["cls"][:, :k])
    np.testing.assert_allclose(want["weight"][:, :k].cpu().numpy(), ref["weight"][:, :k], atol=1e-4)
    assert np.array_equal(got["cls"][:, 0], ref["cls"][:, 0])
    np.testing.assert_allclose(got["weight"][:, 0], ref["weight"][:, 0], atol=1e-4)
    m.close()
