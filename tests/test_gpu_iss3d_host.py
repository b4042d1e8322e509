"""The C++ host with Keypoints type "ISS3D" on the MI355X: train() and detectBatch() take their keypoints from ismhip_iss3d_keypoints on the
batch's search surface, with input normals and through the route that estimates them on the device. The keypoint positions of the
host's features must be those of capi.iss3d_keypoints on the same clouds, bit for bit (every descriptor of these clouds is valid, so no
keypoint leaves between detection and description)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import host_binding as hb
from test_threshold_host import _last_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
ISS = {"SalientRadius": 0.2, "NonMaxRadius": 0.1, "Gamma21": 0.975, "Gamma32": 0.975, "MinNeighbors": 5}
NORMAL_RADIUS = 0.15
N_TRAIN, N_TEST = 9, 6

pytestmark = pytest.mark.gpu


def _cfg():
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Keypoints"] = {"Type": "ISS3D", "Parameters": dict(ISS)}
    j["Parameters"]["NormalRadius"] = NORMAL_RADIUS
    return json.dumps(j)


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _capi_keypoints(pkg, ctx, dev, pt_off, xyz, normals=None):
    """capi.iss3d_keypoints on the clouds the host's descriptor stage sees: as they are (normals given), or after the device's normal
    estimation (ConsistentNormalsMethod 2) and the removal of the points whose normal is NaN -> (offsets, kp [n, 3])"""
    capi = pkg.capi
    t = [_dev(xyz[:, i], dev) for i in range(3)]
    if normals is not None:
        t += [_dev(normals[:, i], dev) for i in range(3)]
    else:
        import torch
        t += [torch.zeros_like(t[0]) for _ in range(3)]
        first = capi.Cloud(ctx, pt_off, *t, NORMAL_RADIUS * 0.5)
        capi.estimate_normals(ctx, first, NORMAL_RADIUS, *t[3:])
        pt_off, *t = capi.filter_normals(ctx, pt_off, *t)[:7]
        first.close()
    cloud = capi.Cloud(ctx, pt_off, *t, 0.11)                             # any cell size: the detector does not depend on it
    ko, kx, ky, kz, _kc, _src = capi.iss3d_keypoints(ctx, cloud, ISS["SalientRadius"], ISS["NonMaxRadius"], ISS["Gamma21"], ISS["Gamma32"], ISS["MinNeighbors"])
    ctx.sync()
    kp = np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1)
    cloud.close()
    return ko, kp


def _processing_time(m, key):
    out = C.c_double(-1.0)
    rc = m.L.ism3d_processing_time(m.h, key.encode(), C.byref(out))
    return None if rc != 0 else out.value


def _same_keypoints(feat_off, feat_kp, ko, kp, what):
    print("%s: %d keypoints in %d objects" % (what, len(kp), len(ko) - 1))
    assert len(kp) >= 10 * (len(ko) - 1)
    assert np.array_equal(np.asarray(feat_off, np.uint32), ko), what    # every descriptor valid: no keypoint was dropped
    assert np.array_equal(feat_kp.view(np.uint32), kp.view(np.uint32)), what


@pytest.fixture(scope="module")
def data(pkg):
    syn = pkg.synthetic
    train = syn.Dataset(3, N_TRAIN, split=0, n_points=2048, leaf=0.2)
    test = syn.Dataset(3, N_TEST, split=1, n_points=2048, leaf=0.2)
    order = sorted(range(N_TRAIN), key=lambda i: (train.label(i), i))
    tr = [train.get(i) for i in order]
    po = np.zeros(N_TRAIN + 1, np.uint32); po[1:] = np.cumsum([len(o["xyz"]) for o in tr])
    return dict(order=order, train=tr, train_off=po, train_xyz=np.concatenate([o["xyz"] for o in tr]),
                train_nrm=np.concatenate([o["normals"] for o in tr]), test=test.batch(range(N_TEST)))


@pytest.mark.parametrize("with_normals", [True, False])
def test_host_train_and_detect_take_the_device_keypoints(pkg, gpu, data, with_normals, monkeypatch):
    ctx, dev = gpu
    monkeypatch.setenv("ISM3D_HOST_KEYPOINTS", "1")                       # the VoxelGrid switch: does not apply to ISS3D
    m = hb.Model()
    m.config_from_json(_cfg())
    for i, o in zip(data["order"], data["train"]):
        m.add_training(o["xyz"], o["normals"] if with_normals else np.zeros_like(o["normals"]), o["label"], i)
    m.train()
    assert _processing_time(m, "keypoints") is not None and _processing_time(m, "keypoints") > 0.0
    f = _last_features(m, 0)
    ko, kp = _capi_keypoints(pkg, ctx, dev, data["train_off"], data["train_xyz"], data["train_nrm"] if with_normals else None)
    assert m.codebook_size() == len(kp)                                   # Clustering "None": one codeword per feature
    assert np.array_equal(f["kp"].view(np.uint32), kp.view(np.uint32))
    nb = data["test"]
    nrm = nb["normals"] if with_normals else np.zeros_like(nb["normals"])
    before = _processing_time(m, "keypoints")
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nrm, max_maxima=4)
    assert _processing_time(m, "keypoints") > before
    d = _last_features(m, 1)
    ko, kp = _capi_keypoints(pkg, ctx, dev, nb["pt_off"], nb["xyz"], nb["normals"] if with_normals else None)
    _same_keypoints(d["off"], d["kp"], ko, kp, "detect, normals %s" % ("given" if with_normals else "estimated"))
    assert (got["n"] > 0).all()
    print("classes", got["cls"][:, 0].tolist(), "labels", nb["labels"].tolist())
    m.close()


def test_host_mixed_batch_takes_iss3d_on_the_device(pkg, gpu, data):
    """a mixed batch (one cloud with normals, one without) goes through the host-side normal filter and still takes ISS3D on the device"""
    ctx, dev = gpu
    m = hb.Model()
    m.config_from_json(_cfg())
    for i, o in zip(data["order"], data["train"]):
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    nb = data["test"]
    e = int(nb["pt_off"][2])
    nrm = nb["normals"][:e].copy()
    nrm[int(nb["pt_off"][1]):] = 0                                        # the second cloud comes without normals
    got = m.detect_batch(nb["pt_off"][:3], nb["xyz"][:e], nrm, max_maxima=4)
    d = _last_features(m, 1)
    assert (got["n"] > 0).all() and d["off"][1] - d["off"][0] >= 10 and d["off"][2] - d["off"][1] >= 10
    ko, kp = _capi_keypoints(pkg, ctx, dev, nb["pt_off"][:2], nb["xyz"][:int(nb["pt_off"][1])], nb["normals"][:int(nb["pt_off"][1])])
    assert np.array_equal(d["kp"][:d["off"][1]].view(np.uint32), kp.view(np.uint32))
    m.close()
