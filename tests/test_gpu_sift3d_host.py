"""The C++ host with Keypoints type "SIFT3D" on the MI355X: train() and detectBatch() take their keypoints from ismhip_normal_curvature (at the
model's NormalRadius) and ismhip_sift3d_keypoints on the batch's search surface, with input normals and through the route that estimates
them on the device. The keypoint positions of the host's features must be those of the direct capi calls on the same clouds, bit for bit
(every descriptor of these clouds is valid, so no keypoint leaves between detection and description)."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
from test_threshold_host import _last_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot_sift3d.ism")
RADIUS = 0.1                       # the shipped config's
NORMAL_RADIUS = 0.15
N_TRAIN, N_TEST = 9, 6

pytestmark = pytest.mark.gpu


def _cfg():
    j = json.load(open(CFG))["ObjectConfig"]
    assert j["Children"]["Keypoints"] == {"Type": "SIFT3D", "Parameters": {"Radius": RADIUS}}
    j["Parameters"]["NormalRadius"] = NORMAL_RADIUS
    return json.dumps(j)


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.array(a, copy=True, order="C")).to(dev)


def _capi_keypoints(pkg, ctx, dev, pt_off, xyz, normals=None):
    """capi.normal_curvature + capi.sift3d_keypoints on the clouds the host's descriptor stage sees: as they are (normals given), or after
    the device's normal estimation (ConsistentNormalsMethod 2) and the removal of the points whose normal is NaN -> (offsets, kp [n, 3])"""
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
    curv, _ = capi.normal_curvature(ctx, cloud, NORMAL_RADIUS, want_counts=False)
    ko, kx, ky, kz, _ks, _sizes = capi.sift3d_keypoints(ctx, cloud, curv, RADIUS)
    ctx.sync()
    kp = np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1)
    cloud.close()
    return ko, kp


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


def _answers(got, objs=None):
    """the valid maxima of a detect_batch answer (the arrays are uninitialised behind n): per object (classes, weight bits)"""
    objs = range(len(got["n"])) if objs is None else objs
    return [(got["cls"][o, :got["n"][o]].tolist(), got["weight"][o, :got["n"][o]].view(np.uint32).tolist()) for o in objs]


def _trained(data, with_normals=True):
    m = hb.Model()
    m.config_from_json(_cfg())
    for i, o in zip(data["order"], data["train"]):
        m.add_training(o["xyz"], o["normals"] if with_normals else np.zeros_like(o["normals"]), o["label"], i)
    m.train()
    return m


@pytest.mark.parametrize("with_normals", [True, False])
def test_host_train_and_detect_take_the_device_keypoints(pkg, gpu, data, with_normals, monkeypatch):
    ctx, dev = gpu
    monkeypatch.setenv("ISM3D_HOST_KEYPOINTS", "1")                       # the VoxelGrid switch: does not apply to SIFT3D
    m = _trained(data, with_normals)
    f = _last_features(m, 0)
    ko, kp = _capi_keypoints(pkg, ctx, dev, data["train_off"], data["train_xyz"], data["train_nrm"] if with_normals else None)
    print("train: %d keypoints in %d objects" % (len(kp), len(ko) - 1))
    assert len(kp) >= 5 * N_TRAIN
    assert m.codebook_size() == len(kp)                                   # Clustering "None": one codeword per feature
    assert np.array_equal(f["kp"].view(np.uint32), kp.view(np.uint32))
    nb = data["test"]
    nrm = nb["normals"] if with_normals else np.zeros_like(nb["normals"])
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nrm, max_maxima=4)
    d = _last_features(m, 1)
    ko, kp = _capi_keypoints(pkg, ctx, dev, nb["pt_off"], nb["xyz"], nb["normals"] if with_normals else None)
    print("detect: %d keypoints, per object %s" % (len(kp), np.diff(ko.astype(np.int64)).tolist()))
    assert np.array_equal(np.asarray(d["off"], np.uint32), ko)            # every descriptor valid: no keypoint was dropped
    assert np.array_equal(d["kp"].view(np.uint32), kp.view(np.uint32))
    assert (got["n"] > 0).all()
    again = m.detect_batch(nb["pt_off"], nb["xyz"], nrm, max_maxima=4)    # reproducible from run to run
    assert _answers(got) == _answers(again)
    print("classes", got["cls"][:, 0].tolist(), "labels", nb["labels"].tolist())
    m.close()


def test_host_batch_with_an_object_without_keypoints(pkg, gpu, data):
    """a batch that mixes ordinary objects with one too small for octave 0 (fewer than 25 voxels): an empty keypoint range, no maxima,
    and the other objects' answers as without it"""
    ctx, dev = gpu
    m = _trained(data)
    nb = data["test"]
    e1, e2 = int(nb["pt_off"][1]), int(nb["pt_off"][2])
    rng = np.random.default_rng(3)
    small = (rng.normal(size=(60, 3)) * 0.02).astype(np.float32)
    sn = small / np.linalg.norm(small, axis=1, keepdims=True)
    xyz = np.concatenate([nb["xyz"][:e1], small, nb["xyz"][e1:e2]])
    nrm = np.concatenate([nb["normals"][:e1], sn.astype(np.float32), nb["normals"][e1:e2]])
    off = np.array([0, e1, e1 + 60, e2 + 60], np.uint32)
    got = m.detect_batch(off, xyz, nrm, max_maxima=4)
    d = _last_features(m, 1)
    assert d["off"][2] == d["off"][1] and got["n"][1] == 0
    assert got["n"][0] > 0 and got["n"][2] > 0
    ko, kp = _capi_keypoints(pkg, ctx, dev, off, xyz, nrm)
    assert ko[2] == ko[1] and np.array_equal(np.asarray(d["off"], np.uint32), ko) and np.array_equal(d["kp"].view(np.uint32), kp.view(np.uint32))
    alone = m.detect_batch(nb["pt_off"][:3], nb["xyz"][:e2], nb["normals"][:e2], max_maxima=4)
    assert _answers(got, (0, 2)) == _answers(alone)
    m.close()
