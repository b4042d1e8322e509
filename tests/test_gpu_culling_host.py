"""The C++ host with Keypoints type "VoxelGridCulling" on the MI355X: train() and detectBatch() with config/modelnet10_shot_culling.ism
(kpq, CutOff 0.5, DisableFilterInTraining) take their keypoints from ismhip_voxel_keypoints + ismhip_principal_curvatures +
ismhip_culling_scores + ismhip_culling_select on the batch's search surface -- with input normals, through the device's normal estimation,
and on coloured clouds with colordistance + RequireBoth. The keypoint positions of the host's features must be those of
capi.voxel_culling_keypoints on the same clouds, bit for bit (every descriptor of these clouds is valid, so no keypoint leaves between
detection and description); in training, under DisableFilterInTraining, those of capi.voxel_keypoints."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import host_binding as hb
from test_threshold_host import _last_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "config", "modelnet10_shot_culling.ism")
NORMAL_RADIUS = 0.15
N_TRAIN, N_TEST = 9, 6

pytestmark = pytest.mark.gpu


def _cfg(**params):
    j = json.load(open(EXAMPLE))["ObjectConfig"]
    j["Children"]["Keypoints"]["Parameters"].update(params)
    j["Parameters"]["NormalRadius"] = NORMAL_RADIUS
    return json.dumps(j), j["Children"]["Keypoints"]["Parameters"]


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _capi_keypoints(pkg, ctx, dev, P, pt_off, xyz, normals=None, rgba=None, is_training=False):
    """capi.voxel_culling_keypoints with the parameters P on the clouds the host's descriptor stage sees: as they are (normals given), or
    after the device's normal estimation (ConsistentNormalsMethod 2) and the removal of the points whose normal is NaN"""
    capi = pkg.capi
    t = [_dev(xyz[:, i], dev) for i in range(3)]
    c = None if rgba is None else _dev(np.asarray(rgba, np.uint32).view(np.int32), dev)
    if normals is not None:
        t += [_dev(normals[:, i], dev) for i in range(3)]
    else:
        import torch
        t += [torch.zeros_like(t[0]) for _ in range(3)]
        first = capi.Cloud(ctx, pt_off, *t, NORMAL_RADIUS * 0.5)
        capi.estimate_normals(ctx, first, NORMAL_RADIUS, *t[3:])
        out = capi.filter_normals(ctx, pt_off, *t, rgba=c)
        pt_off, t = out[0], list(out[1:7])
        c = out[7] if c is not None else None
        first.close()
    cloud = capi.Cloud(ctx, pt_off, *t, 0.11, rgba=c)                     # any cell size: the detector does not depend on it
    ko, kx, ky, kz, _kc = capi.voxel_culling_keypoints(
        ctx, cloud, P["LeafSize"], P["FilterMethodGeometry"], P["FilterMethodColor"], P["FilterTypeGeometry"], P["FilterTypeColor"],
        P["FilterThresholdGeometry"], P["FilterThresholdColor"], P["MaxSimilarColorDistance"], P["FilterCutoffRatio"], P["CombineFilters"],
        P["DisableFilterInTraining"], is_training)
    vo = capi.voxel_keypoints(ctx, pt_off, *t[:3], P["LeafSize"], rgba=c)[0]
    ctx.sync()
    kp = np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1)
    cloud.close()
    return ko, kp, vo


def _processing_time(m, key):
    out = C.c_double(-1.0)
    rc = m.L.ism3d_processing_time(m.h, key.encode(), C.byref(out))
    return None if rc != 0 else out.value


def _colors(xyz):
    base = np.where((np.sin(9.0 * xyz[:, 0]) > 0)[:, None], np.array([200, 60, 40]), np.array([60, 90, 190])).astype(np.uint32)
    base[:, 1] += (np.arange(len(xyz)) % 7).astype(np.uint32)
    return (base[:, 0] << 16) | (base[:, 1] << 8) | base[:, 2]


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


@pytest.mark.parametrize("mode", ["normals", "estimated", "color"])
def test_host_train_and_detect_take_the_device_keypoints(pkg, gpu, data, mode, monkeypatch):
    ctx, dev = gpu
    monkeypatch.setenv("ISM3D_HOST_KEYPOINTS", "1")                       # the VoxelGrid switch: does not apply
    with_normals, color = mode != "estimated", mode == "color"
    text, P = _cfg(**(dict(FilterMethodGeometry="Curvature", FilterMethodColor="ColorDistance", CombineFilters="RequireBoth",
                           MaxSimilarColorDistance=0.02) if color else {}))
    m = hb.Model()
    m.config_from_json(text)
    for i, o in zip(data["order"], data["train"]):
        m.add_training(o["xyz"], o["normals"] if with_normals else np.zeros_like(o["normals"]), o["label"], i, rgba=_colors(o["xyz"]) if color else None)
    m.train()
    assert _processing_time(m, "keypoints") is not None and _processing_time(m, "keypoints") > 0.0
    f = _last_features(m, 0)
    rgba = _colors(data["train_xyz"]) if color else None
    ko, kp, vo = _capi_keypoints(pkg, ctx, dev, P, data["train_off"], data["train_xyz"], data["train_nrm"] if with_normals else None, rgba, is_training=True)
    assert np.array_equal(ko, vo)                                         # DisableFilterInTraining: the plain voxel grid
    assert m.codebook_size() == len(kp)                                   # Clustering "None": one codeword per feature
    assert np.array_equal(f["kp"].view(np.uint32), kp.view(np.uint32))
    nb = data["test"]
    nrm = nb["normals"] if with_normals else np.zeros_like(nb["normals"])
    rgba = _colors(nb["xyz"]) if color else None
    before = _processing_time(m, "keypoints")
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nrm, max_maxima=4, rgba=rgba)
    assert _processing_time(m, "keypoints") > before
    d = _last_features(m, 1)
    ko, kp, vo = _capi_keypoints(pkg, ctx, dev, P, nb["pt_off"], nb["xyz"], nb["normals"] if with_normals else None, rgba)
    print("%s: %d of %d voxel keypoints kept in %d objects" % (mode, len(kp), int(vo[-1]), len(ko) - 1))
    assert 0 < len(kp) < int(vo[-1]) and len(kp) >= 5 * (len(ko) - 1)     # a culling, not a pass-through
    assert np.array_equal(np.asarray(d["off"], np.uint32), ko), mode      # every descriptor valid: no keypoint was dropped
    assert np.array_equal(d["kp"].view(np.uint32), kp.view(np.uint32)), mode
    assert (got["n"] > 0).all()
    print("classes", got["cls"][:, 0].tolist(), "labels", nb["labels"].tolist())
    m.close()


def test_host_refuses_colordistance_without_colours(pkg, gpu, data):
    text, _P = _cfg(FilterMethodGeometry="None", FilterMethodColor="colordistance", DisableFilterInTraining=False)
    m = hb.Model()
    m.config_from_json(text)
    for i, o in zip(data["order"][:3], data["train"][:3]):
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    with pytest.raises(hb.HostError, match="needs clouds with colours"):
        m.train()
    m.close()
