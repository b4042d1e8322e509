"""BoundingBoxType "MVBB" through the C++ host (-m gpu): train() on rigidly rotated objects of the small synthetic split takes one
ismhip_region_mvbb box per training cloud, votes point at its centre and carry box.rotQuat * conj(q(LRF)); "AABB" is today's path
bit for bit; global verification gives an object without maxima its region's MVBB; AverageRotation returns the box turned with the
object."""
import ctypes as C
import json

import numpy as np
import pytest

import host_binding as hb
import mvbb_scenes as ms
from test_gpu_global_host import trained, variant
from test_gpu_host_routes import _split
from test_host_layer import _cfg
from test_threshold_host import _last_features

pytestmark = pytest.mark.gpu
F = np.float32
_state = {}


def rot_quat(l):
    """Utils::matrix2Quat on the matrix whose rows are the axes l[0:3], l[3:6], l[6:9], in float32 as the host takes it -> (w, x, y, z)"""
    m = np.asarray(l, F).reshape(3, 3)
    q = [F(0), F(0), F(0), F(1)]
    trace = F(F(m[0, 0] + m[1, 1]) + m[2, 2])
    if trace > 0:
        root = np.sqrt(F(trace + F(1)))
        q[3] = F(F(0.5) * root)
        root = F(F(0.5) / root)
        q[0] = F(F(m[2, 1] - m[1, 2]) * root); q[1] = F(F(m[0, 2] - m[2, 0]) * root); q[2] = F(F(m[1, 0] - m[0, 1]) * root)
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        root = np.sqrt(F(np.float64(F(F(m[i, i] - m[j, j]) - m[k, k])) + 1.0))
        q[i] = F(F(0.5) * root)
        root = F(F(0.5) / root)
        q[3] = F(F(m[k, j] - m[j, k]) * root); q[j] = F(F(m[j, i] + m[i, j]) * root); q[k] = F(F(m[k, i] + m[i, k]) * root)
    return np.array([q[3], q[0], q[1], q[2]], F)


def qmul(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def quat_axes(q):
    """the matrix whose rows are the axes, from (w, x, y, z): the inverse of rot_quat"""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rotated(o, seed):
    r = ms.rotation(seed)
    return (o["xyz"].astype(np.float64) @ r.T).astype(F), (o["normals"].astype(np.float64) @ r.T).astype(F), r


def train_boxes(m):
    n = m.L.ism3d_last_train_boxes(m.h, None)
    out = np.zeros((n, 10), F)
    assert m.L.ism3d_last_train_boxes(m.h, hb._p(out)) == n
    return out


def models(pkg):
    """the split's nine objects, each turned by a rotation of its own, trained once with "MVBB" and once with "AABB" """
    if "models" not in _state:
        train, _, order = _split(pkg)
        clouds = [rotated(train.get(i), 40 + i) for i in order]
        out = {}
        for kind in ("MVBB", "AABB"):
            m = hb.Model()
            m.config_from_json(_cfg(**{"Parameters/BoundingBoxType": kind}))
            for i, (xyz, nrm, _) in zip(order, clouds):
                m.add_training(xyz, nrm, train.label(i), i)
            m.train()
            out[kind] = dict(boxes=train_boxes(m), features=_last_features(m, 0), codebook=m.codebook_all())
            m.close()
        _state["models"] = (clouds, out)
    return _state["models"]


def device_boxes(pkg, gpu, clouds):
    import torch
    ctx, dev = gpu
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in clouds])]).astype(np.uint32)
    xyz, nrm = np.concatenate([c[0] for c in clouds]), np.concatenate([c[1] for c in clouds])
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (xyz, nrm) for i in range(3)]
    cloud = pkg.capi.Cloud(ctx, off, *t, 0.3)
    try:
        out = {k: v.cpu().numpy() for k, v in pkg.capi.region_mvbb(ctx, cloud, dev, np.arange(len(clouds))).items()}
        ctx.sync()
    finally:
        cloud.close()
    return out


def test_training_boxes_are_the_device_boxes(pkg, gpu):
    clouds, out = models(pkg)
    boxes, dev = out["MVBB"]["boxes"], device_boxes(pkg, gpu, clouds)
    assert boxes.shape == (9, 10)
    assert np.array_equal(boxes[:, 0:3], dev["center"]) and np.array_equal(boxes[:, 3:6], dev["size"])
    want = np.stack([rot_quat(a) for a in dev["axes"]])
    assert np.array_equal(boxes[:, 6:10], want)
    assert (np.abs(boxes[:, 6] - 1) > 1e-3).all()             # no box quaternion is the identity: every object was turned
    aabb = out["AABB"]["boxes"]
    assert (np.prod(boxes[:, 3:6].astype(np.float64), axis=1) < np.prod(aabb[:, 3:6].astype(np.float64), axis=1)).all()
    assert np.abs(boxes[:, 0:3] - aabb[:, 0:3]).max() > 1e-3


def expected_votes(model):
    """per training feature: the vote vector, box quaternion and box size that codeword_distribution.cpp:49-70 stores for it"""
    f, boxes = model["features"], model["boxes"]
    lrf = f["lrf"].astype(np.float64).reshape(-1, 3, 3)
    box = boxes[f["model"]]
    assert np.array_equal(f["center"], box[:, 0:3])           # the votes' centre is the box's position
    vec = np.einsum("fij,fj->fi", lrf, (f["center"].astype(np.float64) - f["kp"].astype(np.float64)))
    quat = np.stack([qmul(box[i, 6:10], rot_quat(f["lrf"][i]) * np.array([1, -1, -1, -1], F)) for i in range(len(lrf))])
    return vec, quat, box[:, 3:6]


def test_votes_point_at_the_box_centres_and_carry_the_box_in_the_keypoint_frame(pkg, gpu):
    _, out = models(pkg)
    for kind in ("MVBB", "AABB"):
        cb = out[kind]["codebook"]
        vec, quat, size = expected_votes(out[kind])
        # Clustering "None", K = 1: codeword w is training feature word_id[w]; every vote of it comes from a feature whose nearest
        # codeword it is -- found here as the feature whose expected vote it equals
        n_votes = len(cb["vote_xyz"])
        assert n_votes >= len(cb["words"]) > 100
        for w in range(len(cb["words"])):
            for v in range(cb["vote_offsets"][w], cb["vote_offsets"][w + 1]):
                d = np.abs(vec - cb["vote_xyz"][v]).max(1)
                fi = int(np.argmin(d))
                assert d[fi] <= 1e-5, (kind, w, v, d[fi])
                assert np.abs(quat[fi] - cb["vote_bbox_quat"][v]).max() <= 1e-6, (kind, w, v)
                assert np.array_equal(size[fi], cb["vote_bbox_size"][v]), (kind, w, v)


def test_aabb_is_todays_path_bit_for_bit(pkg, gpu):
    clouds, out = models(pkg)
    a, mv = out["AABB"], out["MVBB"]
    for o, (xyz, _, _) in enumerate(clouds):                   # Utils::computeAABB in float: size = max - min, position = min + size / 2
        lo, hi = xyz.min(0), xyz.max(0)
        size = (hi - lo).astype(F)
        assert np.array_equal(a["boxes"][o, 3:6], size) and np.array_equal(a["boxes"][o, 0:3], (lo + size / F(2)).astype(F))
        assert a["boxes"][o, 6:10].tolist() == [1, 0, 0, 0]
    f, cb = a["features"], a["codebook"]
    # the stored quaternion is conj(q(LRF)) itself, not a product with the identity: bits of the float32 transcription
    conj = {tuple(f["lrf"][i].view(np.uint32).tolist()): rot_quat(f["lrf"][i]) * np.array([1, -1, -1, -1], F) for i in range(len(f["lrf"]))}
    stored = {tuple(q.view(np.uint32).tolist()) for q in cb["vote_bbox_quat"]}
    assert stored <= {tuple(q.view(np.uint32).tolist()) for q in conj.values()}
    # what does not depend on the box is the same in both models, bit for bit
    for k in ("words", "word_id", "word_class", "word_weight", "word_keypoint", "vote_offsets", "vote_weight", "vote_class_weight", "vote_class",
              "vote_instance", "class_sigma"):
        assert np.array_equal(np.ascontiguousarray(a["codebook"][k]).view(np.uint8), np.ascontiguousarray(mv["codebook"][k]).view(np.uint8)), k
    for k in ("desc", "lrf", "kp", "cls", "model"):
        assert np.array_equal(a["features"][k].view(np.uint32), mv["features"][k].view(np.uint32)), k
    assert not np.array_equal(a["codebook"]["vote_xyz"], mv["codebook"]["vote_xyz"])


def test_global_verification_box_of_an_object_without_maxima(pkg, gpu, tmp_path_factory):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, "novotes_box", GlobalFeatureInfluenceType=3, SingleObjectMode=True, MinVotesThreshold=10000000)
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=4)
    n_obj = len(nb["pt_off"]) - 1
    assert (got["n_total"] == 1).all()
    n = m.L.ism3d_last_global_boxes(m.h, None)
    assert n == n_obj
    boxes = np.zeros((n, 10), F)
    assert m.L.ism3d_last_global_boxes(m.h, hb._p(boxes)) == n
    clouds = [(nb["xyz"][nb["pt_off"][o]:nb["pt_off"][o + 1]], nb["normals"][nb["pt_off"][o]:nb["pt_off"][o + 1]]) for o in range(n_obj)]
    dev = device_boxes(pkg, gpu, clouds)
    assert np.array_equal(boxes[:, 0:3], dev["center"]) and np.array_equal(boxes[:, 3:6], dev["size"])
    assert np.array_equal(boxes[:, 6:10], np.stack([rot_quat(a) for a in dev["axes"]]))
    assert np.array_equal(got["bbox_quat"][:, 0], boxes[:, 6:10])
    m.close()


def test_average_rotation_turns_the_box_with_the_object(pkg, gpu):
    """one training object per class, each in a pose of its own; the same objects in other poses are detected with AverageRotation: the
    box of the best maximum has the training box's axes turned by the rotation between the two poses, up to sign and order (the
    keypoints of the two poses differ, so the averaged quaternion is near, not equal: 0.95 is 18 degrees)"""
    train, _, _ = _split(pkg)
    m = hb.Model()
    m.config_from_json(_cfg(**{"Parameters/BoundingBoxType": "MVBB",
                               "Children/Voting/Parameters": {"MinThreshold": 0.0, "MinVotesThreshold": 1, "BestK": -1, "Bandwidth": 0.6, "AverageRotation": True}}))
    poses = []
    for i in range(3):
        xyz, nrm, r = rotated(train.get(i), 70 + i)
        m.add_training(xyz, nrm, train.label(i), i)
        poses.append(r)
    m.train()
    boxes = train_boxes(m)
    test = [rotated(train.get(i), 80 + i) for i in range(3)]
    off = np.concatenate([[0], np.cumsum([len(t[0]) for t in test])]).astype(np.uint32)
    got = m.detect_batch(off, np.concatenate([t[0] for t in test]), np.concatenate([t[1] for t in test]), max_maxima=8)
    m.close()
    for i in range(3):
        assert got["n"][i] >= 1 and got["cls"][i, 0] == train.label(i)
        turn = test[i][2] @ poses[i].T                         # training pose -> test pose
        want = quat_axes(boxes[i, 6:10]) @ turn.T              # rows: the training box's axes, turned
        have = quat_axes(got["bbox_quat"][i, 0])
        d = np.abs(have @ want.T)
        print("object", i, "axis cosines", d.max(1))
        assert sorted(d.argmax(1).tolist()) == [0, 1, 2] and d.max(1).min() >= 0.95, (i, d)
