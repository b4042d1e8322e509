"""The C++ host with Features type "RSD" and VoxelGrid keypoints on the MI355X, in both modes: three synthetic classes of two small
objects each are trained; the codebook has dim 25 (or 2) and its rows are, bit for bit, those of the Python pipeline
(pipeline.Recognizer with feature="RSD") on the same clouds; the model is written and read back with both parameters, and detectBatch
agrees with the pipeline's maxima.

The two hosts form the voxel centroids with different accumulation widths (the device in fixed point and float, the pipeline's input in
float64), which elsewhere moves a keypoint by an ulp -- and an ulp can move a point across the ball of this discontinuous descriptor. So
the clouds here are rounded to multiples of 2^-10: every voxel sum is then exact in either width (12 bits a coordinate, a few hundred
points a voxel) and both divide the same two numbers, while no such point comes nearer than 1 / 5120 to a voxel face of LeafSize 0.2."""
import json
import os

import numpy as np
import pytest

import host_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_rsd.ism")
N_TRAIN = 6

pytestmark = pytest.mark.gpu


def _lattice_batch(pkg, train, order, leaf):
    objs = []
    for i in order:
        o = train.get(i)
        xyz = (np.rint(o["xyz"].astype(np.float64) * 1024.0) / 1024.0).astype(np.float32)
        objs.append(dict(xyz=xyz, normals=o["normals"], kp=pkg.synthetic.voxel_grid(xyz, leaf), label=o["label"]))
    pt_off = np.concatenate([[0], np.cumsum([len(o["xyz"]) for o in objs])]).astype(np.uint32)
    kp_off = np.concatenate([[0], np.cumsum([len(o["kp"]) for o in objs])]).astype(np.uint32)
    return objs, dict(pt_off=pt_off, kp_off=kp_off, xyz=np.concatenate([o["xyz"] for o in objs]),
                      normals=np.concatenate([o["normals"] for o in objs]), kp=np.concatenate([o["kp"] for o in objs]),
                      labels=np.array([o["label"] for o in objs], np.int32))


@pytest.mark.parametrize("full, dim", [(True, 25), (False, 2)])
def test_host_trains_and_detects_with_rsd(pkg, gpu, tmp_path, full, dim):
    ctx, dev = gpu
    obj_cfg = json.load(open(CFG))["ObjectConfig"]
    feat = obj_cfg["Children"]["Features"]
    assert feat["Type"] == "RSD" and obj_cfg["Children"]["Keypoints"]["Type"] == "VoxelGrid"
    feat["Parameters"]["UseFullRSDHistogram"] = full
    leaf = obj_cfg["Children"]["Keypoints"]["Parameters"]["LeafSize"]
    train = pkg.synthetic.Dataset(3, N_TRAIN, split=0, n_points=2048, leaf=leaf)
    order = sorted(range(N_TRAIN), key=lambda i: (train.label(i), i))
    objs, nb = _lattice_batch(pkg, train, order, leaf)
    m = hb.Model()
    m.config_from_json(json.dumps(obj_cfg))
    for i, o in zip(order, objs):
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    # the Python pipeline on the same clouds
    cfg = pkg.pipeline.IsmConfig(n_classes=3, feature="RSD", use_full_rsd_histogram=full)
    assert cfg.dim == dim and cfg.radius == pytest.approx(feat["Parameters"]["Radius"])
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(nb, dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(dim, 3)
    print("codebook: %d words of %d floats from %d keypoints" % (len(words), dim, len(nb["kp"])))
    assert words.shape == cb["words"].shape and words.shape[1] == dim and len(words) >= 10 * N_TRAIN
    assert np.array_equal(words.view(np.uint32), np.asarray(cb["words"], np.float32).view(np.uint32))
    assert np.isfinite(words).all() and np.array_equal(vcls, cb["vote_class"])
    if full:
        assert (words >= 0).all() and (words.sum(1) > 0).all()
    else:                                                                # [smaller, larger], neither above 1.1f * Radius
        assert (words[:, 0] <= words[:, 1]).all() and (words > 0).all()
        assert words.max() <= np.float32(np.float32(feat["Parameters"]["Radius"]) * np.float32(1.1))
    # persistence: both parameters survive
    path = str(tmp_path / "rsd.ism")
    m.write(path)
    saved = json.load(open(path))["ObjectConfig"]["Children"]["Features"]
    assert saved["Type"] == "RSD" and saved["Parameters"]["UseFullRSDHistogram"] is full
    assert saved["Parameters"]["Radius"] == pytest.approx(feat["Parameters"]["Radius"]) and os.path.exists(str(tmp_path / "rsd.ismd"))
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(dim, 3)[0].view(np.uint32), words.view(np.uint32))
    back = json.loads(m2.config_to_json())["Children"]["Features"]["Parameters"]
    assert back["UseFullRSDHistogram"] is full and back["Radius"] == pytest.approx(feat["Parameters"]["Radius"])
    # detection on the training clouds: the host's answer is the pipeline's
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    ctx.sync()
    wn = np.minimum(want["n"].cpu().numpy(), 8)
    assert np.array_equal(got["n"], wn) and (wn > 0).all()
    print("classes", got["cls"][:, 0].tolist(), "labels", nb["labels"].tolist())
    for o in range(N_TRAIN):
        k = int(wn[o])
        assert np.array_equal(got["cls"][o, :k], want["cls"][o, :k].cpu().numpy())
        assert np.allclose(got["weight"][o, :k], want["weight"][o, :k].cpu().numpy(), rtol=1e-5, atol=1e-7)
        assert np.allclose(got["pos"][o, :k], want["pos"][o, :k].cpu().numpy(), rtol=0, atol=1e-5)
    m.close(); m2.close()
