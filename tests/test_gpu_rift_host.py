"""The C++ host with Features type "RIFT" on the MI355X: a model trained on three coloured synthetic classes has a codebook of dim 128
with the rows and vote classes of the Python driver (pipeline.Recognizer with feature="RIFT") on the same clouds, survives write / read
bit for bit, and both hosts label the training shapes correctly, with equal class scores.

The two hosts place their voxel-grid keypoints with different accumulation widths, which moves a keypoint by an ulp; RIFT's weights are
continuous in the keypoint (a ball point that crosses the boundary carries weight 0 at the outer distance bin), so rows are compared
within the descriptor tolerance 1e-4, and the kept rows (the keypoints whose row is not NaN) must be the same."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
from test_gpu_host_routes import _split

pytestmark = pytest.mark.gpu


def _model_cfg():
    """the value set of config/kinect_rift.ism with its lengths (Radius, ReferenceFrameRadius, LeafSize, Bandwidth: those of 0.15-unit
    Kinect views) replaced by the ones that fit the unit-sized synthetic shapes"""
    j = json.load(open(os.path.join(hb.ROOT, "config", "kinect_rift.ism")))["ObjectConfig"]
    assert j["Children"]["Features"]["Type"] == "RIFT"
    j["Children"]["Features"]["Parameters"].update(Radius=0.4, ReferenceFrameRadius=0.3)
    j["Children"]["Keypoints"]["Parameters"]["LeafSize"] = 0.2
    j["Children"]["Voting"]["Parameters"]["Bandwidth"] = 0.6
    return json.dumps(j)


def test_rift_end_to_end_through_host_and_driver(pkg, gpu, tmp_path):
    ctx, dev = gpu
    train, _, order = _split(pkg, with_color=True)
    m = hb.Model()
    m.config_from_json(_model_cfg())
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i, rgba=o["rgba"])
    m.train()
    cfg = pkg.pipeline.IsmConfig(n_classes=3, feature="RIFT", distance="ChiSquared", radius=0.4, lrf_radius=0.3, bandwidth=0.6)
    assert cfg.dim == pkg.capi.RIFT_DIM == 128
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(train.batch(order), dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(128, 3)
    # the kept rows: as many words, in the same order, with the same vote classes
    assert words.shape == cb["words"].shape and words.shape[1] == 128 and len(words) > 100
    assert np.array_equal(vcls, cb["vote_class"])
    row_err = np.abs(words - cb["words"]).max(1)
    print("codebook: %d words of 128 floats; largest difference between the two hosts' rows %.3g" % (len(words), row_err.max()))
    assert row_err.max() <= 1e-4
    assert np.isfinite(words).all() and (words >= 0).all() and np.allclose((words.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-5)
    path = str(tmp_path / "rift.ism")
    m.write(path)
    saved = json.load(open(path))["ObjectConfig"]["Children"]["Features"]
    assert saved["Type"] == "RIFT" and saved["Parameters"]["Radius"] == pytest.approx(0.4) and os.path.exists(str(tmp_path / "rift.ismd"))
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(128, 3)[0].view(np.uint32), words.view(np.uint32))
    nb = train.batch(order)
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8, rgba=nb["rgba"])
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    ctx.sync()
    print("classes", got["cls"][:, 0].tolist(), "labels", nb["labels"].tolist())
    assert (got["cls"][:, 0] == nb["labels"]).all()
    assert np.array_equal(want["cls"][:, 0].cpu().numpy(), got["cls"][:, 0])
    assert np.allclose(got["weight"][:, 0], want["weight"][:, 0].cpu().numpy(), rtol=1e-4, atol=1e-6)   # the class scores
    m.close(); m2.close()
