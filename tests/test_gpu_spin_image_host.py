"""The C++ host with Features type "SpinImage" and Keypoints type "ISS3D" on the MI355X: three synthetic classes of two small objects each
are trained; the codebook has dim 153 and its rows are, bit for bit, those of the Python pipeline (pipeline.Recognizer with
feature="SpinImage") on the same clouds and the same ISS3D keypoints; the model is written, read back, and detectBatch agrees with the
pipeline's labels and maxima. ISS3D keypoints are cloud points, so every keypoint finds its normal (tests/test_gpu_spin_image.py checks the
lookup itself)."""
import json
import os

import numpy as np
import pytest

import host_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_spin_image_iss3d.ism")
N_TRAIN = 6

pytestmark = pytest.mark.gpu


def _with_iss3d_keypoints(pkg, ctx, dev, nb, iss):
    """the batch nb with its keypoints replaced by capi.iss3d_keypoints on its clouds (what the host's finishBatch computes)"""
    import torch
    capi = pkg.capi
    t = [torch.as_tensor(np.ascontiguousarray(nb[k][:, i])).to(dev) for k in ("xyz", "normals") for i in range(3)]
    cloud = capi.Cloud(ctx, nb["pt_off"], *t, 0.11)                       # any cell size: the detector does not depend on it
    ko, kx, ky, kz, _kc, _src = capi.iss3d_keypoints(ctx, cloud, iss["SalientRadius"], iss["NonMaxRadius"], iss["Gamma21"], iss["Gamma32"],
                                                     iss["MinNeighbors"])
    ctx.sync()
    out = dict(nb)
    out["kp_off"] = np.asarray(ko, np.uint32)
    out["kp"] = np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1)
    cloud.close()
    return out


def test_host_trains_and_detects_with_spin_image(pkg, gpu, tmp_path):
    ctx, dev = gpu
    obj_cfg = json.load(open(CFG))["ObjectConfig"]
    assert obj_cfg["Children"]["Features"]["Type"] == "SpinImage" and obj_cfg["Children"]["Keypoints"]["Type"] == "ISS3D"
    iss = obj_cfg["Children"]["Keypoints"]["Parameters"]
    train = pkg.synthetic.Dataset(3, N_TRAIN, split=0, n_points=2048, leaf=0.2)
    order = sorted(range(N_TRAIN), key=lambda i: (train.label(i), i))
    m = hb.Model()
    m.config_from_json(json.dumps(obj_cfg))
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    # the Python pipeline on the same clouds and keypoints
    nb = _with_iss3d_keypoints(pkg, ctx, dev, train.batch(order), iss)
    cfg = pkg.pipeline.IsmConfig(n_classes=3, feature="SpinImage")
    assert cfg.dim == 153 and cfg.radius == pytest.approx(obj_cfg["Children"]["Features"]["Parameters"]["Radius"])
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(nb, dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(153, 3)
    print("codebook: %d words from %d keypoints" % (len(words), len(nb["kp"])))
    assert words.shape == cb["words"].shape and words.shape[1] == 153 and len(words) >= 10 * N_TRAIN
    assert np.array_equal(words.view(np.uint32), np.asarray(cb["words"], np.float32).view(np.uint32))
    assert np.isfinite(words).all() and np.abs(words.sum(1) - 1.0).max() < 1e-5          # every keypoint found its axis and its neighbours
    assert np.array_equal(vcls, cb["vote_class"])
    # persistence
    path = str(tmp_path / "spin.ism")
    m.write(path)
    saved = json.load(open(path))
    assert saved["ObjectConfig"]["Children"]["Features"]["Type"] == "SpinImage" and os.path.exists(str(tmp_path / "spin.ismd"))
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(153, 3)[0].view(np.uint32), words.view(np.uint32))
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
