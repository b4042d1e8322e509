"""The C++ host with Features type "USC" and VoxelGrid keypoints on the MI355X: three synthetic classes of three small objects each are
trained with the settings of config/modelnet10_usc.ism; the codebook has dim 1960 and its rows are, bit for bit, those of the Python
pipeline (pipeline.Recognizer with feature="USC") on the same clouds -- both compute the point density once per cloud, the rows' own
SHOT frames at Radius - 0.1 and the rows with the minimal radius Radius / 10; the model is written and read back, detectBatch agrees with
the pipeline's maxima, a second detection gives the same bytes, and the activated codewords are those of the oracle's exact search
(the FLANN functor in its own order) on the device's own rows: rows of 1960 floats go through the wide scan of ismhip_knn.

As in test_gpu_rsd_host.py the clouds are rounded to multiples of 2^-10, so that the two hosts' voxel centroids are the same floats and
no keypoint's ball differs by a point."""
import json
import os

import numpy as np
import pytest

import host_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_usc.ism")
N_TRAIN = 9
DIM = 1960

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


def test_host_trains_and_detects_with_usc(pkg, gpu, ora, tmp_path):
    ctx, dev = gpu
    obj_cfg = json.load(open(CFG))["ObjectConfig"]
    feat = obj_cfg["Children"]["Features"]
    assert feat["Type"] == "USC" and obj_cfg["Children"]["Keypoints"]["Type"] == "VoxelGrid"
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
    cfg = pkg.pipeline.IsmConfig(n_classes=3, feature="USC")
    assert cfg.dim == DIM and cfg.radius == pytest.approx(feat["Parameters"]["Radius"])
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(nb, dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(DIM, 3)
    print("codebook: %d words of %d floats from %d keypoints" % (len(words), DIM, len(nb["kp"])))
    assert words.shape == cb["words"].shape and words.shape[1] == DIM and len(words) >= 10 * N_TRAIN
    assert np.array_equal(words.view(np.uint32), np.asarray(cb["words"], np.float32).view(np.uint32))
    assert np.isfinite(words).all() and np.array_equal(vcls, cb["vote_class"])
    assert (words >= 0).all() and (words > 0).any(1).all()                     # not normalised: non-negative, no empty row
    # persistence
    path = str(tmp_path / "usc.ism")
    m.write(path)
    saved = json.load(open(path))["ObjectConfig"]["Children"]["Features"]
    assert saved["Type"] == "USC" and saved["Parameters"]["Radius"] == pytest.approx(feat["Parameters"]["Radius"])
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(DIM, 3)[0].view(np.uint32), words.view(np.uint32))
    # detection on the training clouds: the host's answer is the pipeline's, and the same from run to run
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    again = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev), keep_intermediates=True)
    ctx.sync()
    # the activation: the oracle's exact search on the device's own rows
    rows = want["features"]["desc"].cpu().numpy()
    assert rows.shape[1] == DIM
    widx, wdist = ora.knn(cfg.metric, np.asarray(cb["words"], np.float32), rows, 1)
    assert np.array_equal(want["idx"].cpu().numpy().reshape(-1), widx.reshape(-1))
    assert np.array_equal(want["dist"].cpu().numpy().reshape(-1).view(np.uint32), wdist.reshape(-1).view(np.uint32))
    wn = np.minimum(want["n"].cpu().numpy(), 8)
    assert np.array_equal(got["n"], wn) and (wn > 0).all()
    print("classes", got["cls"][:, 0].tolist(), "labels", nb["labels"].tolist())
    for key in ("n", "cls", "weight", "pos"):
        assert np.array_equal(np.asarray(got[key]).view(np.uint8), np.asarray(again[key]).view(np.uint8)), key
    for o in range(N_TRAIN):
        k = int(wn[o])
        assert np.array_equal(got["cls"][o, :k], want["cls"][o, :k].cpu().numpy())
        assert np.allclose(got["weight"][o, :k], want["weight"][o, :k].cpu().numpy(), rtol=1e-5, atol=1e-7)
        assert np.allclose(got["pos"][o, :k], want["pos"][o, :k].cpu().numpy(), rtol=0, atol=1e-5)
    m.close(); m2.close()
