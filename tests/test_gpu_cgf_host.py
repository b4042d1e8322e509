"""The C++ host with Features type "CGF" on the MI355X: a model trained on three synthetic classes with seeded weights has a codebook whose
rows agree with the Python driver's (pipeline.Recognizer with feature="CGF") within the perceptron's derived bound, the same vote classes,
survives write / read bit for bit, and both hosts label the training shapes alike, with equal class scores. The host's chunking
(ISMHIP_CGF_CHUNK) does not move a bit.

The two hosts place their voxel-grid keypoints with different accumulation widths, which can move a keypoint by an ulp. A raw row is
made of integer counts, so it moves only when that ulp carries a neighbour across a bin edge; the rows of the two codebooks are held to
twice the perceptron's derived bound (cgf_ref.mlp_bound_unit_mass: each host within e of the exact embedding of the same raw row)."""
import json
import os

import numpy as np
import pytest

import cgf_ref as ref
import cgf_scenes as scenes
import host_binding as hb
from test_gpu_host_routes import _split

pytestmark = pytest.mark.gpu
D = 32


def _model_cfg(weights):
    j = json.load(open(os.path.join(hb.ROOT, "config", "modelnet10_cgf.ism")))["ObjectConfig"]
    assert j["Children"]["Features"]["Type"] == "CGF"
    j["Children"]["Features"]["Parameters"]["CgfModelFile"] = weights
    return json.dumps(j)


def test_cgf_end_to_end_through_host_and_driver(pkg, gpu, tmp_path, monkeypatch):
    ctx, dev = gpu
    layers = scenes.random_layers(np.random.default_rng(41), [ref.DIM, 64, 64, D], scenes.MLP_NNZ)
    weights = str(tmp_path / "seeded.cgfw")
    pkg.capi.cgfw_write(weights, layers)
    train, _, order = _split(pkg)
    m = hb.Model()
    m.config_from_json(_model_cfg(weights))
    assert m.L.ism3d_descriptor_length(m.h) == D
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    cfg = pkg.pipeline.IsmConfig(n_classes=3, feature="CGF", cgf_model=weights, radius=0.4, lrf_radius=0.3, bandwidth=0.6)
    assert cfg.dim == D
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(train.batch(order), dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(D, 3)
    assert words.shape == cb["words"].shape and words.shape[1] == D and len(words) > 100
    assert np.array_equal(vcls, cb["vote_class"])
    # either host is within e of the exact embedding of its raw row, e derived in cgf_ref for any row of non-negative bins that sum to 1
    e = ref.mlp_bound_unit_mass(layers)
    row_err = np.abs(words.astype(np.float64) - cb["words"])
    print("codebook: %d words of %d floats; largest difference between the two hosts' rows %.3g (%.3g of the bound 2 e; largest e %.3g)"
          % (len(words), D, row_err.max(), (row_err / (2.0 * e)).max(), e.max()))
    assert (row_err <= 2.0 * e).all()
    assert np.isfinite(words).all()
    path = str(tmp_path / "cgf.ism")
    m.write(path)
    saved = json.load(open(path))["ObjectConfig"]["Children"]["Features"]
    assert saved["Type"] == "CGF" and saved["Parameters"]["CgfModelFile"] == weights and os.path.exists(str(tmp_path / "cgf.ismd"))
    monkeypatch.setenv("ISMHIP_CGF_CHUNK", "37")                           # the second model embeds in chunks of 37 keypoints
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(D, 3)[0].view(np.uint32), words.view(np.uint32))
    nb = train.batch(order)
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    monkeypatch.delenv("ISMHIP_CGF_CHUNK")
    got1 = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    assert np.array_equal(got["cls"], got1["cls"]) and np.array_equal(got["weight"].view(np.uint32), got1["weight"].view(np.uint32))
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    ctx.sync()
    print("classes", got["cls"][:, 0].tolist(), "labels", nb["labels"].tolist())
    assert np.array_equal(want["cls"][:, 0].cpu().numpy(), got["cls"][:, 0])   # labels identical between the hosts
    assert np.allclose(got["weight"][:, 0], want["weight"][:, 0].cpu().numpy(), rtol=1e-4, atol=1e-6)
    m.close(); m2.close()
