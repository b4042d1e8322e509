"""The SHOTNA reference frame on the device (-m gpu): ismhip_shotna_lrf through capi on the scenes of shotna_scenes.py against the numpy
restatement shotna_ref.py and against ismhip_shot_lrf on the same Cloud. test_shotna_cpu.py proves on the host that every scene reaches
the branch asserted here and that no vote of a compared keypoint can fall either way. Frames are held to the 1e-5 of the other frame
tests; the relation to the SHOT frame is bit-exact: x equal, z equal up to one sign s per keypoint, y_na = s * y_shot, NaN rows equal."""
import json

import numpy as np
import pytest

import frontend_scenes as fs
import host_binding as hb
import shotna_scenes as sc
from test_gpu_frontend import LRF_TOL, TOL, Batch, assert_close_nan
from test_host_layer import _cfg, _dataset

pytestmark = pytest.mark.gpu


def both_frames(pkg, ctx, dev, s):
    """(SHOTNA frames, SHOT frames) of a scene on one Cloud -> numpy"""
    b = Batch(pkg, ctx, dev, s.objs, s.kps, s.cell)
    try:
        na = pkg.capi.shotna_lrf(ctx, b.cloud, b.kp_off, *b.tk, s.radius).cpu().numpy()
        shot = pkg.capi.shot_lrf(ctx, b.cloud, b.kp_off, *b.tk, s.radius).cpu().numpy()
    finally:
        ctx.sync(); b.close()
    return na, shot


def sign_relation(na, shot):
    """asserts the bit relation of the two frames and returns s per keypoint (0 on NaN rows)"""
    assert na.shape == shot.shape and np.array_equal(np.isnan(na), np.isnan(shot))
    nan = np.isnan(na[:, 0])
    assert np.array_equal(np.isnan(na).all(1), nan)
    a, b = na[~nan], shot[~nan]
    assert np.array_equal(a[:, :3].view(np.uint32), b[:, :3].view(np.uint32))
    same = (a[:, 6:9].view(np.uint32) == b[:, 6:9].view(np.uint32)).all(1)
    opposite = (a[:, 6:9].view(np.uint32) == (-b[:, 6:9]).view(np.uint32)).all(1)
    assert (same ^ opposite).all()
    sgn = np.where(same, 1.0, -1.0).astype(np.float32)
    assert np.array_equal(a[:, 3:6].view(np.uint32), (sgn[:, None] * b[:, 3:6]).view(np.uint32))
    out = np.zeros(len(na), np.float32); out[~nan] = sgn
    return out


def assert_matches_restatement(got, r):
    """NaN pattern exact; x and z along the restatement's wherever that sign is decided; within 1e-5 per component where both are"""
    nan = np.isnan(r["frame"][:, 0])
    assert np.array_equal(np.isnan(got), np.isnan(r["frame"]))
    assert (r["gap"][~nan] >= 1e-3).all()
    dx = (got[:, 0:3].astype(np.float64) * r["frame"][:, 0:3]).sum(1)
    dz = (got[:, 6:9].astype(np.float64) * r["frame"][:, 6:9]).sum(1)
    okx, okz = ~nan & r["decided_x"], ~nan & r["decided_z"]
    assert (dx[okx] > 0.99).all(), np.nonzero(okx & ~(dx > 0.99))[0]
    assert (dz[okz] > 0.99).all(), np.nonzero(okz & ~(dz > 0.99))[0]
    both = okx & okz
    err = np.abs(got[both] - r["frame"][both]).max() if both.any() else 0.0
    print(f"{int(both.sum())} of {int((~nan).sum())} valid keypoints decided, max |device - restatement| {err:.3g}")
    assert err <= LRF_TOL
    return both


# ------------------------------------------------------------------------------------------------ 1. generic
@pytest.mark.parametrize("negated", [False, True], ids=["outward", "negated"])
def test_generic_scene(pkg, gpu, negated):
    ctx, dev = gpu
    s = sc.get(sc.generic, negated)
    na, shot = both_frames(pkg, ctx, dev, s)
    sgn = sign_relation(na, shot)
    assert np.isfinite(na).all() and len(na) == 64
    assert_matches_restatement(na, s.reference())
    assert_matches_restatement(shot, s.reference(False))
    assert (sgn == (1.0 if negated else -1.0)).all()


# ------------------------------------------------------------------------------------------------ 2. ragged batch
def test_ragged_batch_and_block_order(pkg, gpu, monkeypatch):
    ctx, dev = gpu
    s = sc.get(sc.ragged)
    na, shot = both_frames(pkg, ctx, dev, s)
    sign_relation(na, shot)
    r = s.reference()
    assert np.isnan(r["frame"][:, 0]).sum() == 7
    assert_matches_restatement(na, r)
    monkeypatch.setenv("ISMHIP_XCD_MAP", "0")
    ctx2 = pkg.capi.Ctx(0)                                                  # the switch is read when a context is created
    try:
        na2, shot2 = both_frames(pkg, ctx2, dev, s)
    finally:
        ctx2.close()
    assert na2.tobytes() == na.tobytes() and shot2.tobytes() == shot.tobytes()


# ------------------------------------------------------------------------------------------------ 3. counts exact to one vote
@pytest.mark.parametrize("m", sc.MIRROR_M)
def test_mirror_counts_are_exact_to_one_vote(pkg, gpu, m):
    ctx, dev = gpu
    z = {}
    for kind in sc.MIRROR_SETS:
        s = sc.get(sc.mirror, m, kind)
        na, shot = both_frames(pkg, ctx, dev, s)
        sign_relation(na, shot)
        r = s.reference()
        assert r["decided"].all() and r["valid"][0] == 2 * m
        assert_matches_restatement(na, r)
        z[kind] = na[0, 6:9]
    assert np.array_equal(z["half-minus"], -z["half-plus"]) and np.array_equal(z["half"], z["mirrored"])
    assert np.array_equal(z["half"], z["half-plus"]) != np.array_equal(z["half"], z["half-minus"])


# ------------------------------------------------------------------------------------------------ 4. several candidate windows
@pytest.mark.parametrize("deal", [None] + list(sc.DENSE_DEALS), ids=lambda d: d or "own-normals")
def test_dense_ball_keeps_position_and_normal_paired(pkg, gpu, deal):
    ctx, dev = gpu
    s = sc.get(sc.dense, deal)
    na, shot = both_frames(pkg, ctx, dev, s)
    sign_relation(na, shot)
    r = s.reference()
    assert r["valid"].max() > 20000 and (deal is None or abs(r["plusN"][0]) == abs(sc.DENSE_DEALS[deal]))
    both = assert_matches_restatement(na, r)
    assert both.all()


# ------------------------------------------------------------------------------------------------ 5. the cloud's current normals
def test_the_normals_the_cloud_holds_now_are_read(pkg, gpu):
    import torch
    ctx, dev = gpu
    s = sc.get(sc.generic, False, (0.3, -0.2, 3.0))                          # away from the origin: orientation 0 flips towards it
    pt_off, p, n, kp_off, kp = s.soa()
    b = Batch(pkg, ctx, dev, [(p, np.zeros_like(p))], s.kps, s.cell)
    try:
        zero = pkg.capi.shotna_lrf(ctx, b.cloud, b.kp_off, *b.tk, s.radius).cpu().numpy()
        nx, ny, nz = (torch.empty(len(p), dtype=torch.float32, device=dev) for _ in range(3))
        pkg.capi.estimate_normals_pca(ctx, b.cloud, 0.15, 0, nx, ny, nz)
        na = pkg.capi.shotna_lrf(ctx, b.cloud, b.kp_off, *b.tk, s.radius).cpu().numpy()
        shot = pkg.capi.shot_lrf(ctx, b.cloud, b.kp_off, *b.tk, s.radius).cpu().numpy()
        dev_n = torch.stack([nx, ny, nz], 1).cpu().numpy()
    finally:
        ctx.sync(); b.close()
    assert np.isfinite(dev_n).all()
    r0 = s.reference(normals=np.zeros_like(p))                               # zero normals: every vote is a plus
    assert (r0["plusN"] == 2 * r0["in_ball"] - r0["valid"]).all()
    sgn = sign_relation(na, shot)
    r = s.reference(normals=dev_n)
    both = assert_matches_restatement(na, r)
    assert both.sum() >= 60                                                  # of 64: the comparison is not an empty one
    assert_matches_restatement(zero, r0)
    assert (sgn == 1).any() and (sgn == -1).any() and not np.array_equal(zero, na)   # the far side of the surface looks away from the origin


# ------------------------------------------------------------------------------------------------ 6. descriptors and the host
def test_shot352_on_shotna_frames(pkg, gpu, ora):
    ctx, dev = gpu
    s = sc.get(sc.generic, False)
    b = Batch(pkg, ctx, dev, s.objs, s.kps, s.cell)
    try:
        lrf = pkg.capi.shotna_lrf(ctx, b.cloud, b.kp_off, *b.tk, s.radius)
        got, cnt = pkg.capi.shot352(ctx, b.cloud, b.kp_off, *b.tk, lrf, 0.4, want_counts=True)
        got, cnt, lrf = got.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), lrf.cpu().numpy()
    finally:
        ctx.sync(); b.close()
    want, wcnt = ora.shot352(b.pt_off, *fs.cols(b.p), *fs.cols(b.n), b.kp_off, *fs.cols(b.kp), lrf, 0.4)
    assert np.array_equal(cnt, wcnt) and np.isfinite(want).all()
    assert_close_nan(got, want, TOL)


def _train_host(train, order, frame_type):
    m = hb.Model()
    m.config_from_json(_cfg(**{"Children/Features/Parameters/ReferenceFrameType": frame_type}))
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    return m


def test_shotna_end_to_end_through_host_and_driver(pkg, gpu, tmp_path):
    """a SHOT model with ReferenceFrameType "SHOTNA" trained on three synthetic classes by the C++ host: the codebook is the Python
    driver's with lrf_type="SHOTNA" and differs from the "SHOT" one, the model survives write / read with the key intact, and both
    label the training shapes correctly with the same maxima"""
    ctx, dev = gpu
    train, _ = _dataset(pkg, 3, 9, 6)
    order = sorted(range(9), key=lambda i: (train.label(i), i))
    m = _train_host(train, order, "SHOTNA")
    rec = pkg.pipeline.Recognizer(ctx, pkg.pipeline.IsmConfig(n_classes=3, lrf_type="SHOTNA"))
    cb = rec.train([pkg.pipeline.DeviceBatch(train.batch(order), dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(352, 3)
    assert words.shape == cb["words"].shape and len(words) > 100
    # the tolerances of test_host_train_write_read_detect_matches_python_harness (1-ulp keypoint differences between the two hosts)
    np.testing.assert_allclose(words, cb["words"], atol=2e-5)
    np.testing.assert_allclose(vxyz, cb["vote_xyz"], atol=1e-4)
    assert np.array_equal(vcls, cb["vote_class"])
    plain = _train_host(train, order, "SHOT")
    pw = plain.codebook(352, 3)[0]
    assert pw.shape != words.shape or np.abs(pw - words).max() > 1e-2
    plain.close()
    path = str(tmp_path / "shotna.ism")
    m.write(path)
    assert json.load(open(path))["ObjectConfig"]["Children"]["Features"]["Parameters"]["ReferenceFrameType"] == "SHOTNA"
    m2 = hb.Model()
    m2.read(path)
    assert json.loads(m2.config_to_json())["Children"]["Features"]["Parameters"]["ReferenceFrameType"] == "SHOTNA"
    assert m2.codebook_size() == m.codebook_size() and np.array_equal(m2.codebook(352, 3)[0], words)
    nb = train.batch(order)
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    assert (got["cls"][:, 0] == nb["labels"]).all()
    assert np.array_equal(want["cls"][:, 0].cpu().numpy(), got["cls"][:, 0])
    np.testing.assert_allclose(got["weight"][:, 0], want["weight"][:, 0].cpu().numpy(), rtol=1e-3)
    m.close(); m2.close()
