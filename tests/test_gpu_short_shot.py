"""SHORT_SHOT on the device (-m gpu): ismhip_short_shot through capi on the cases of short_shot_scenes.py against the restatement
short_shot_ref.py, on the frames the device itself estimates (or the frames a scene supplies). Every keypoint of every case is
compared, none exempted: descriptors to the project's 1e-4, neighbour counts and the NaN pattern exactly. test_short_shot_cpu.py proves
on the host that the scenes keep clear of the hard bin decisions and reach their paths. Then the codeword search at the short
dimensions (never exercised below 33) and the descriptor end to end through the C++ host and the Python driver."""
import json
import os

import numpy as np
import pytest

import frontend_scenes as fs
import host_binding as hb
import short_shot_scenes as sss
from test_gpu_frontend import TOL, Batch, T, assert_close_nan
from test_gpu_parity import _cb
from test_host_layer import _dataset

pytestmark = pytest.mark.gpu
_frames = {}


def run_case(pkg, gpu, case):
    """-> (device rows, device counts, the frames used, the case's batch closed again)"""
    ctx, dev = gpu
    s = Batch(pkg, ctx, dev, case.objs, case.kps, case.cell)
    try:
        key = (id(case.objs), case.radius)
        if case.frames is None and key not in _frames:
            _frames[key] = pkg.capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, case.radius).cpu().numpy()
        frames = case.frames_from(_frames.get(key))
        got, cnt = pkg.capi.short_shot(ctx, s.cloud, s.kp_off, *s.tk, T(frames, dev), case.radius, bins=case.bins, min_radius=case.min_radius,
                                       log_radius=case.log_radius, want_counts=True)
        return got.cpu().numpy(), cnt.cpu().numpy().astype(np.int64), frames
    finally:
        s.close()


def check_rows(got, cnt, want, wcnt, dim):
    """device rows and counts against the restatement's: shape, exact counts and NaN pattern, values within TOL, finite rows of unit norm"""
    assert got.shape == (len(want), dim)
    assert np.array_equal(cnt, wcnt)
    assert_close_nan(got, want, TOL)
    finite = ~np.isnan(want).any(1)
    if finite.any():
        assert np.abs(np.linalg.norm(got[finite].astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("case", sss.all_cases(), ids=lambda c: c.name)
def test_short_shot_matches_the_restatement(pkg, gpu, case):
    """the four grids on the mid object (a keypoint on a cloud point, a NaN frame row, an empty ball inside the grid and one off the
    grid), on the nine-object thin batch (XCD block map, ragged keypoints, balls of 54 000 neighbours) and on the queue clusters (4 to
    129 neighbours: the queue boundaries, and counts below SHOT's five that still give a descriptor); logarithmic radius, UseMinRadius,
    a minimum radius above every neighbour (NaN rows with their counts); the dyadic lattice in two frames"""
    got, cnt, frames = run_case(pkg, gpu, case)
    want, wcnt, frac, switch = case.reference(frames)
    finite = ~np.isnan(want).any(1)
    err = np.abs(got[finite] - want[finite]).max() if finite.any() else 0.0
    print(f"{case.name}: {finite.sum()} of {len(want)} rows finite, max |device - restatement| {err:.3g}, switch margin on these frames {switch.min():.3g}")
    check_rows(got, cnt, want, wcnt, case.bins[0] * case.bins[1] * case.bins[2])
    if case.name.startswith("queue") and case.min_radius_relative < 0.9:
        assert finite.all() and wcnt.min() == 4


def test_short_shot_is_bitwise_reproducible(pkg, gpu):
    """integer accumulation: the same call twice gives the same bits, whatever order the neighbours arrive in (and the "short_shot" timer counts both)"""
    ctx, _ = gpu
    case = sss.thin_case((2, 2, 8))
    ctx.timers_enable(True); ctx.timers_reset()
    a, ca, _ = run_case(pkg, gpu, case)
    b, cb, _ = run_case(pkg, gpu, case)
    ctx.sync()
    ms, launches = ctx.timer("short_shot")
    ctx.timers_enable(False)
    assert launches == 2 and ms > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca, cb)


def test_short_shot_refusals(pkg, gpu):
    ctx, dev = gpu
    case = sss.queue_case((2, 2, 8))
    s = Batch(pkg, ctx, dev, case.objs, case.kps, case.cell)
    call = lambda **kw: pkg.capi.short_shot(ctx, s.cloud, s.kp_off, *s.tk, T(case.frames, dev), case.radius, **kw)
    try:
        with pytest.raises(pkg.capi.IsmHipError, match=r"\(-4\).*more than 256 bins"):        # ISMHIP_ERR_UNSUPPORTED
            call(bins=(8, 8, 8))
        with pytest.raises(pkg.capi.IsmHipError, match="fewer than one bin"):
            call(bins=(2, 0, 8))
        with pytest.raises(pkg.capi.IsmHipError, match="logarithmic radius"):
            call(log_radius=True, min_radius=0.0)
        with pytest.raises(pkg.capi.IsmHipError, match="logarithmic radius"):
            call(log_radius=True, min_radius=case.radius)
        assert call(bins=(8, 4, 8)).shape == (len(case.kps[0]), 256)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ codeword search at short dims
_rows = {}


def short_rows(pkg, gpu, bins):
    """~5000 SHORT_SHOT rows of the mid object: 4000 codewords and 1000 queries (NaN rows dropped)"""
    if bins not in _rows:
        ctx, dev = gpu
        p, n, rng = fs.mid_object()
        kp = p[rng.choice(len(p), 5200, replace=False)]
        s = Batch(pkg, ctx, dev, [(p, n)], [kp], sss.MID_CELL)
        try:
            lrf = pkg.capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, sss.MID_RADIUS)
            rows = pkg.capi.short_shot(ctx, s.cloud, s.kp_off, *s.tk, lrf, sss.MID_RADIUS, bins=bins).cpu().numpy()
        finally:
            s.close()
        rows = rows[np.isfinite(rows).all(1)]
        assert len(rows) >= 5000
        _rows[bins] = (rows[:4000].copy(), rows[4000:5000].copy())
    return _rows[bins]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("bins", [(1, 1, 8), (1, 3, 5), (2, 2, 8)], ids=["D8", "D15", "D32"])
def test_knn_on_short_shot_rows(pkg, gpu, ora, metric, bins):
    """ismhip_knn at D = 8, 15, 32 (below the 33 of FPFH no dimension had been searched): non-negative unit rows of real descriptors,
    near-duplicates included; indices equal and distances bit-equal to the oracle's exact search, as test_gpu_parity holds the others"""
    ctx, dev = gpu
    words, q = short_rows(pkg, gpu, bins)
    q = q.copy(); q[:5] = words[:5]                                        # exact hits: distance 0
    host, cb = _cb(pkg, gpu, words)
    for k in (1, 3):
        idx, dist = pkg.capi.knn(ctx, cb, metric, T(q, dev), k)
        widx, wdist = ora.knn(metric, words, q, k)
        assert np.array_equal(idx.cpu().numpy(), widx)
        assert np.array_equal(dist.cpu().numpy(), wdist)
    cb.close()


# ------------------------------------------------------------------------------------------------ end to end
def _short_model_cfg(**codebook):
    j = json.load(open(os.path.join(hb.ROOT, "config", "modelnet10_short_shot.ism")))["ObjectConfig"]
    j["Children"]["Codebook"]["Parameters"].update(codebook)
    return json.dumps(j)


def test_short_shot_end_to_end_through_host_and_driver(pkg, gpu, tmp_path):
    """a SHORT_SHOT model (32 bins) trained on three synthetic classes by the C++ host: the codebook has dim 32 and is the Python
    driver's, the model survives write / read, and both label the training shapes correctly with the same maxima"""
    ctx, dev = gpu
    train, _ = _dataset(pkg, 3, 9, 6)
    order = sorted(range(9), key=lambda i: (train.label(i), i))
    m = hb.Model()
    m.config_from_json(_short_model_cfg())
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    cfg = pkg.pipeline.IsmConfig(n_classes=3, feature="SHORT_SHOT")
    assert cfg.dim == 32
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(train.batch(order), dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(32, 3)
    assert words.shape == cb["words"].shape and words.shape[1] == 32 and len(words) > 100
    # The two hosts compute the voxel-grid keypoints with different accumulation widths (float vs double); a 1-ulp keypoint difference
    # moves SHOT entries by a few 1e-6 (the 2e-5 of test_host_train_write_read_detect_matches_python_harness). This histogram is not
    # continuous: the same ulp can carry one neighbour across a switch and move a whole deposit of its row (~1 / neighbours). Expected
    # flips: ~1e-7 raw units x 6 thresholds per neighbour x ~2e5 neighbours = ~0.1 per run, so at most 1 % of the rows may differ.
    row_err = np.abs(words - cb["words"]).max(1)
    assert (row_err <= 2e-5).mean() >= 0.99, row_err.max()
    assert np.array_equal(vcls, cb["vote_class"])
    path = str(tmp_path / "short.ism")
    m.write(path)
    saved = json.load(open(path))
    assert saved["ObjectConfig"]["Children"]["Features"]["Type"] == "SHORT_SHOT" and os.path.exists(str(tmp_path / "short.ismd"))
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(32, 3)[0], words)
    nb = train.batch(order)
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    assert (got["cls"][:, 0] == nb["labels"]).all()
    assert np.array_equal(want["cls"][:, 0].cpu().numpy(), got["cls"][:, 0])
    np.testing.assert_allclose(got["weight"][:, 0], want["weight"][:, 0].cpu().numpy(), rtol=1e-3)
    m.close(); m2.close()


def test_partial_shot_stays_refused_for_short_shot(pkg, gpu):
    """UsePartialShot keeps signatures of SHOT-352: with any other descriptor the host refuses it, as does the driver"""
    ctx, dev = gpu
    train, _ = _dataset(pkg, 3, 9, 6)
    m = hb.Model()
    m.config_from_json(_short_model_cfg(UsePartialShot=True))
    o = train.get(0)
    m.add_training(o["xyz"], o["normals"], o["label"], 0)
    with pytest.raises(hb.HostError, match="SHOT-352"):
        m.train()
        nb = train.batch([0])
        m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
    m.close()
    rec = pkg.pipeline.Recognizer(ctx, pkg.pipeline.IsmConfig(n_classes=3, feature="SHORT_SHOT", use_partial_shot=True))
    with pytest.raises(pkg.capi.IsmHipError, match="SHOT-352"):
        rec.train([pkg.pipeline.DeviceBatch(train.batch([0]), dev)], instance_ids=[0])
