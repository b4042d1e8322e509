"""SHORT_CSHOT on the device (-m gpu): ismhip_short_cshot through capi on the cases of short_cshot_scenes.py against the restatement
short_cshot_ref.py, on the frames the device itself estimates (or the frames a scene supplies). Every keypoint of every case is
compared, none exempted: descriptors to the project's 1e-4, neighbour counts and the NaN pattern exactly. test_short_cshot_cpu.py
proves on the host that the scenes keep clear of the hard geometric bin decisions of both grids and reach their paths. Then the
codeword search on real rows at D = 512 and D = 71, and the descriptor end to end through the C++ host and the Python driver."""
import json
import os

import numpy as np
import pytest

import frontend_scenes as fs
import host_binding as hb
import short_cshot_ref as scr
import short_cshot_scenes as scs
import short_shot_scenes as sss
from test_gpu_frontend import TOL, Batch, T, assert_close_nan
from test_gpu_host_routes import _split
from test_gpu_parity import _cb
from test_gpu_short_shot import check_rows

pytestmark = pytest.mark.gpu
_frames = {}


def run_case(pkg, gpu, case, **over):
    """-> (device rows, device counts, the frames used); the case's batch is closed again"""
    ctx, dev = gpu
    geo = case.geo
    s = Batch(pkg, ctx, dev, geo.objs, geo.kps, geo.cell, case.rgba, case.kp_rgba)
    try:
        key = (id(geo.objs), geo.radius)
        if geo.frames is None and key not in _frames:
            _frames[key] = pkg.capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, geo.radius).cpu().numpy()
        frames = geo.frames_from(_frames.get(key))
        kw = dict(bins=geo.bins, color_bins=case.color_bins, hist_size=case.hist_size, min_radius=geo.min_radius, log_radius=geo.log_radius)
        kw.update(over)
        got, cnt = pkg.capi.short_cshot(ctx, s.cloud, s.kp_off, *s.tk, s.t_kp_rgba, T(frames, dev), geo.radius, want_counts=True, **kw)
        return got.cpu().numpy(), cnt.cpu().numpy().astype(np.int64), frames
    finally:
        s.close()


@pytest.mark.parametrize("case", scs.parity_cases(), ids=lambda c: c.name)
def test_short_cshot_matches_the_restatement(pkg, gpu, ora, case):
    """the mid object (a keypoint on a cloud point, a NaN frame row, an empty ball inside the grid and one off the grid) at the default
    512 bins, with single-bin axes and H = 1 (16 bins), at 1216 bins on two different grids, and at 71 bins (no multiple of 4); the
    nine-object thin batch (XCD block map, ragged keypoint runs, balls of 54 000 neighbours); the queue clusters (4 to 129 neighbours),
    also with UseMinRadius 0.4 and 0.9 (NaN rows with their counts); logarithmic radius; the dyadic lattice in two frames with the
    colour edge list on its innermost points; the palette object (cd = 0, black, white)"""
    got, cnt, frames = run_case(pkg, gpu, case)
    want, wcnt, switch = case.reference(ora.rgb2lab, frames)
    finite = ~np.isnan(want).any(1)
    err = np.abs(got[finite] - want[finite]).max() if finite.any() else 0.0
    print(f"{case.name}: {finite.sum()} of {len(want)} rows finite, max |device - restatement| {err:.3g}, switch margin on these frames {switch.min():.3g}")
    check_rows(got, cnt, want, wcnt, case.dim)
    if case.geo.name.startswith("queue") and case.geo.min_radius_relative < 0.9:
        assert finite.all() and wcnt.min() == 4


def test_short_cshot_is_bitwise_reproducible(pkg, gpu):
    """integer accumulation: the same call twice gives the same bits, whatever order the neighbours arrive in (and the "short_cshot" timer counts both)"""
    ctx, _ = gpu
    case = scs.thin_case()
    ctx.timers_enable(True); ctx.timers_reset()
    a, ca, _ = run_case(pkg, gpu, case)
    b, cb, _ = run_case(pkg, gpu, case)
    ctx.sync()
    ms, launches = ctx.timer("short_cshot")
    ctx.timers_enable(False)
    assert launches == 2 and ms > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca, cb)


def test_short_cshot_refusals(pkg, gpu):
    """every refusal of the ABI table, by status and message; then a row of exactly 1344 bins is computed"""
    ctx, dev = gpu
    case = scs.queue_case()
    geo = case.geo
    Err = pkg.capi.IsmHipError
    s = Batch(pkg, ctx, dev, geo.objs, geo.kps, geo.cell, case.rgba, case.kp_rgba)
    plain = Batch(pkg, ctx, dev, geo.objs, geo.kps, geo.cell)                               # a cloud made without colours
    call = lambda b=s, kp_rgba=s.t_kp_rgba, **kw: pkg.capi.short_cshot(ctx, b.cloud, b.kp_off, *b.tk, kp_rgba, T(geo.frames, dev), geo.radius, **kw)
    try:
        for kw in (dict(bins=(2, 0, 8)), dict(color_bins=(2, 2, 0)), dict(color_bins=(-1, 2, 8))):
            with pytest.raises(Err, match=r"\(-1\).*fewer than one bin"):                   # ISMHIP_ERR_INVALID
                call(**kw)
        with pytest.raises(Err, match=r"\(-1\).*colour histogram of fewer than one bin"):
            call(hist_size=0)
        with pytest.raises(Err, match=r"\(-4\).*more than 256 shape bins"):                 # ISMHIP_ERR_UNSUPPORTED
            call(bins=(8, 8, 8))
        with pytest.raises(Err, match=r"\(-4\).*longer than 1344"):
            call(bins=(8, 4, 8), color_bins=(2, 4, 8), hist_size=18)                        # 256 + 64 * 18 = 1408
        with pytest.raises(Err, match=r"\(-4\).*longer than 1344"):
            call(color_bins=(4, 4, 8), hist_size=15)                                        # 32 + 128 * 15 = 1952
        with pytest.raises(Err, match=r"\(-1\).*colour arrays missing"):
            call(b=plain)
        with pytest.raises(Err, match=r"\(-1\).*colour arrays missing"):
            call(kp_rgba=None)
        for mr in (0.0, geo.radius):
            with pytest.raises(Err, match=r"\(-1\).*logarithmic radius"):
                call(log_radius=True, min_radius=mr)
        for mr in (-0.1, float("nan"), float("inf")):
            with pytest.raises(Err, match=r"\(-1\).*bad argument"):
                call(min_radius=mr)
        got = call(bins=(8, 4, 8), color_bins=(2, 4, 8), hist_size=17)                      # 256 + 64 * 17 = 1344 exactly
        assert got.shape == (len(geo.kps[0]), 1344) and bool(np.isfinite(got.cpu().numpy()).all())
    finally:
        s.close(); plain.close()


# ------------------------------------------------------------------------------------------------ codeword search on real rows
_rows = {}


def short_rows(pkg, gpu, cfg):
    """~5000 SHORT_CSHOT rows of the mid object with random colours: 4000 codewords and 1000 queries (NaN rows dropped)"""
    if cfg not in _rows:
        ctx, dev = gpu
        p, n, rng = fs.mid_object()
        sel = rng.choice(len(p), 5200, replace=False)
        crng = np.random.default_rng(75)
        rgba = crng.integers(0, 1 << 24, size=len(p)).astype(np.uint32)
        s = Batch(pkg, ctx, dev, [(p, n)], [p[sel]], sss.MID_CELL, [rgba], [rgba[sel]])
        try:
            lrf = pkg.capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, sss.MID_RADIUS)
            rows = pkg.capi.short_cshot(ctx, s.cloud, s.kp_off, *s.tk, s.t_kp_rgba, lrf, sss.MID_RADIUS, bins=cfg[0], color_bins=cfg[1],
                                        hist_size=cfg[2]).cpu().numpy()
        finally:
            s.close()
        rows = rows[np.isfinite(rows).all(1)]
        assert len(rows) >= 5000
        _rows[cfg] = (rows[:4000].copy(), rows[4000:5000].copy())
    return _rows[cfg]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("cfg", [scs.MID_CONFIGS[0], scs.MID_CONFIGS[3]], ids=["D512", "D71"])
def test_knn_on_short_cshot_rows(pkg, gpu, ora, metric, cfg):
    """ismhip_knn on real SHORT_CSHOT rows at D = 512 and D = 71 (no multiple of 4), 4000 words and 1000 queries with five exact hits:
    indices equal and distances bit-equal to the oracle's exact search, as test_knn_on_short_shot_rows holds the short dimensions"""
    ctx, dev = gpu
    words, q = short_rows(pkg, gpu, cfg)
    assert words.shape[1] == scr.total_dims(*cfg)
    q = q.copy(); q[:5] = words[:5]                                        # exact hits: distance 0
    host, cb = _cb(pkg, gpu, words)
    for k in (1, 3):
        idx, dist = pkg.capi.knn(ctx, cb, metric, T(q, dev), k)
        widx, wdist = ora.knn(metric, words, q, k)
        assert np.array_equal(idx.cpu().numpy(), widx)
        assert np.array_equal(dist.cpu().numpy(), wdist)
    cb.close()


# ------------------------------------------------------------------------------------------------ end to end
def _model_cfg(**codebook):
    """the value set of config/kinect_short_cshot.ism with its lengths (Radius, ReferenceFrameRadius, LeafSize, Bandwidth: those of
    0.15-unit Kinect views) replaced by the ones that fit the unit-sized synthetic shapes"""
    j = json.load(open(os.path.join(hb.ROOT, "config", "kinect_short_cshot.ism")))["ObjectConfig"]
    j["Children"]["Features"]["Parameters"].update(Radius=0.4, ReferenceFrameRadius=0.3)
    j["Children"]["Keypoints"]["Parameters"]["LeafSize"] = 0.2
    j["Children"]["Voting"]["Parameters"]["Bandwidth"] = 0.6
    j["Children"]["Codebook"]["Parameters"].update(codebook)
    return json.dumps(j)


def _driver_cfg(pkg, **kw):
    return pkg.pipeline.IsmConfig(n_classes=3, feature="SHORT_CSHOT", distance="ChiSquared", radius=0.4, lrf_radius=0.3, bandwidth=0.6, **kw)


def test_short_cshot_end_to_end_through_host_and_driver(pkg, gpu, tmp_path):
    """A SHORT_CSHOT model (512 bins, chi-square) trained on three coloured synthetic classes by the C++ host: the codebook has dim 512
    and as many words and the same vote classes as the Python driver's, the model survives write / read bit for bit, and both hosts label
    the training shapes correctly, with equal top classes.
    The two hosts' codebook ROWS are not asserted equal: their voxel-grid keypoint COLOURS come from different centroid code (each
    channel's mean is truncated to 8 bits after differently accumulated sums), and one colour step of a keypoint changes the colour
    distance to EVERY neighbour, so it can move deposits all over the 480 colour bins of the row, while the 32 shape bins only see the
    few-1e-6 effect of a 1-ulp keypoint position. The share of rows within 2e-5 is printed (on this split, when the test was written:
    1.000 of 1924 rows, largest difference 1.4e-6 -- no keypoint colour differed)."""
    ctx, dev = gpu
    train, _, order = _split(pkg, with_color=True)
    m = hb.Model()
    m.config_from_json(_model_cfg())
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i, rgba=o["rgba"])
    m.train()
    cfg = _driver_cfg(pkg)
    assert cfg.dim == 512
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(train.batch(order), dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(512, 3)
    assert words.shape == cb["words"].shape and words.shape[1] == 512 and len(words) > 100
    assert np.array_equal(vcls, cb["vote_class"])
    row_err = np.abs(words - cb["words"]).max(1)
    shape_err = np.abs(words[:, :32] - cb["words"][:, :32]).max(1)
    print(f"codebook rows of the two hosts within 2e-5: {(row_err <= 2e-5).mean():.3f} of {len(words)} (largest difference {row_err.max():.3g}; "
          f"shape part alone {(shape_err <= 2e-5).mean():.3f})")
    path = str(tmp_path / "short_cshot.ism")
    m.write(path)
    saved = json.load(open(path))
    assert saved["ObjectConfig"]["Children"]["Features"]["Type"] == "SHORT_CSHOT" and os.path.exists(str(tmp_path / "short_cshot.ismd"))
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(512, 3)[0].view(np.uint32), words.view(np.uint32))
    nb = train.batch(order)
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8, rgba=nb["rgba"])
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    assert (got["cls"][:, 0] == nb["labels"]).all()
    assert np.array_equal(want["cls"][:, 0].cpu().numpy(), got["cls"][:, 0])
    m.close(); m2.close()


def test_partial_shot_stays_refused_for_short_cshot(pkg, gpu):
    """UsePartialShot keeps signatures of SHOT-352: with any other descriptor the host refuses it, as does the driver"""
    ctx, dev = gpu
    train, _, order = _split(pkg, with_color=True)
    m = hb.Model()
    m.config_from_json(_model_cfg(UsePartialShot=True))
    o = train.get(0)
    m.add_training(o["xyz"], o["normals"], o["label"], 0, rgba=o["rgba"])
    with pytest.raises(hb.HostError, match="SHOT-352"):
        m.train()
        nb = train.batch([0])
        m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8, rgba=nb["rgba"])
    m.close()
    rec = pkg.pipeline.Recognizer(ctx, _driver_cfg(pkg, use_partial_shot=True))
    with pytest.raises(pkg.capi.IsmHipError, match="SHOT-352"):
        rec.train([pkg.pipeline.DeviceBatch(train.batch([0]), dev)], instance_ids=[0])
