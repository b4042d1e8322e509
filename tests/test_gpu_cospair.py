"""CoSPAIR on the device (-m gpu): ismhip_cospair through capi on the scenes of cospair_scenes.py against the float64 interval
reference cospair_ref.py. Snap indices, level and pair counts and NaN patterns are equal; every decided entry is BIT-equal (the row
is two float operations on exact integer counts); an undecided entry lies between the values of its count bounds. test_cospair_cpu.py
proves on the host that the scenes reach their decisions and how little they leave undecided. Then reproducibility and the timer, the
refusals, the codeword search on real rows at D = 378, and the descriptor end to end through the C++ host and the Python driver."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cospair_ref as cr
import cospair_scenes as cs
import frontend_scenes as fs
import host_binding as hb
import short_shot_scenes as sss
from test_gpu_frontend import Batch, T
from test_gpu_host_routes import _split
from test_gpu_parity import _cb

pytestmark = pytest.mark.gpu


def run_scene(pkg, gpu, name):
    """-> (rows [K, 378], pair counts [K], level counts [K, 7], snap indices [K], -1 for a NaN row); the scene's batch is closed again"""
    ctx, dev = gpu
    s = cs.scene(name)
    b = Batch(pkg, ctx, dev, s["objs"], s["kps"], s["cell"], s["rgba"])
    try:
        got, cnt, lev, snap = pkg.capi.cospair(ctx, b.cloud, b.kp_off, *b.tk, s["radius"], want_counts=True, want_levels=True, want_snap=True)
        return got.cpu().numpy(), cnt.cpu().numpy().astype(np.int64), lev.cpu().numpy().astype(np.int64), snap.cpu().numpy().astype(np.int64)
    finally:
        b.close()


def counts_of(got, n):
    """the integer counts behind a row: rint(v n / l) per entry"""
    lev = np.repeat(np.arange(1, cr.LEVELS + 1), cr.LEVEL)[None, :].astype(np.float64)
    return np.rint(got.astype(np.float64) * np.repeat(n, cr.LEVEL, axis=1) / lev).astype(np.int64)


def check_rows(ref, got, cnt, lev, snap):
    """device rows, pair counts, level counts and snap indices against cospair_ref.Result: everything integer exact, NaN rows as a whole,
    decided entries bit for bit, the others inside their interval, 3 n deposits per level and half -> rows with an undecided deposit"""
    assert got.shape == (len(ref.nan), cr.DIM)
    assert np.array_equal(snap, ref.snap)
    assert np.array_equal(lev, ref.n) and np.array_equal(cnt, ref.n.sum(1))
    assert np.array_equal(np.isnan(got), np.repeat(ref.nan[:, None], cr.DIM, axis=1))
    live = ~ref.nan
    decided = (ref.lo == ref.hi) & live[:, None]
    assert np.array_equal(got.view(np.uint32)[decided], ref.want_lo.view(np.uint32)[decided])
    open_ = ~decided & live[:, None]
    assert ((got[open_] >= ref.want_lo[open_]) & (got[open_] <= ref.want_hi[open_])).all()
    c = counts_of(got[live], ref.n[live]).reshape(-1, cr.LEVELS, 2, cr.BLOCK).sum(3)
    assert np.array_equal(c[:, :, 0], 3 * ref.n[live]) and np.array_equal(c[:, :, 1], 3 * ref.n[live])
    return int((~ref.decided_row & live).sum())


@pytest.mark.parametrize("name", list(cs.SCENES))
def test_cospair_matches_the_interval_reference(pkg, gpu, ora, name):
    """shells (points exactly on r_l, an empty level, coincident duplicates, snap ties, a keypoint 100 radii away), queue (1 .. 129
    pairs), the hard decisions (spills of f1 = +pi and f2 = -1, the pole, a vanishing cross product: asserted entry by entry; the seam,
    role-tie and degenerate constructions of the FPFH scenes), the palette, one colour on 4 000 neighbours, the nine-object thin batch
    (ragged runs, no keypoints, one point, a NaN normal at the snapped point, a NaN keypoint, a ball of >= 50 000 pairs), generic"""
    got, cnt, lev, snap = run_scene(pkg, gpu, name)
    ref = cs.reference(name, ora.rgb2lab)
    und_rows = check_rows(ref, got, cnt, lev, snap)
    live = ~ref.nan
    print(f"{name}: {live.sum()} rows, {und_rows} with an undecided deposit ({und_rows / max(live.sum(), 1):.3f}), {ref.n.sum()} pairs")
    if name == "hard":
        geo = counts_of(got, ref.n).reshape(-1, cr.LEVELS, 2, cr.BLOCK)[:, :, 0, :]
        for (o, level), want in cs.scene(name)["want"].items():          # one keypoint per object: row o
            assert {int(i): int(geo[o, level, i]) for i in np.nonzero(geo[o, level])[0]} == want, (o, level)
    if name == "hard_seam":
        geo = counts_of(got, ref.n).reshape(-1, cr.LEVELS, 2, cr.BLOCK)[:, :, 0, :]
        # y = +2^-12 / -2^-12 with x < 0: f1 a hair below +pi (bin 8) / above -pi (bin 0) for all three pairs; y = -0.0: -pi, bin 0
        assert geo[0, :, :cr.BINS].sum(0).tolist() == [0] * 8 + [3] and geo[1, :, :cr.BINS].sum(0).tolist() == [3] + [0] * 8
        assert geo[4, :, :cr.BINS].sum(0).tolist() == [3] + [0] * 8
    if name == "thin":
        s = cs.scene(name)
        assert ref.nan.nonzero()[0].tolist() == s["nan_rows"] and ref.n[s["big_row"]].sum() >= 50000
        assert not got[s["single_row"]].any() and cnt[s["single_row"]] == 0 and snap[s["single_row"]] == 0


def test_cospair_is_bitwise_reproducible(pkg, gpu):
    """integer counters: the same call twice gives the same bits, and the "cospair" timer counts both"""
    ctx, _ = gpu
    ctx.timers_enable(True); ctx.timers_reset()
    a = run_scene(pkg, gpu, "thin")
    b = run_scene(pkg, gpu, "thin")
    ctx.sync()
    ms, launches = ctx.timer("cospair")
    ctx.timers_enable(False)
    assert launches == 2 and ms > 0
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_cospair_refusals(pkg, gpu):
    """every refusal of the ABI, by status and message; a cloud without colours is refused"""
    ctx, dev = gpu
    s = cs.scene("queue")
    Err = pkg.capi.IsmHipError
    b = Batch(pkg, ctx, dev, s["objs"], s["kps"], s["cell"], s["rgba"])
    plain = Batch(pkg, ctx, dev, s["objs"], s["kps"], s["cell"])
    try:
        for radius in (0.0, -0.25, float("nan")):
            with pytest.raises(Err, match=r"\(-1\).*cospair: bad argument"):                # ISMHIP_ERR_INVALID
                pkg.capi.cospair(ctx, b.cloud, b.kp_off, *b.tk, radius)
        import torch
        out = torch.empty((int(b.kp_off[-1]), cr.DIM), dtype=torch.float32, device=dev)
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        ko = np.ascontiguousarray(b.kp_off, np.uint32)
        for missing in range(5):                                                            # offsets, kpx, kpy, kpz, desc_out
            arg = [C.c_void_p(ko.ctypes.data), p(b.tk[0]), p(b.tk[1]), p(b.tk[2]), p(out)]
            arg[missing] = C.c_void_p(0)
            rc = pkg.capi.lib().ismhip_cospair(ctx._h, b.cloud._h, *arg[:4], C.c_float(s["radius"]), arg[4], None, None, None)
            with pytest.raises(Err, match=r"\(-1\).*cospair: bad argument"):
                ctx.check(rc, "ismhip_cospair")
        with pytest.raises(Err, match=r"\(-1\).*cospair: colour arrays missing"):
            pkg.capi.cospair(ctx, plain.cloud, plain.kp_off, *plain.tk, s["radius"])
        got = pkg.capi.cospair(ctx, b.cloud, b.kp_off, *b.tk, s["radius"])                   # and the call itself still works
        assert got.shape == (len(cs.QUEUE_PAIRS), cr.DIM) and bool(np.isfinite(got.cpu().numpy()).all())
    finally:
        b.close(); plain.close()


# ------------------------------------------------------------------------------------------------ codeword search on real rows
_rows = {}


def cospair_rows(pkg, gpu):
    """~5000 CoSPAIR rows of the mid object with random colours: 4000 codewords and 1000 queries"""
    if "rows" not in _rows:
        ctx, dev = gpu
        p, n, rng = fs.mid_object()
        sel = rng.choice(len(p), 5200, replace=False)
        rgba = np.random.default_rng(76).integers(0, 1 << 24, size=len(p)).astype(np.uint32)
        s = Batch(pkg, ctx, dev, [(p, n)], [p[sel]], sss.MID_CELL, [rgba])
        try:
            rows = pkg.capi.cospair(ctx, s.cloud, s.kp_off, *s.tk, sss.MID_RADIUS).cpu().numpy()
        finally:
            s.close()
        rows = rows[np.isfinite(rows).all(1)]
        assert len(rows) >= 5000
        _rows["rows"] = (rows[:4000].copy(), rows[4000:5000].copy())
    return _rows["rows"]


@pytest.mark.parametrize("metric", [0, 1])
def test_knn_on_cospair_rows(pkg, gpu, ora, metric):
    """ismhip_knn on real CoSPAIR rows, D = 378 (no multiple of 4; padded to 384), 4000 words and 1000 queries with five exact hits:
    indices equal and distances bit-equal to the oracle's exact search, squared L2 and chi-square, k = 1 and 3"""
    ctx, dev = gpu
    words, q = cospair_rows(pkg, gpu)
    assert words.shape[1] == cr.DIM
    q = q.copy(); q[:5] = words[:5]                                        # exact hits: distance 0
    host, cb = _cb(pkg, gpu, words)
    for k in (1, 3):
        idx, dist = pkg.capi.knn(ctx, cb, metric, T(q, dev), k)
        widx, wdist = ora.knn(metric, words, q, k)
        assert np.array_equal(idx.cpu().numpy(), widx)
        assert np.array_equal(dist.cpu().numpy(), wdist)
    cb.close()


# ------------------------------------------------------------------------------------------------ end to end
def _model_cfg():
    """the value set of config/kinect_cospair.ism with its lengths (Radius, ReferenceFrameRadius, LeafSize, Bandwidth: those of 0.15-unit
    Kinect views) replaced by the ones that fit the unit-sized synthetic shapes"""
    j = json.load(open(os.path.join(hb.ROOT, "config", "kinect_cospair.ism")))["ObjectConfig"]
    j["Children"]["Features"]["Parameters"].update(Radius=0.4, ReferenceFrameRadius=0.3)
    j["Children"]["Keypoints"]["Parameters"]["LeafSize"] = 0.2
    j["Children"]["Voting"]["Parameters"]["Bandwidth"] = 0.6
    return json.dumps(j)


def test_cospair_end_to_end_through_host_and_driver(pkg, gpu, tmp_path):
    """A CoSPAIR model (378 floats, chi-square) trained on three coloured synthetic classes by the C++ host ("Type": "CoSPAIR"): the
    codebook has dim 378 and as many words and the same vote classes as the Python driver's, the model survives write / read bit for
    bit, and both hosts label the training shapes correctly, with equal top classes."""
    ctx, dev = gpu
    train, _, order = _split(pkg, with_color=True)
    m = hb.Model()
    m.config_from_json(_model_cfg())
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i, rgba=o["rgba"])
    m.train()
    cfg = pkg.pipeline.IsmConfig(n_classes=3, feature="CoSPAIR", distance="ChiSquared", radius=0.4, lrf_radius=0.3, bandwidth=0.6)
    assert cfg.dim == cr.DIM
    rec = pkg.pipeline.Recognizer(ctx, cfg)
    cb = rec.train([pkg.pipeline.DeviceBatch(train.batch(order), dev)], instance_ids=order)
    words, vxyz, vcls, sigma = m.codebook(cr.DIM, 3)
    assert words.shape == cb["words"].shape and words.shape[1] == cr.DIM and len(words) > 100
    assert np.array_equal(vcls, cb["vote_class"])
    path = str(tmp_path / "cospair.ism")
    m.write(path)
    saved = json.load(open(path))
    assert saved["ObjectConfig"]["Children"]["Features"]["Type"] == "CoSPAIR" and os.path.exists(str(tmp_path / "cospair.ismd"))
    m2 = hb.Model()
    m2.read(path)
    assert m2.codebook_size() == m.codebook_size()
    assert np.array_equal(m2.codebook(cr.DIM, 3)[0].view(np.uint32), words.view(np.uint32))
    nb = train.batch(order)
    got = m2.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8, rgba=nb["rgba"])
    want = rec.detect(pkg.pipeline.DeviceBatch(nb, dev))
    assert (got["cls"][:, 0] == nb["labels"]).all()
    assert np.array_equal(want["cls"][:, 0].cpu().numpy(), got["cls"][:, 0])
    m.close(); m2.close()
