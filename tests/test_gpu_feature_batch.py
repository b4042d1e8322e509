"""Every Features type on the wide ragged batch of batch_scenes.py (-m gpu), up to the NaN filter and the codeword search.

Eleven objects put the per-object kernels on the XCD-local block map (csrc/common.h: xcd_object_block) with five padding slots and a
unique longest keypoint run; test_batch_cpu.py proves that from the inputs alone. Per type:
  a  the device's rows, counts and special rows against the type's own restatement, by the comparison and the tolerance of its own
     test_gpu_*.py (the helpers are imported from there; nothing is introduced here)
  b  the rows of every object are the bytes of a call on that object alone (n_obj = 1: plain block order), same cell size
  c  ... and the bytes of a context created with ISMHIP_XCD_MAP=0 (one such context per run of this file)
  d  ismhip_compact_descriptor_rows (one float per row) and ismhip_compact_features (every element) agree on the device's own rows and
     frames, keep exactly the rows the restatement keeps, and every device row is finite throughout or NaN throughout
  e  pipeline.Recognizer.compute_features gives the offsets, source indices and bytes of d
  f  ismhip_knn on what came through equals the oracle bit for bit
Every byte comparison of b and c is strict: the frames, the histograms and the moments of these kernels are sums of integers (fixed
point) or are taken in one order per keypoint, so nothing depends on where a block runs."""
import numpy as np
import pytest

import batch_scenes as bs
import bshot_ref
import cgf_ref
import rift_ref
from test_fpfh_cpu import TOL as FPFH_TOL
from test_gpu_bshot import check_bshot_rows
from test_gpu_cgf import check_keypoint_normals, check_raw_rows
from test_gpu_cospair import check_rows as check_cospair_rows
from test_gpu_esf_local import check_scene as check_esf_scene
from test_gpu_fpfh import check_rows as check_fpfh_rows
from test_gpu_parity import _cb
from test_gpu_rift import _check_gradients, _check_rows as check_rift_rows
from test_gpu_rsd import check_histogram
from test_gpu_short_shot import check_rows as check_short_rows
from test_gpu_shot_ref import check as check_shot_bound
from test_gpu_shotna import assert_matches_restatement
from test_gpu_spin_image import check_rows as check_spin_rows

pytestmark = pytest.mark.gpu
F = np.float32
COLOUR_TYPES = ("CSHOT", "SHORT_CSHOT", "CoSPAIR", "RIFT")              # pipeline.py: the cloud carries colours for these only
_runs, _plain, _answers = {}, {}, {}


def T(a, dev, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, copy=True, order="C"), dtype=dtype).to(dev)


def N(t):
    return t.cpu().numpy()


def _col(a, i, dev):
    """column i of a [n, 3] array on the device; an empty array still hands over a valid pointer"""
    return T(a[:, i] if len(a) else np.zeros(1, F), dev)


def run_type(pkg, ctx, dev, name, b, mlp, esf_samples=bs.ESF_SAMPLES):
    """The calls of pipeline.Recognizer.compute_features for type `name` on the batch dict b, in its order and with its cell size: the cloud
    (with colours only where the harness hands them over), the SHOT frames at LRF_RADIUS, the descriptor. esf_samples None: the library's
    constant, as the harness. -> dict of numpy arrays (rows, cnt, lrf and what the type's comparison needs) plus `dev`: the device tensors
    (desc, lrf, kx, ky, kz) for the hand-over"""
    import torch
    capi = pkg.capi
    kw = bs.capi_kwargs(name)
    t = [_col(b["xyz"], i, dev) for i in range(3)] + [_col(b["normals"], i, dev) for i in range(3)]
    tk = [_col(b["kp"], i, dev) for i in range(3)]
    rgba = T(b["rgba"] if len(b["rgba"]) else np.zeros(1, np.int32), dev, torch.int32)
    kp_rgba = T(b["kp_rgba"] if len(b["kp_rgba"]) else np.zeros(1, np.int32), dev, torch.int32)
    ko = b["kp_off"]
    cloud = capi.Cloud(ctx, b["pt_off"], *t, bs.pipeline_cell(name), rgba=rgba if name in COLOUR_TYPES else None)
    try:
        lrf = capi.shot_lrf(ctx, cloud, ko, *tk, bs.LRF_RADIUS)
        out = {}
        if name == "SHOT":
            desc, cnt = capi.shot352(ctx, cloud, ko, *tk, lrf, kw["radius"], want_counts=True)
        elif name == "BSHOT":
            desc, cnt = capi.bshot352(ctx, cloud, ko, *tk, lrf, kw["radius"], want_counts=True)
            out["shot"] = N(capi.shot352(ctx, cloud, ko, *tk, lrf, kw["radius"]))
        elif name == "CSHOT":
            desc, cnt = capi.cshot1344(ctx, cloud, ko, *tk, kp_rgba, lrf, kw["radius"], want_counts=True)
        elif name == "SHORT_SHOT":
            desc, cnt = capi.short_shot(ctx, cloud, ko, *tk, lrf, want_counts=True, **kw)
        elif name == "SHORT_CSHOT":
            desc, cnt = capi.short_cshot(ctx, cloud, ko, *tk, kp_rgba, lrf, want_counts=True, **kw)
        elif name == "FPFH":
            desc, cnt = capi.fpfh33(ctx, cloud, ko, *tk, kw["radius"], want_counts=True)
        elif name == "CoSPAIR":
            desc, cnt, lev, snap = capi.cospair(ctx, cloud, ko, *tk, kw["radius"], want_counts=True, want_levels=True, want_snap=True)
            out.update(lev=N(lev).astype(np.int64), snap=N(snap).astype(np.int64))
        elif name == "SpinImage":
            ax, ay, az, idx = capi.keypoint_normals(ctx, cloud, ko, *tk, want_index=True)
            desc, cnt = capi.spin_image(ctx, cloud, ko, *tk, ax, ay, az, kw["radius"], kw["image_width"], want_counts=True)
            out.update(axes=np.stack([N(ax), N(ay), N(az)], 1), idx=N(idx))
        elif name == "RSD":
            desc, cnt = capi.rsd(ctx, cloud, ko, *tk, kw["radius"], full_histogram=True, want_counts=True)
        elif name == "RIFT":
            grad, gcnt = capi.intensity_gradients(ctx, cloud, kw["radius"], want_counts=True)
            desc, cnt = capi.rift(ctx, cloud, ko, *tk, kw["radius"], grad, want_counts=True)
            out.update(grad=N(grad), gcnt=N(gcnt))
        elif name == "CGF":
            desc, cnt = capi.cgf(ctx, cloud, ko, *tk, kw["radius"], mlp, want_counts=True)
            R, rmin, rl = capi.cgf_radii(kw["radius"])                    # the same calls taken apart, for the raw rows
            clrf = capi.shot_lrf(ctx, cloud, ko, *tk, rl)
            kn = capi.keypoint_normals_pca(ctx, cloud, ko, *tk, 0.1 * R)
            raw, rcnt = capi.cgf_raw(ctx, cloud, ko, *tk, clrf, *kn, R, rmin, want_counts=True)
            out.update(cgf_lrf=N(clrf).reshape(-1, 9), normals=np.stack([N(x) for x in kn], 1), raw=N(raw), raw_cnt=N(rcnt))
        elif name == "ESF_LOCAL":
            more = {} if esf_samples is None else dict(n_samples=esf_samples)
            desc, cnt, bins, scale = capi.esf_local(ctx, cloud, ko, *tk, kw["radius"], want_counts=True, want_bins=True, want_scale=True, **more)
            out.update(bins=N(bins).astype(np.int64), scale=N(scale))
        else:
            raise KeyError(name)
        ctx.sync()
        out.update(rows=N(desc), cnt=N(cnt).astype(np.int64), lrf=N(lrf).reshape(-1, 9), dev=(desc, lrf, *tk))
        return out
    finally:
        cloud.close()


def byte_keys(got):
    """every numpy output of a run, for the byte comparisons"""
    return sorted(k for k, v in got.items() if isinstance(v, np.ndarray))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def default_run(pkg, gpu, name):
    """the whole batch on the shared context (default block map), once per type"""
    if name not in _runs:
        ctx, dev = gpu
        mlp = pkg.capi.Mlp(ctx, bs.cgf_layers()) if name == "CGF" else None
        try:
            _runs[name] = run_type(pkg, ctx, dev, name, bs.batch(), mlp)
        finally:
            if mlp is not None:
                mlp.close()
    return _runs[name]


def plain_runs(pkg, dev, monkeypatch):
    """every type on ONE context created with ISMHIP_XCD_MAP=0 (the switch is read when a context is created), closed again"""
    if not _plain:
        monkeypatch.setenv("ISMHIP_XCD_MAP", "0")
        ctx = pkg.capi.Ctx(0)
        monkeypatch.delenv("ISMHIP_XCD_MAP")
        mlp = None
        try:
            mlp = pkg.capi.Mlp(ctx, bs.cgf_layers())
            runs = {name: run_type(pkg, ctx, dev, name, bs.batch(), mlp) for name in bs.TYPES}
        finally:
            if mlp is not None:
                mlp.close()
            ctx.close()
        _plain.update(runs)                                               # published whole: a failure above shows again in every case
    return _plain


def answer(name, ora, **kw):
    key = (name, tuple(sorted(kw)))
    if key not in _answers:
        _answers[key] = bs.answer(name, rgb2lab=ora.rgb2lab, **kw)
    return _answers[key]


# ------------------------------------------------------------------------------------------------------------------ a
def test_frames_match_the_restatement(pkg, gpu):
    """the SHOT frames every type's keypoints are filtered by: NaN rows exact, 1e-5 per component on the decided ones (all of them)"""
    got = default_run(pkg, gpu, "SHOT")["lrf"]
    r = bs.frames()
    both = assert_matches_restatement(got, r)
    assert both.sum() == (~np.isnan(r["frame"][:, 0])).sum() == 36


@pytest.mark.parametrize("name", bs.TYPES)
def test_batch_rows_match_the_restatement(pkg, gpu, ora, name):
    got = default_run(pkg, gpu, name)
    b = bs.batch()
    rows, cnt = got["rows"], got["cnt"]
    K = len(b["kp"])
    if name in ("SHOT", "CSHOT"):
        a = answer(name, ora, lrf=got["lrf"])                           # on the device's own frames, as test_gpu_shot_ref.py
        assert np.array_equal(cnt, a["cnt"]) and np.array_equal(np.isnan(rows), np.isnan(a["rows"]))
        fin = ~np.isnan(a["rows"][:, 0])
        assert fin.sum() == 36 and not a["undecided"].any()
        check_shot_bound("batch " + name, rows[fin], a["rows"][fin], a["bound"][fin])
    elif name == "BSHOT":
        a = answer("SHOT", ora, lrf=got["lrf"])
        assert np.array_equal(cnt, a["cnt"])
        left_out, groups, zero = check_bshot_rows(rows, got["shot"], a["rows"])
        print("batch BSHOT: groups %d, zero-sum %d, non-zero left out share %.3f" % (groups, zero, left_out))
        assert left_out <= 0.30
    elif name in ("SHORT_SHOT", "SHORT_CSHOT"):
        a = answer(name, ora, lrf=got["lrf"])
        check_short_rows(rows, cnt, a["rows"], a["cnt"], a["rows"].shape[1])
    elif name == "FPFH":
        r = answer(name, ora)["ref"]
        ex = check_fpfh_rows(r, rows, cnt)
        print("batch FPFH: largest excess %.3g, exempt keypoints %s" % (ex.max(initial=0.0), np.nonzero(r.exempt)[0].tolist()))
        want, wcnt = ora.fpfh33(b["pt_off"], *b["xyz"].T.copy(), *b["normals"].T.copy(), b["kp_off"], *b["kp"].T.copy(), bs.RADIUS)
        assert r.exempt.sum() == 1 and np.abs(rows[r.exempt] - want[r.exempt]).max() <= FPFH_TOL     # the planted one: the oracle's row decides
    elif name == "CoSPAIR":
        und = check_cospair_rows(answer(name, ora)["ref"], rows, cnt, got["lev"], got["snap"])
        print("batch CoSPAIR: %d rows with an undecided deposit" % und)
    elif name == "SpinImage":
        dev_ = check_spin_rows(got["axes"], got["idx"], rows, cnt, answer(name, ora))
        print("batch SpinImage: largest deviation %.3e" % dev_)
    elif name == "RSD":
        check_histogram(rows, cnt, answer(name, ora)["ref"])
    elif name == "RIFT":
        n_und = 0
        for o, (ps, ks) in enumerate(bs.objects()):
            ga = bs.rift_gradients(o)
            n_und += _check_gradients(got["grad"][ps], got["gcnt"][ps], ga, bs.RADIUS, "batch RIFT object %d" % o)[0]
            want = rift_ref.rift(b["xyz"][ps], got["grad"][ps], b["kp"][ks], bs.RADIUS, undecided_points=ga["undecided"])   # on the device's gradients
            n_und += check_rift_rows(rows[ks], cnt[ks], want, "batch RIFT object %d" % o)[0]
            # and end to end, the restatement's rows from ITS gradients, as test_gpu_rift.py
            gerr = rift_ref.grad_tol(ga["x"], bs.RADIUS, ps.stop - ps.start) + 2.0 ** -24 * np.abs(ga["grad"]).max(1) if ps.stop > ps.start else None
            want = rift_ref.rift(b["xyz"][ps], ga["grad"].astype(F), b["kp"][ks], bs.RADIUS, undecided_points=ga["undecided"], gerr=gerr)
            n_und += check_rift_rows(rows[ks], cnt[ks], want, "batch RIFT object %d end to end" % o)[0]
        assert n_und == 0
        zero = slice(*bs.kp_range("four_points"))
        assert not rows[zero].any()
    elif name == "CGF":
        a = answer(name, ora, device=dict(lrf=got["cgf_lrf"], normals=got["normals"]))
        finite_kp = np.isfinite(b["kp"]).all(1)
        want = dict(undecided=a["undecided"] | ~finite_kp, sum=a["cnt"], rows=a["raw"], ball=a["ball"])
        dec = check_raw_rows(dict(rows=got["raw"], count=got["raw_cnt"]), want)
        assert dec.sum() == finite_kp.sum() and not got["raw"][(a["cnt"] == 0) & finite_kp].any()
        assert np.isnan(got["raw"][~finite_kp]).all() and np.isfinite(got["raw"][finite_kp]).all()
        y, e = cgf_ref.mlp(got["raw"], bs.cgf_layers())                  # the embedding of the device's own raw rows, as test_gpu_mlp.py
        assert np.array_equal(np.isnan(rows), np.isnan(y)) and (np.abs(rows - y)[finite_kp] <= e[finite_kp]).all()
        assert np.array_equal(cnt, got["raw_cnt"])
    elif name == "ESF_LOCAL":
        s = dict(pt_off=b["pt_off"], xyz=b["xyz"], kp_off=b["kp_off"], kp=b["kp"], radius=bs.ESF_RADIUS, n_samples=bs.ESF_SAMPLES)
        a = check_esf_scene(s, (rows, cnt, got["bins"], got["scale"]))
        assert not a["whole"].any()
    # the special rows are the restatement's, whatever the comparison above covers
    a = answer(name, ora) if name not in ("SHOT", "CSHOT", "SHORT_SHOT", "SHORT_CSHOT") else answer(name, ora, lrf=got["lrf"])
    if name == "BSHOT":
        a = dict(rows=bshot_ref.binarize(answer("SHOT", ora, lrf=got["lrf"])["rows"]))
    want_nan, want_zero, _ = bs.special_rows(name, a)
    assert rows.shape == (K, np.asarray(a["rows"]).shape[1])
    assert np.array_equal(np.isnan(rows).all(1), want_nan) and np.array_equal(np.isnan(rows).any(1), want_nan)
    assert np.array_equal(~rows.any(1), want_zero)


# ------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("name", bs.TYPES)
def test_batch_placement_changes_nothing(pkg, gpu, name):
    """common.h: "the result does not depend on the placement". Every object with a keypoint, alone (n_obj = 1 runs the plain object-major
    block order, nbx from its own run), against its rows of the 11-object call: every output, byte for byte."""
    ctx, dev = gpu
    whole = default_run(pkg, gpu, name)
    b = bs.batch()
    mlp = pkg.capi.Mlp(ctx, bs.cgf_layers()) if name == "CGF" else None
    try:
        for o, (ps, ks) in enumerate(bs.objects()):
            if ks.stop == ks.start:
                continue
            one = run_type(pkg, ctx, dev, name, bs.single(o), mlp)
            for key in byte_keys(one):
                sl = ps if key in ("grad", "gcnt") else ks
                assert same_bytes(one[key], whole[key][sl]), (name, bs.NAMES[o], key)
    finally:
        if mlp is not None:
            mlp.close()


# ------------------------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("name", bs.TYPES)
def test_plain_block_order_gives_the_same_bytes(pkg, gpu, monkeypatch, name):
    whole = default_run(pkg, gpu, name)
    plain = plain_runs(pkg, gpu[1], monkeypatch)[name]
    assert byte_keys(plain) == byte_keys(whole)
    for key in byte_keys(whole):
        assert same_bytes(plain[key], whole[key]), (name, key)


# ------------------------------------------------------------------------------------------------------------------ d, e, f
def kept_by_the_restatement(name, ora):
    rows = np.asarray(answer(name, ora)["rows"])
    lrf = bs.frames()["frame"]
    return ~np.isnan(rows).any(1) & np.isfinite(lrf[:, [0, 3, 6]]).all(1)


@pytest.mark.parametrize("name", bs.TYPES)
def test_hand_over_to_the_search(pkg, gpu, ora, tmp_path, name):
    """d, e, f on one run of the harness's own calls (ESF_LOCAL at the library's sample count, as the harness)"""
    ctx, dev = gpu
    capi, pipeline = pkg.capi, pkg.pipeline
    b = bs.batch()
    path = str(tmp_path / "net.cgfw")
    mlp = None
    if name == "CGF":
        capi.cgfw_write(path, bs.cgf_layers())
        mlp = capi.Mlp.from_file(ctx, path, cgf_ref.DIM)
    try:
        got = run_type(pkg, ctx, dev, name, b, mlp, esf_samples=None)
    finally:
        if mlp is not None:
            mlp.close()
    rows, lrf = got["rows"], got["lrf"]
    desc_t, lrf_t, kx, ky, kz = got["dev"]
    # d: the device's rows are whole, and the two filters agree with each other and with the restatement
    assert np.array_equal(np.isnan(rows).any(1), np.isnan(rows[:, 0])) and np.array_equal(np.isnan(rows).all(1), np.isnan(rows[:, 0]))
    assert not np.isinf(rows).any()
    if name == "BSHOT":
        assert not np.isnan(rows).any()
        shot_nan = np.isnan(got["shot"][:, 0])
        assert shot_nan.sum() == 8 and (rows[shot_nan] == 1).all()      # a NaN SHOT row becomes 352 ones and stays
    fast = capi.compact_descriptor_rows(ctx, b["kp_off"], desc_t, lrf_t, kx, ky, kz)
    full = capi.compact_features(ctx, b["kp_off"], desc_t, lrf_t, kx, ky, kz)
    ctx.sync()
    assert np.array_equal(fast[0], full[0])
    for f, g in zip(fast[1:], full[1:]):
        assert same_bytes(N(f), N(g))
    src = N(fast[6]).astype(np.int64)
    keep = kept_by_the_restatement(name, ora)
    assert np.array_equal(src, np.nonzero(keep)[0])
    want_off = np.concatenate([[0], np.cumsum([keep[ks].sum() for _ps, ks in bs.objects()])]).astype(np.uint32)
    assert np.array_equal(fast[0], want_off)
    assert same_bytes(N(fast[1]), rows[src]) and same_bytes(N(fast[2]).reshape(-1, 9), lrf[src])
    assert same_bytes(np.stack([N(fast[3]), N(fast[4]), N(fast[5])], 1), b["kp"][src])
    assert 20 <= len(src) < len(rows) and (np.diff(want_off.astype(np.int64)) == 0).sum() >= 4       # dropped rows, and empty ranges between kept ones
    # e: the harness's own wiring
    cfg = pipeline.IsmConfig(**bs.config_kwargs(name), **(dict(cgf_model=path) if name == "CGF" else {}))
    rec = pipeline.Recognizer(ctx, cfg)                                   # (it owns the CGF embedding it loads, as in test_gpu_cgf_host.py)
    f = rec.compute_features(pipeline.DeviceBatch(b, dev), want_counts=True)
    try:
        ctx.sync()
        assert np.array_equal(f["off"], fast[0]) and np.array_equal(N(f["src"]), N(fast[6]))
        assert same_bytes(N(f["desc"]), N(fast[1])) and same_bytes(N(f["lrf"]), N(fast[2]))
        assert np.array_equal(N(f["counts"]).astype(np.int64), got["cnt"])
    finally:
        f["cloud"].close()
    # f: search on what came through
    q = rows[src]
    words = np.ascontiguousarray(q[:len(q) // 2])
    _host, cb = _cb(pkg, gpu, words)
    try:
        idx, dist = capi.knn(ctx, cb, capi.METRIC_L2SQ, fast[1].contiguous(), 1)
        widx, wdist = ora.knn(capi.METRIC_L2SQ, words, q, 1)
        assert np.array_equal(N(idx), widx) and np.array_equal(N(dist).view(np.uint32), wdist.view(np.uint32))
        assert np.isfinite(N(dist)).all() and len(words) >= 10
        if name == "BSHOT":
            cb.make_binary()
            bidx, bdist = capi.knn_binary(ctx, cb, fast[1].contiguous(), 1)
            hidx, hdist = bshot_ref.hamming_knn(words, q, 1)
            assert np.array_equal(N(bidx), hidx) and np.array_equal(N(bdist).view(np.uint32), hdist.view(np.uint32))
    finally:
        cb.close()
