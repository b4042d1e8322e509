"""The cloud passes and the three keypoint detectors on the wide ragged batch of batch_scenes.py (-m gpu): ismhip_keypoint_normals,
ismhip_keypoint_normals_pca, ismhip_intensity_gradients; ISS3D (saliency, keypoints); VoxelGridCulling (principal curvatures, scores,
selection, the convenience call); SIFT3D (normal curvature, scale space, extrema, the octave driver).

Eleven objects, five padding slots of the XCD-local block map, and per-object maxima (k_cull_nmax, k_cull_kmax, k_sift_imax, k_rift_gmax)
that differ by powers of two between neighbouring objects (test_batch_cpu.py proves both from the inputs): a reduction that answers for
the wrong object puts that object's fixed point on another grid. Per pass:
  - values against the module's restatement, object by object, by the comparison and the bounds of the module's own test_gpu_*.py;
  - output offsets equal to the restatement's counts per object (the SIFT3D detector: to its stage entries composed by hand, since
    sift3d_ref.py restates one octave without the downsampling in front of it; see test_sift3d_matches_the_restatement);
  - every output of every object the bytes of a call on that object alone (n_obj = 1), strictly: these sums are order free (fixed point);
  - every output the bytes of a context created with ISMHIP_XCD_MAP=0 (one per run of this file);
  - detectors: a capacity of exactly the total is accepted, one less is refused by name (a test of its own, on the whole batch), and the
    empty and the all-NaN object yield empty ranges between non-empty ones."""
import numpy as np
import pytest

import batch_scenes as bs
import cgf_ref
import culling_ref
import spin_image_ref
import test_gpu_culling as gc
from test_gpu_cgf import check_keypoint_normals
from test_gpu_iss3d import _check_object as check_iss3d_object
from test_gpu_rift import _check_gradients
from test_gpu_sift3d import _by_hand as sift3d_by_hand

pytestmark = pytest.mark.gpu
SELECT_KW = dict(combine="RequireCombinedList")
_whole, _plain = {}, {}


def T(a, dev, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, copy=True, order="C"), dtype=dtype).to(dev)


def N(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _pad(a):
    """an empty array still hands over a valid pointer"""
    return a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)


def run_passes(pkg, ctx, dev, b):
    """every pass of this file on the batch dict b -> dict(pt: per point, kp: per keypoint of the batch, obj: per object, rag: name ->
    (offsets, dict of arrays packed object after object)), all numpy. Cell sizes as the modules' own tests choose them."""
    import torch
    capi = pkg.capi
    po, ko = b["pt_off"], b["kp_off"]
    xyz, nrm = _pad(b["xyz"]), _pad(b["normals"])
    t = [T(xyz[:, i], dev) for i in range(3)] + [T(nrm[:, i], dev) for i in range(3)]
    kp = _pad(b["kp"])
    tk = [T(kp[:, i], dev) for i in range(3)]
    rgba = T(_pad(b["rgba"]), dev, torch.int32)
    inten = T(_pad(b["intensity"]), dev)
    pt, kpo, obj, rag = {}, {}, {}, {}
    # ---- the lookups and the gradients (SpinImage, CGF, RIFT)
    R = capi.cgf_radii(bs.CGF_RADIUS)[0]
    cloud = capi.Cloud(ctx, po, *t, 0.4 * bs.RADIUS, rgba=rgba)
    try:
        if int(ko[-1]) > 0:                                               # (no keypoint at all: no output array to hand over)
            ax, ay, az, idx = capi.keypoint_normals(ctx, cloud, ko, *tk, want_index=True)
            pn = capi.keypoint_normals_pca(ctx, cloud, ko, *tk, 0.1 * R)
            kpo.update(axes=np.stack([N(ax), N(ay), N(az)], 1), idx=N(idx), pca=np.stack([N(x) for x in pn], 1))
        grad, gcnt = capi.intensity_gradients(ctx, cloud, bs.RADIUS, want_counts=True)
        ctx.sync()
        pt.update(grad=N(grad), gcnt=N(gcnt))
    finally:
        cloud.close()
    # ---- ISS3D
    cloud = capi.Cloud(ctx, po, *t, 0.4 * bs.ISS_NONMAX, rgba=rgba)
    try:
        sal, eig, cnt = capi.iss3d_saliency(ctx, cloud, bs.ISS_SALIENT, bs.ISS_GAMMA, bs.ISS_GAMMA, bs.ISS_MIN_NEIGHBORS)
        io, kx, ky, kz, kc, src = capi.iss3d_keypoints(ctx, cloud, bs.ISS_SALIENT, bs.ISS_NONMAX, bs.ISS_GAMMA, bs.ISS_GAMMA, bs.ISS_MIN_NEIGHBORS)
        ctx.sync()
        pt.update(sal=N(sal), eig=N(eig), iss_cnt=N(cnt))
        rag["iss"] = (io, dict(kxyz=np.stack([N(kx), N(ky), N(kz)], 1).reshape(-1, 3), krgba=N(kc), src=N(src)))
    finally:
        cloud.close()
    # ---- VoxelGridCulling (the Device of test_gpu_culling.py: the cloud, its voxel keypoints, the scores)
    # (an object without a single point, alone, has nothing to build a Device from: its outputs are the empty ranges)
    d = gc.Device(pkg, (ctx, dev), (po, b["xyz"], b["normals"], b["rgba"].astype(np.int32).view(np.uint32)), leaf=bs.CULL_LEAF) if len(b["xyz"]) else None
    if d is not None:
        try:
            pc1, pc2, pcn = d.curvatures()
            g_curv, col, cnt = d.scores("curvature")
            g_kpq, col2, cnt2 = d.scores("kpq")
            sel = d.select(**SELECT_KW)
            vo, vx, vy, vz, vc = capi.voxel_culling_keypoints(ctx, d.cloud, bs.CULL_LEAF, geometry="kpq", color="colordistance", max_similar_color_distance=gc.MAX_DIST)
            ctx.sync()
            assert same_bytes(col, col2) and same_bytes(cnt, cnt2)
            pt.update(pc1=pc1, pc2=pc2, pcn=pcn)
            rag["vox"] = (d.ko, dict(kp=d.kp, kp_rgba=d.kp_rgba, g_curv=g_curv, col=col, cnt=cnt, g_kpq=g_kpq, keep=sel["keep"], combined=sel["combined"]))
            rag["sel"] = (sel["kp_offsets"], dict(kxyz=np.stack([sel["kx"], sel["ky"], sel["kz"]], 1).reshape(-1, 3), krgba=sel["krgba"]))
            rag["vck"] = (vo, dict(kxyz=np.stack([N(vx), N(vy), N(vz)], 1).reshape(-1, 3), krgba=N(vc)))
            obj["thresholds"] = sel["thresholds"]
        finally:
            d.close()
    # ---- SIFT3D
    sc = capi.sift3d_scales(bs.SIFT_MIN_SCALE, bs.SIFT_SCALES)
    assert same_bytes(sc, bs.sift_scales())
    cloud = capi.Cloud(ctx, po, *t, 0.4 * 3.0 * float(sc[-1]))
    try:
        curv, ccnt = capi.normal_curvature(ctx, cloud, bs.CURV_RADIUS)
        dog, dcnt = capi.sift3d_scale_space(ctx, cloud, inten, sc)
        flags, nn = capi.sift3d_extrema(ctx, cloud, dog)
        so, sx, sy, sz, ss, sizes = capi.sift3d_keypoints(ctx, cloud, inten, bs.SIFT_MIN_SCALE, bs.SIFT_OCTAVES, bs.SIFT_SCALES)
        ctx.sync()
        n = int(po[-1])
        pt.update(curv=N(curv), curv_cnt=N(ccnt), dog=N(dog)[:n], dog_cnt=N(dcnt), flags=N(flags)[:n], nn=N(nn)[:n])
        rag["sift"] = (so, dict(kxyz=np.stack([N(sx), N(sy), N(sz)], 1).reshape(-1, 3), scale=N(ss)))
        obj["sizes"] = sizes
    finally:
        cloud.close()
    return dict(pt=pt, kp=kpo, obj=obj, rag=rag)


def whole_run(pkg, gpu):
    """the batch on the shared context (default block map), once"""
    if not _whole:
        _whole.update(run_passes(pkg, *gpu, bs.batch()))
    return _whole


def plain_run(pkg, dev, monkeypatch):
    """the batch on a context created with ISMHIP_XCD_MAP=0 (read when a context is created), once, closed again"""
    if not _plain:
        monkeypatch.setenv("ISMHIP_XCD_MAP", "0")
        ctx = pkg.capi.Ctx(0)
        monkeypatch.delenv("ISMHIP_XCD_MAP")
        try:
            _plain.update(run_passes(pkg, ctx, dev, bs.batch()))
        finally:
            ctx.close()
    return _plain


def points_of(o):
    return bs.objects()[o][0]


# ------------------------------------------------------------------------------------------------------------------ against the restatements
def test_keypoint_normals_and_gradients_match_the_restatements(pkg, gpu):
    w = whole_run(pkg, gpu)
    b = bs.batch()
    axes, idx = spin_image_ref.batch_normals(b["pt_off"], b["xyz"], b["normals"], b["kp_off"], b["kp"])
    assert np.array_equal(w["kp"]["idx"], idx) and same_bytes(w["kp"]["axes"], axes)           # a lookup: exact
    assert (idx >= 0).sum() >= 25 and (idx < 0).sum() >= 10
    R = cgf_ref.radii(bs.CGF_RADIUS)[0]
    compared = 0
    for o, (ps, ks) in enumerate(bs.objects()):
        want, cnt, gap = cgf_ref.pca_normal(b["xyz"][ps], b["kp"][ks], 0.1 * R)
        ok, err, tol = check_keypoint_normals(w["kp"]["pca"][ks], want, cnt, gap)
        compared += int(ok.sum())
        n_und, _rel, _err = _check_gradients(w["pt"]["grad"][ps], w["pt"]["gcnt"][ps], bs.rift_gradients(o), bs.RADIUS, "batch object %d" % o)
        assert n_und == 0
    assert compared >= 25
    g = w["pt"]["grad"]
    ps = points_of(bs.obj("four_points"))
    assert not g[ps].any() and np.isfinite(g[points_of(bs.obj("longest"))]).all()


def test_iss3d_matches_the_restatement(pkg, gpu):
    w = whole_run(pkg, gpu)
    b = bs.batch()
    off, out = w["rag"]["iss"]
    got = dict(saliency=w["pt"]["sal"], eig=w["pt"]["eig"], count=w["pt"]["iss_cnt"], off=off, **out)
    want_off = [0]
    for o, (ps, _ks) in enumerate(bs.objects()):
        want = bs.iss3d_answer(o)
        assert check_iss3d_object(got, o, ps.start, ps.stop, b["xyz"][ps], want, b["rgba"], "batch") == 0
        want_off.append(want_off[-1] + int(want["keep"].sum()))
    assert np.array_equal(off, np.asarray(want_off, np.uint32))
    n = np.diff(off.astype(np.int64))
    print("ISS3D keypoints per object", n.tolist())
    assert n[bs.obj("empty")] == 0 and n[bs.obj("all_nan")] == 0 and n[bs.obj("longest")] > 0 and n[bs.obj("small3")] > 0 and n[bs.obj("holes")] > 0


def test_culling_matches_the_restatement(pkg, gpu, ora):
    w = whole_run(pkg, gpu)
    ctx, dev = gpu
    b = bs.batch()
    arrays = (b["pt_off"], b["xyz"], b["normals"], b["rgba"].view(np.uint32))
    ko, v = w["rag"]["vox"]

    class Scored:                                                         # what gc.check_scores reads of a Device
        leaf, kp, kp_rgba = bs.CULL_LEAF, v["kp"], v["kp_rgba"]
    Scored.ko = ko
    n_kp = gc.check_scores("batch", Scored, arrays, ora.rgb2lab, w["pt"]["pc1"], w["pt"]["pc2"], w["pt"]["pcn"], v["g_curv"], v["col"], v["cnt"], v["g_kpq"],
                           pcs=[bs.pc_answer(o) for o in range(bs.N_OBJ)])
    assert n_kp == int(ko[-1]) >= 200
    # the selection: the restatement's on the device's own scores, bit for bit, and its counts are the offsets
    so, s = w["rag"]["sel"]
    want_off, keep_all = [0], np.zeros(len(v["keep"]), bool)
    for o in range(bs.N_OBJ):
        kb, ke = int(ko[o]), int(ko[o + 1])
        want = culling_ref.select(v["g_kpq"][kb:ke], v["col"][kb:ke])
        assert np.array_equal(v["keep"][kb:ke].astype(bool), want["keep"]), o
        assert gc.same_bits(w["obj"]["thresholds"][o], want["thresholds"]) or (np.isnan(want["thresholds"]).any() and
                                                                               np.array_equal(w["obj"]["thresholds"][o], want["thresholds"], equal_nan=True)), o
        assert np.array_equal(v["combined"][kb:ke], want["combined"], equal_nan=True), o
        keep_all[kb:ke] = want["keep"]
        want_off.append(want_off[-1] + int(want["keep"].sum()))
    assert np.array_equal(so, np.asarray(want_off, np.uint32))
    assert same_bytes(s["kxyz"], v["kp"][keep_all]) and same_bytes(s["krgba"].view(np.uint32), v["kp_rgba"][keep_all])
    vo, vk = w["rag"]["vck"]                                              # the convenience call is the three entries in a row
    assert np.array_equal(vo, so) and same_bytes(vk["kxyz"], s["kxyz"]) and same_bytes(vk["krgba"], s["krgba"])
    n = np.diff(so.astype(np.int64))
    print("VoxelGridCulling: voxel keypoints", np.diff(ko.astype(np.int64)).tolist(), "kept", n.tolist())
    assert n[bs.obj("empty")] == 0 and n[bs.obj("all_nan")] == 0 and n[bs.obj("longest")] > 0 and n[bs.obj("small3")] > 0 and n[bs.obj("holes")] > 0
    assert 0 < int(so[-1]) < int(ko[-1])
    # per-object thresholds differ: an object's cutoff is its own
    assert len({float(x) for x in w["obj"]["thresholds"][:, 2] if np.isfinite(x)}) >= 5


def test_sift3d_matches_the_restatement(pkg, gpu):
    """sift3d_ref.py restates one octave on the cloud as given: the scale space, the extremum flags and the neighbour counts of the
    stage entries are held to it per object. The detector itself (ismhip_sift3d_keypoints) downsamples the cloud before every octave and
    runs up to four of them, which the restatement does not cover: its output offsets, keypoints, scales and octave sizes are held to
    the same stage entries composed by hand (test_gpu_sift3d._by_hand, the comparison of the detector's own test), not to counts of the
    restatement."""
    w = whole_run(pkg, gpu)
    ctx, dev = gpu
    b = bs.batch()
    und = size = 0
    for o, (ps, _ks) in enumerate(bs.objects()):
        c = bs.curvature_answer(o)                                        # the normal curvature is the culling score (test_gpu_sift3d.py)
        assert np.array_equal(w["pt"]["curv_cnt"][ps], c["count"]), o
        gc.check_within("batch object %d normal curvature" % o, w["pt"]["curv"][ps], np.where(np.isnan(c["geo"]), np.nan, c["geo64"]), c["bound"])
        want = bs.sift3d_answer(o)
        dog = w["pt"]["dog"][ps].astype(np.float64)
        nan = np.isnan(want["dog"])
        assert np.array_equal(np.isnan(dog), nan) and np.array_equal(w["pt"]["dog_cnt"][ps], want["count"]), o
        if (~nan).any():
            ratio = np.abs(dog - want["dog"])[~nan] / want["bound"][~nan]
            print("batch object %d: worst dog error / bound %.3f" % (o, ratio.max()))
            assert (ratio <= 1.0).all(), o
        u = want["undecided"]
        assert np.array_equal(w["pt"]["nn"][ps], want["nn"]), o
        assert np.array_equal(w["pt"]["flags"][ps][~u], want["flags"][~u]), o
        und += int(u[:, 1:-1].sum()); size += u[:, 1:-1].size
    assert und / size <= 0.02
    f = w["pt"]["flags"]
    assert not f[:, 0].any() and not f[:, -1].any() and (f > 0).sum() >= 50
    # the driver: the four stage entries composed by hand, as test_gpu_sift3d.py composes them
    so, s = w["rag"]["sift"]
    objs = [b["xyz"][ps] for ps, _ in bs.objects()]
    inten = [b["intensity"][ps] for ps, _ in bs.objects()]
    wo, wkp, wks, wsizes = sift3d_by_hand(pkg, ctx, dev, objs, inten, bs.SIFT_MIN_SCALE, bs.SIFT_OCTAVES, bs.SIFT_SCALES)
    n = np.diff(so.astype(np.int64))
    print("SIFT3D keypoints per object", n.tolist(), "octave sizes", w["obj"]["sizes"].tolist())
    assert np.array_equal(so, wo) and np.array_equal(w["obj"]["sizes"], wsizes)
    assert same_bytes(s["kxyz"], wkp) and same_bytes(s["scale"], wks)
    assert n[bs.obj("empty")] == 0 and n[bs.obj("all_nan")] == 0 and n[bs.obj("longest")] > 0 and n[bs.obj("small3")] > 0 and n[bs.obj("holes")] > 0


# ------------------------------------------------------------------------------------------------------------------ capacity
def test_detectors_take_a_capacity_of_exactly_the_total_and_refuse_one_less(pkg, gpu):
    """the three detectors on the whole batch: output arrays of exactly the total give the offsets and the keypoints of the default
    capacity; one entry less is an argument error that names the capacity, as the detectors' own tests ask"""
    import torch
    w = whole_run(pkg, gpu)
    ctx, dev = gpu
    capi = pkg.capi
    b = bs.batch()
    po = b["pt_off"]
    t = [T(b["xyz"][:, i], dev) for i in range(3)] + [T(b["normals"][:, i], dev) for i in range(3)]
    rgba = T(b["rgba"], dev, torch.int32)
    iss = (bs.ISS_SALIENT, bs.ISS_NONMAX, bs.ISS_GAMMA, bs.ISS_GAMMA, bs.ISS_MIN_NEIGHBORS)
    io, out = w["rag"]["iss"]
    total = int(io[-1])
    assert total > 0
    cloud = capi.Cloud(ctx, po, *t, 0.4 * bs.ISS_NONMAX, rgba=rgba)
    try:
        o2, kx, ky, kz, _kc, src = capi.iss3d_keypoints(ctx, cloud, *iss, capacity=total)
        ctx.sync()
        assert np.array_equal(o2, io) and same_bytes(N(src), out["src"]) and same_bytes(np.stack([N(kx), N(ky), N(kz)], 1).reshape(-1, 3), out["kxyz"])
        with pytest.raises(capi.IsmHipError, match=r"\(-1\).*capacity"):
            capi.iss3d_keypoints(ctx, cloud, *iss, capacity=total - 1)
    finally:
        cloud.close()
    so, out = w["rag"]["sel"]
    kept = int(so[-1])
    assert kept > 0
    d = gc.Device(pkg, gpu, (po, b["xyz"], b["normals"], b["rgba"].astype(np.int32).view(np.uint32)), leaf=bs.CULL_LEAF)
    try:
        d.curvatures()
        d.scores("kpq")
        r = capi.culling_select(ctx, d.ko, d.geo, d.col, d.kx, d.ky, d.kz, d.kc, capacity=kept, **SELECT_KW)
        ctx.sync()
        assert np.array_equal(r["kp_offsets"], so)
        assert same_bytes(np.stack([N(r["kx"]), N(r["ky"]), N(r["kz"])], 1).reshape(-1, 3), out["kxyz"]) and same_bytes(N(r["krgba"]), out["krgba"])
        with pytest.raises(capi.IsmHipError, match="capacity too small"):
            capi.culling_select(ctx, d.ko, d.geo, d.col, d.kx, d.ky, d.kz, d.kc, capacity=kept - 1, **SELECT_KW)
    finally:
        d.close()
    fo, out = w["rag"]["sift"]
    total = int(fo[-1])
    assert total > 0
    sift = (bs.SIFT_MIN_SCALE, bs.SIFT_OCTAVES, bs.SIFT_SCALES)
    inten = T(b["intensity"], dev)
    cloud = capi.Cloud(ctx, po, *t, 0.4 * 3.0 * float(bs.sift_scales()[-1]))
    try:
        o2, sx, sy, sz, ss, sizes = capi.sift3d_keypoints(ctx, cloud, inten, *sift, capacity=total)
        ctx.sync()
        assert np.array_equal(o2, fo) and np.array_equal(sizes, w["obj"]["sizes"])
        assert same_bytes(np.stack([N(sx), N(sy), N(sz)], 1).reshape(-1, 3), out["kxyz"]) and same_bytes(N(ss), out["scale"])
        with pytest.raises(capi.IsmHipError, match="capacity"):
            capi.sift3d_keypoints(ctx, cloud, inten, *sift, capacity=total - 1)
    finally:
        cloud.close()


# ------------------------------------------------------------------------------------------------------------------ placement
def _object_slices(w, o):
    """(group, key, the rows of object o) of every output of a run of the whole batch"""
    ps, ks = bs.objects()[o]
    for key, a in w["pt"].items():
        yield "pt", key, a[ps]
    for key, a in w["kp"].items():
        yield "kp", key, a[ks]
    for key, a in w["obj"].items():
        yield "obj", key, a[o:o + 1]
    for name, (off, arrays) in w["rag"].items():
        yield "rag", name + ".count", np.asarray([int(off[o + 1]) - int(off[o])])
        for key, a in arrays.items():
            yield "rag", name + "." + key, a[int(off[o]):int(off[o + 1])]


def test_every_object_alone_gives_the_bytes_of_the_batch(pkg, gpu):
    """an object on its own is a call with n_obj = 1: plain block order, its own longest run, its own maximum in slot 0"""
    w = whole_run(pkg, gpu)
    ctx, dev = gpu
    for o in range(bs.N_OBJ):
        one = run_passes(pkg, ctx, dev, bs.single(o))
        alone = {(g, k): a for g, k, a in _object_slices_of_single(one)}
        for g, key, a in _object_slices(w, o):
            if (g, key) not in alone:                                     # an object without a point has no culling Device of its own
                assert len(a) == 0 or key in ("thresholds",) or key.endswith(".count") and not a.any(), (bs.NAMES[o], key)
                continue
            assert same_bytes(alone[(g, key)], a), (bs.NAMES[o], g, key)


def _object_slices_of_single(one):
    for key, a in one["pt"].items():
        yield "pt", key, a
    for key, a in one["kp"].items():
        yield "kp", key, a
    for key, a in one["obj"].items():
        yield "obj", key, a[0:1]
    for name, (off, arrays) in one["rag"].items():
        yield "rag", name + ".count", np.asarray([int(off[1]) - int(off[0])])
        for key, a in arrays.items():
            yield "rag", name + "." + key, a[int(off[0]):int(off[1])]


def test_plain_block_order_gives_the_same_bytes(pkg, gpu, monkeypatch):
    w = whole_run(pkg, gpu)
    p = plain_run(pkg, gpu[1], monkeypatch)
    for group in ("pt", "kp", "obj"):
        assert sorted(p[group]) == sorted(w[group])
        for key in w[group]:
            assert same_bytes(p[group][key], w[group][key]), (group, key)
    assert sorted(p["rag"]) == sorted(w["rag"])
    for name, (off, arrays) in w["rag"].items():
        assert np.array_equal(p["rag"][name][0], off), name
        for key, a in arrays.items():
            assert same_bytes(p["rag"][name][1][key], a), (name, key)
