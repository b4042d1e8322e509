"""SIFT3D keypoints on the MI355X, stage by stage (ismhip_normal_curvature, ismhip_voxel_downsample_xyzi, ismhip_sift3d_scale_space,
ismhip_sift3d_extrema) and the driver ismhip_sift3d_keypoints, against the restatement tests/sift3d_ref.py.

Tolerances: every dog value within the bound the restatement derives beside it (sift3d_ref.py: exponential, the two fixed-point quanta,
the float roundings); voxel intensities within voxel_mean_bound of the float64 mean. Counts, neighbour lists, positions, order and
offsets are exact; extremum flags are exact on every test the restatement calls decided, at most 2 % of a scene may be undecided."""
import numpy as np
import pytest

import sift3d_ref as ref
import sift3d_scenes as scenes
from iss3d_scenes import bumpy_ellipsoid

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.array(a, copy=True, order="C")).to(dev)


def _cloud(pkg, ctx, dev, objs, cell):
    """objs: list of float32 [n, 3] -> (Cloud, pt_off, xyz)"""
    pt_off = np.zeros(len(objs) + 1, np.uint32)
    pt_off[1:] = np.cumsum([len(o) for o in objs])
    xyz = np.concatenate([np.asarray(o, np.float32).reshape(-1, 3) for o in objs]) if len(objs) else np.zeros((0, 3), np.float32)
    pad = max(len(xyz), 1)                                              # an empty batch still hands over valid pointers
    t = [_dev(np.resize(xyz[:, i], pad) if len(xyz) else np.zeros(pad, np.float32), dev) for i in range(3)] + [_dev(np.zeros(pad, np.float32), dev) for _ in range(3)]
    return pkg.capi.Cloud(ctx, pt_off, *t, cell), pt_off, xyz


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- normal curvature ---------------------------------------------------------------------------------------------------------
def test_normal_curvature_is_the_culling_score_bit_for_bit(pkg, gpu):
    ctx, dev = gpu
    capi = pkg.capi
    a = bumpy_ellipsoid(900, 21).copy()
    a[17] = np.nan                                                        # a NaN position
    sparse = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.012, 0], [3, 3, 3], [3.01, 3, 3], [9, 9, 9]], np.float32)   # balls of 3, 2 and 1 points
    b = bumpy_ellipsoid(600, 22)
    objs = [a, np.zeros((0, 3), np.float32), sparse, b]
    radius = 0.08
    cloud, pt_off, xyz = _cloud(pkg, ctx, dev, objs, 0.05)
    curv, cnt = capi.normal_curvature(ctx, cloud, radius)
    kx, ky, kz = (_dev(xyz[:, i], dev) for i in range(3))
    geo, _col, kcnt = capi.culling_scores(ctx, cloud, pt_off, kx, ky, kz, None, radius, geometry="curvature")
    ctx.sync()
    curv, cnt, geo, kcnt = curv.cpu().numpy(), cnt.cpu().numpy(), geo.cpu().numpy(), kcnt.cpu().numpy()
    fin = np.isfinite(xyz).all(1)
    assert np.array_equal(_bits(curv[fin]), _bits(geo[fin])) and np.array_equal(cnt[fin], kcnt[fin])
    assert np.isnan(curv[~fin]).all() and (cnt[~fin] == 0).all()
    s = int(pt_off[2])
    assert cnt[s:s + 6].tolist() == [3, 3, 3, 2, 2, 1]
    assert np.isfinite(curv[s:s + 3]).all() and np.isnan(curv[s + 3:s + 6]).all()
    ok = np.isfinite(curv)
    print("curvature: %d points, %d finite scores, range %.3g .. %.3g" % (len(curv), ok.sum(), curv[ok].min(), curv[ok].max()))
    assert ok.sum() > 1300 and (curv[ok] >= 0).all() and (curv[ok] <= 1.0 / 3.0 + 1e-6).all()
    cloud.close()


# ---- downsample ---------------------------------------------------------------------------------------------------------------
def test_downsample_positions_and_intensities(pkg, gpu):
    ctx, dev = gpu
    capi = pkg.capi
    a = bumpy_ellipsoid(1500, 31); b = bumpy_ellipsoid(700, 32)
    b = np.concatenate([b, np.array([[2.0, 2.0, 2.0]], np.float32)])      # a voxel that holds one point
    objs = [a, np.zeros((0, 3), np.float32), b]
    inten = [scenes.field(a, 31), np.zeros(0, np.float32), scenes.field(b, 32)]
    pt_off = np.zeros(4, np.uint32); pt_off[1:] = np.cumsum([len(o) for o in objs])
    xyz = np.concatenate(objs); I = np.concatenate(inten)
    leaf = 0.07
    t = [_dev(xyz[:, i], dev) for i in range(3)]
    ko, kx, ky, kz, ki = capi.voxel_downsample_xyzi(ctx, pt_off, *t, _dev(I, dev), leaf)
    vo, vx, vy, vz, _ = capi.voxel_keypoints(ctx, pt_off, *t, leaf)
    ctx.sync()
    assert np.array_equal(ko, vo) and ko[1] == ko[2] and ko[1] > 100 and ko[3] - ko[2] > 50
    for g, w in ((kx, vx), (ky, vy), (kz, vz)):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w.cpu().numpy()))
    ki = ki.cpu().numpy()
    worst = 0.0
    for o in (0, 2):
        mean64, counts = ref.voxel_means(objs[o], inten[o], leaf)
        got = ki[ko[o]:ko[o + 1]].astype(np.float64)
        assert len(mean64) == len(got)
        bound = ref.voxel_mean_bound(mean64, np.abs(inten[o]).max())
        worst = max(worst, float((np.abs(got - mean64) / bound).max()))
        assert (np.abs(got - mean64) <= bound).all()
        single = counts == 1
        assert single.any() and np.array_equal(got[single], mean64[single])          # one point: its own intensity, exactly
    print("voxel intensities: worst error / bound %.3f" % worst)
    assert _bits(ki[ko[3] - 1:ko[3]])[0] == _bits(inten[2][-1:])[0]                   # the far point's voxel is the last one


# ---- scale space --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scale_space(pkg, gpu):
    """every scene on two cell sizes, the second one twice: per scene a list of (dog, counts)"""
    ctx, dev = gpu
    out = []
    for k in range(len(scenes.SCENES)):
        xyz, inten, sc = scenes.scene(k)
        runs = []
        for cell in (0.4 * 3.0 * float(sc[-1]), 0.09, 0.09):
            cloud, _po, _x = _cloud(pkg, ctx, dev, [xyz], cell)
            dog, cnt = pkg.capi.sift3d_scale_space(ctx, cloud, _dev(inten, dev), sc)
            ctx.sync()
            runs.append((dog.cpu().numpy(), cnt.cpu().numpy()))
            cloud.close()
        out.append(runs)
    return out


@pytest.mark.parametrize("k", range(len(scenes.SCENES)))
def test_scale_space_within_its_bound(scale_space, k):
    want = scenes.answer(k)
    dog, cnt = scale_space[k][0]
    ratio = np.abs(dog.astype(np.float64) - want["dog"]) / want["bound"]
    print("scene %d: worst error / bound %.3f, largest bound %.2e, largest |dog| %.3e" % (k, ratio.max(), want["bound"].max(), np.abs(want["dog"]).max()))
    assert np.array_equal(cnt, want["count"])
    assert (ratio <= 1.0).all()
    for other in scale_space[k][1:]:                                      # another cell size, another run: the same bits
        assert np.array_equal(_bits(other[0]), _bits(dog)) and np.array_equal(other[1], cnt)


def test_scale_space_boundary_isolated_and_nonfinite(pkg, gpu):
    ctx, dev = gpu
    capi = pkg.capi
    lat = scenes.lattice()
    rng = np.random.default_rng(5)
    lat_i = rng.uniform(0.25, 1.0, len(lat)).astype(np.float32)
    iso = np.array([[0, 0, 0], [5, 5, 5], [np.nan, 0, 0], [5.001, 5, 5]], np.float32)
    iso_i = np.array([0.75, -0.25, 0.5, np.inf], np.float32)            # the last one's intensity is not finite: not a neighbour, NaN row
    cloud, pt_off, xyz = _cloud(pkg, ctx, dev, [lat, iso], 1.0 / 16.0)
    I = _dev(np.concatenate([lat_i, iso_i]), dev)
    for sc, reach2 in ((np.array([1 / 128, 1 / 64, 1 / 32], np.float32), 36), (np.array([1 / 128, 1 / 64, 1 / 64], np.float32), 9)):
        dog, cnt = capi.sift3d_scale_space(ctx, cloud, I, sc)
        ctx.sync()
        dog, cnt = dog.cpu().numpy(), cnt.cpu().numpy()
        n = len(lat)
        assert np.array_equal(cnt[:n], scenes.lattice_counts(reach2=reach2))       # the points at exactly d2 == 9 s2 count
        D, B, c = ref.dog(lat, lat_i, sc)
        assert np.array_equal(c, cnt[:n]) and (np.abs(dog[:n] - D) <= B).all()
        assert cnt[n:].tolist() == [1, 1, 0, 0]
        assert np.array_equal(dog[n:n + 2], np.zeros((2, 2), np.float32))           # response = own intensity at every scale
        assert np.isnan(dog[n + 2:]).all()
    for bad in ([0.1, 0.2], [0.1] * 17, [0.1, -0.2, 0.3], [0.1, float("nan"), 0.3]):
        with pytest.raises(capi.IsmHipError):
            capi.sift3d_scale_space(ctx, cloud, I, np.array(bad, np.float32))
    cloud.close()


# ---- extrema ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(scenes.SCENES)))
def test_extrema_flags_and_neighbours(pkg, gpu, scale_space, k):
    ctx, dev = gpu
    xyz, _inten, sc = scenes.scene(k)
    want = scenes.answer(k)
    dog = scale_space[k][0][0]
    cloud, _po, _x = _cloud(pkg, ctx, dev, [xyz], 0.4 * 3.0 * float(sc[-1]))
    flags, nn = pkg.capi.sift3d_extrema(ctx, cloud, _dev(dog, dev))
    ctx.sync()
    flags, nn = flags.cpu().numpy(), nn.cpu().numpy()
    cloud.close()
    und = want["undecided"]
    share = scenes.undecided_share(want)
    print("scene %d: gpu %d minima %d maxima, ref %d / %d, undecided share %.4f" %
          (k, (flags == 1).sum(), (flags == 2).sum(), (want["flags"] == 1).sum(), (want["flags"] == 2).sum(), share))
    assert np.array_equal(nn, want["nn"])
    assert share <= 0.02
    assert np.array_equal(flags[~und], want["flags"][~und])
    assert not flags[:, 0].any() and not flags[:, -1].any()
    # the device's own columns leave nothing undecided: the restatement on them, as exact values, gives the device's flags everywhere
    f2, u2, _ = ref.extrema(xyz, dog.astype(np.float64), None, nn=want["nn"])
    assert not u2.any() and np.array_equal(flags, f2)


def test_extrema_ties_small_objects_and_k(pkg, gpu):
    ctx, dev = gpu
    capi = pkg.capi
    rng = np.random.default_rng(7)
    lat = scenes.lattice(5)                                               # exact distance ties everywhere
    dup = np.concatenate([lat[:40], lat[:40], np.array([[np.nan, 0, 0]], np.float32)])     # every point twice, and a NaN
    ten = rng.normal(size=(10, 3)).astype(np.float32)
    objs = [lat, dup, ten, np.zeros((0, 3), np.float32)]
    cloud, pt_off, xyz = _cloud(pkg, ctx, dev, objs, 0.05)
    n = len(xyz)
    dog = rng.normal(size=(n, 5)).astype(np.float32)
    for k in (25, 1, 64, 7):
        flags, nn = capi.sift3d_extrema(ctx, cloud, _dev(dog, dev), k=k)
        ctx.sync()
        flags, nn = flags.cpu().numpy(), nn.cpu().numpy()
        for o in range(len(objs)):
            b, e = int(pt_off[o]), int(pt_off[o + 1])
            f, u, wnn = ref.extrema(xyz[b:e], dog[b:e].astype(np.float64), None, k=k)
            assert np.array_equal(nn[b:e], wnn), (k, o)
            assert np.array_equal(flags[b:e], f), (k, o)
        b = int(pt_off[2])
        assert (nn[b:b + 10, :min(k, 10)] >= 0).all() and (nn[b:b + 10, 10:] == -1).all()   # 10 points: all of them, then -1
        if k == 1:   # no neighbour but itself: the point's own three columns decide (a duplicate's one neighbour may be its twin)
            own = (dog[:, 1:-1] > dog[:, :-2]) & (dog[:, 1:-1] > dog[:, 2:])
            for o in (0, 2):
                b, e = int(pt_off[o]), int(pt_off[o + 1])
                assert np.array_equal(nn[b:e, 0], np.arange(e - b)) and np.array_equal(flags[b:e, 1:-1] == 2, own[b:e])
            b = int(pt_off[1])
            assert np.array_equal(nn[b + 40:b + 80, 0], np.arange(40))   # the second copies find the first ones: the lowest index wins
    const = _dev(np.full((n, 5), 0.25, np.float32), dev)                 # a plateau: strict comparisons give nothing
    flags, _ = capi.sift3d_extrema(ctx, cloud, const, want_nn=False)
    assert not flags.cpu().numpy().any()
    flags, _ = capi.sift3d_extrema(ctx, cloud, _dev(dog, dev), min_contrast=float(np.abs(dog).max()) * 1.5, want_nn=False)
    assert not flags.cpu().numpy().any()                                 # min_contrast above every |v|
    flags, _ = capi.sift3d_extrema(ctx, cloud, _dev(dog, dev), min_contrast=0.5, want_nn=False)
    f = flags.cpu().numpy()
    assert f.any() and (np.abs(dog)[f != 0] >= 0.5).all()
    with pytest.raises(capi.IsmHipError, match="not built"):
        capi.sift3d_extrema(ctx, cloud, _dev(dog, dev), k=65)
    cloud.close()


# ---- driver -------------------------------------------------------------------------------------------------------------------
def _by_hand(pkg, ctx, dev, objs, inten, min_scale, nr_octaves, nr_scales):
    """the four stage entries composed through the C ABI as the driver composes them -> (offsets, kp [n, 3], scale [n], sizes)"""
    capi = pkg.capi
    n_obj = len(objs)
    off = np.zeros(n_obj + 1, np.uint32); off[1:] = np.cumsum([len(o) for o in objs])
    xyz = np.concatenate(objs); I = np.concatenate(inten)
    cur = [_dev(xyz[:, i], dev) for i in range(3)] + [_dev(I, dev)]
    alive = np.ones(n_obj, bool)
    sizes = np.zeros((n_obj, nr_octaves), np.uint32)
    per_obj = [[] for _ in range(n_obj)]
    scale = np.float32(min_scale)
    for oc in range(nr_octaves):
        if int(off[-1]) == 0:
            break
        off, kx, ky, kz, ki = capi.voxel_downsample_xyzi(ctx, off, *cur, float(scale))
        n_o = np.diff(off.astype(np.int64))
        sizes[alive, oc] = n_o[alive]
        alive &= n_o >= capi.SIFT3D_MIN_POINTS
        if not alive.any():
            break
        sc = capi.sift3d_scales(float(scale), nr_scales)
        cloud = capi.Cloud(ctx, off, kx, ky, kz, kx, ky, kz, 0.123)     # any cell size
        dog, _ = capi.sift3d_scale_space(ctx, cloud, ki, sc, want_counts=False)
        flags, _ = capi.sift3d_extrema(ctx, cloud, dog, want_nn=False)
        ctx.sync()
        cloud.close()
        f = flags.cpu().numpy(); p = np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1)
        for o in np.nonzero(alive)[0]:
            for i in range(int(off[o]), int(off[o + 1])):
                for c in np.nonzero(f[i])[0]:
                    per_obj[o].append((p[i], sc[c]))
        cur = [kx, ky, kz, ki]
        scale = np.float32(scale * np.float32(2.0))
    ko = np.zeros(n_obj + 1, np.uint32); ko[1:] = np.cumsum([len(l) for l in per_obj])
    flat = [e for l in per_obj for e in l]
    kp = np.array([e[0] for e in flat], np.float32).reshape(-1, 3); ks = np.array([e[1] for e in flat], np.float32)
    return ko, kp, ks, sizes


def test_driver_equals_the_stages_by_hand(pkg, gpu):
    ctx, dev = gpu
    capi = pkg.capi
    a = bumpy_ellipsoid(3000, 41)                                         # goes through several octaves
    b = bumpy_ellipsoid(600, 42) * np.float32(0.2)                        # small: octave 1 falls below 25 points
    c = bumpy_ellipsoid(2000, 43)
    tiny = (bumpy_ellipsoid(40, 44) * np.float32(0.02)).astype(np.float32)   # fewer than 25 voxels at octave 0: an empty range
    objs = [a, b, np.zeros((0, 3), np.float32), c, tiny]
    inten = [scenes.field(o, 40 + i) if len(o) else np.zeros(0, np.float32) for i, o in enumerate(objs)]
    inten[3] = inten[3].copy(); inten[3][5] = np.nan                      # leaves the cloud before octave 0
    min_scale = 0.04
    cloud, pt_off, xyz = _cloud(pkg, ctx, dev, objs, 0.1)
    I = _dev(np.concatenate(inten), dev)
    ko, kx, ky, kz, ks, sizes = capi.sift3d_keypoints(ctx, cloud, I, min_scale)
    ctx.sync()
    kp = np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1); ks = ks.cpu().numpy()
    wo, wkp, wks, wsizes = _by_hand(pkg, ctx, dev, objs, inten, min_scale, 4, 3)
    print("driver: keypoints per object", np.diff(ko.astype(np.int64)).tolist(), "octave sizes", sizes.tolist())
    assert np.array_equal(ko, wo) and np.array_equal(sizes, wsizes)
    assert np.array_equal(_bits(kp), _bits(wkp)) and np.array_equal(_bits(ks), _bits(wks))
    n_kp = np.diff(ko.astype(np.int64))
    assert n_kp[0] >= 10 and n_kp[3] >= 10 and n_kp[2] == 0 and n_kp[4] == 0
    assert sizes[0, 1] >= 25                                              # the large object reaches octave 1
    assert sizes[1, 0] >= 25 and 0 < sizes[1, 1] < 25 and sizes[1, 2] == 0 and n_kp[1] > 0    # the small one stops there, its neighbours go on
    assert 0 < sizes[4, 0] < 25 and not sizes[4, 1:].any() and not sizes[2].any()
    oct0 = set(capi.sift3d_scales(min_scale, 3)[1:4].tolist())
    assert set(ks[ko[1]:ko[2]].tolist()) <= oct0                          # the stopped object's keypoints come from octave 0 only
    assert len(set(ks[ko[0]:ko[1]].tolist()) - oct0) > 0                  # the large one's also from later octaves
    # again: the same bits
    ko2, kx2, ky2, kz2, ks2, _ = capi.sift3d_keypoints(ctx, cloud, I, min_scale)
    assert np.array_equal(ko2, ko) and np.array_equal(_bits(kx2.cpu().numpy()), _bits(kp[:, 0])) and np.array_equal(_bits(ks2.cpu().numpy()), _bits(ks))
    # capacity one too small: refused, nothing written
    total = int(ko[-1])
    with pytest.raises(capi.IsmHipError, match="capacity"):
        capi.sift3d_keypoints(ctx, cloud, I, min_scale, capacity=total - 1)
    import torch
    import ctypes as C
    sentinel = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
    outs = [sentinel.clone() for _ in range(4)]
    off_h = np.full(len(objs) + 1, 99, np.uint32)
    rc = capi.lib().ismhip_sift3d_keypoints(ctx._h, cloud._h, capi._p(I), C.c_float(min_scale), C.c_int(4), C.c_int(3), C.c_float(0.0), C.c_uint32(total - 1),
                                            *[capi._p(t) for t in outs], capi._p(off_h), C.c_void_p(0))
    ctx.sync()
    assert rc == -1 and not off_h.any()
    assert all(bool((t == -7.0).all()) for t in outs)
    ko3, *_ = capi.sift3d_keypoints(ctx, cloud, I, min_scale, capacity=total)
    assert np.array_equal(ko3, ko)
    cloud.close()
