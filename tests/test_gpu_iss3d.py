"""ISS3D keypoints on the MI355X (ismhip_iss3d_saliency, ismhip_iss3d_keypoints) against the restatement tests/iss3d_ref.py.

Tolerances: saliency and eigenvalues within MARGIN * e1 = 1e-9 * e1 of the restatement (derived in iss3d_ref.py; the device rounds every
product to 2^-44 of the squared radius, about 1e-13 * e1 in the sum). Neighbour counts, the keypoint set, its order, positions, colours
and source indices are exact on every point the restatement calls decided; at most 1 % of a scene may be undecided."""
import numpy as np
import pytest

import iss3d_ref as ref
import iss3d_scenes as scenes

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _cloud(pkg, ctx, dev, objs, cell, rgba=None):
    """objs: list of float32 [n, 3] -> (Cloud, pt_off)"""
    pt_off = np.zeros(len(objs) + 1, np.uint32)
    pt_off[1:] = np.cumsum([len(o) for o in objs])
    xyz = np.concatenate([np.asarray(o, np.float32).reshape(-1, 3) for o in objs]) if len(objs) else np.zeros((0, 3), np.float32)
    pad = max(len(xyz), 1)                                              # an empty batch still hands over valid pointers
    t = [_dev(np.resize(xyz[:, i], pad) if len(xyz) else np.zeros(pad, np.float32), dev) for i in range(3)] + [_dev(np.zeros(pad, np.float32), dev) for _ in range(3)]
    c = None if rgba is None else _dev(np.asarray(rgba, np.int32), dev)
    return pkg.capi.Cloud(ctx, pt_off, *t, cell, rgba=c) if rgba is not None else pkg.capi.Cloud(ctx, pt_off, *t, cell), pt_off


def _run(pkg, ctx, cloud, rs, rn, g21=scenes.GAMMA, g32=scenes.GAMMA, mn=scenes.MIN_NEIGHBORS):
    capi = pkg.capi
    sal, eig, cnt = capi.iss3d_saliency(ctx, cloud, rs, g21, g32, mn)
    ko, kx, ky, kz, kc, src = capi.iss3d_keypoints(ctx, cloud, rs, rn, g21, g32, mn)
    ctx.sync()
    return dict(saliency=sal.cpu().numpy(), eig=eig.cpu().numpy(), count=cnt.cpu().numpy(), off=ko,
                kxyz=np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1), krgba=None if kc is None else kc.cpu().numpy(),
                src=src.cpu().numpy())


def _check_object(got, o, b, e, xyz, want, rgba=None, tag=""):
    """the device answer of object o (points [b, e) of the batch) against the restatement `want`"""
    e1 = want["eig"][:, 0]
    tol = ref.MARGIN * e1
    ds = np.abs(got["saliency"][b:e] - want["saliency"]); de = np.abs(got["eig"][b:e] - want["eig"]).max(1)
    dec_s = ~want["undecided_saliency"]
    rel = np.where(e1 > 0, np.maximum(np.where(dec_s, ds, 0), de) / np.where(e1 > 0, e1, 1), 0).max() if len(e1) else 0.0
    kb, ke = int(got["off"][o]), int(got["off"][o + 1])
    src = got["src"][kb:ke]
    und = want["undecided"]
    print("%s object %d: n %d keypoints gpu %d ref %d undecided %d max |saliency, eig| err %.3g e1" % (tag, o, e - b, ke - kb, want["keep"].sum(), und.sum(), rel))
    assert np.array_equal(got["count"][b:e], want["count"])
    assert (de <= tol).all()
    assert (ds[dec_s] <= tol[dec_s]).all()
    assert (np.diff(src) > 0).all() and (src >= 0).all() and (src < e - b).all()                 # ascending original index
    keep = np.zeros(e - b, bool); keep[src] = True
    assert np.array_equal(keep[~und], want["keep"][~und])
    assert np.array_equal(got["kxyz"][kb:ke].view(np.uint32), xyz[src].view(np.uint32))          # the points themselves
    if rgba is not None:
        assert np.array_equal(got["krgba"][kb:ke], rgba[b:e][src])
    return int(und.sum())


@pytest.mark.parametrize("gammas", scenes.GAMMAS)
def test_scenes_match_restatement(pkg, gpu, gammas):
    ctx, dev = gpu
    rng = np.random.default_rng(5)
    for k, (n, rs, rn, _seed) in enumerate(scenes.SCENES):
        xyz = scenes.scene(k)
        rgba = rng.integers(0, 1 << 24, n).astype(np.int32)
        cloud, _po = _cloud(pkg, ctx, dev, [xyz], 0.4 * rn, rgba=rgba)
        got = _run(pkg, ctx, cloud, rs, rn, *gammas)
        cloud.close()
        want = scenes.answer(k, gammas)
        n_und = _check_object(got, 0, 0, n, xyz, want, rgba, "scene %d" % k)
        assert n_und <= 0.01 * n
        assert got["off"][1] >= 40                                       # a detector, not an empty answer


def test_lattice_counts_are_exact(pkg, gpu):
    ctx, dev = gpu
    xyz = scenes.lattice()
    cloud, _po = _cloud(pkg, ctx, dev, [xyz], 1.0 / 64.0)
    sal, eig, cnt = pkg.capi.iss3d_saliency(ctx, cloud, scenes.LATTICE_RADIUS)
    assert np.array_equal(cnt.cpu().numpy(), scenes.lattice_counts())
    want = ref.iss3d(xyz, scenes.LATTICE_RADIUS, scenes.LATTICE_RADIUS)
    assert (np.abs(eig.cpu().numpy() - want["eig"]).max(1) <= ref.MARGIN * want["eig"][:, 0]).all()
    cloud.close()


def test_plane_and_small_cluster_have_no_keypoints(pkg, gpu):
    ctx, dev = gpu
    cloud, _po = _cloud(pkg, ctx, dev, [scenes.plane(), scenes.small_cluster()], 0.02)
    got = _run(pkg, ctx, cloud, 0.05, 0.03)
    cloud.close()
    n = len(scenes.plane())
    assert np.array_equal(got["off"], [0, 0, 0]) and not got["saliency"].any()
    assert np.array_equal(got["eig"][:n, 2], np.zeros(n)) and (got["eig"][:n, 0] > 0).all()     # e3 exactly 0 on the plane
    assert np.array_equal(got["count"][n:], [4, 4, 4, 4]) and not got["eig"][n:].any()           # below MinNeighbors: the zero matrix


def _batch_objects():
    """objects of 0, 1, 63, 64, 65 and 257 points (cut from scene 2, whose radii suit a 700-point sampling)"""
    p = scenes.scene(2)
    return [p[:0], p[:1], p[100:163], p[200:264], p[300:365], p[400:657]]


def test_small_and_empty_objects_in_one_batch(pkg, gpu):
    ctx, dev = gpu
    objs = _batch_objects()
    rs, rn = 0.3, 0.2                                                   # sparse cuts: wide balls so that the larger objects are searched
    cloud, po = _cloud(pkg, ctx, dev, objs, 0.1)
    got = _run(pkg, ctx, cloud, rs, rn)
    cloud.close()
    assert got["off"][0] == 0 and got["off"][1] == 0 and got["off"][2] == 0          # 0 and 1 points: no keypoint
    n_kp = 0
    for o, xyz in enumerate(objs):
        want = ref.iss3d(xyz, rs, rn, scenes.GAMMA, scenes.GAMMA, scenes.MIN_NEIGHBORS)
        assert _check_object(got, o, int(po[o]), int(po[o + 1]), xyz, want, tag="sizes") == 0
        n_kp += int(want["keep"].sum())
    assert n_kp > 0 and got["off"][-1] == n_kp


def test_batch_with_an_empty_object_between(pkg, gpu):
    ctx, dev = gpu
    objs = [scenes.scene(2), scenes.scene(2)[:0], scenes.scene(0)]                  # [700, 0, 2048]
    rs, rn = scenes.SCENES[0][1], scenes.SCENES[0][2]
    cloud, po = _cloud(pkg, ctx, dev, objs, 0.03)
    got = _run(pkg, ctx, cloud, rs, rn)
    cloud.close()
    assert got["off"][1] == got["off"][2]
    assert _check_object(got, 0, 0, 700, objs[0], ref.iss3d(objs[0], rs, rn), tag="[700, 0, 2048]") <= 7
    assert _check_object(got, 2, 700, 2748, objs[2], scenes.answer(0), tag="[700, 0, 2048]") <= 20
    assert got["off"][3] - got["off"][2] == scenes.answer(0)["keep"].sum()


def test_non_finite_points_are_neither_neighbours_nor_keypoints(pkg, gpu):
    ctx, dev = gpu
    n, rs, rn, _seed = scenes.SCENES[2]
    xyz = scenes.scene(2).copy()
    bad = np.arange(3, n, 9)
    xyz[bad[0::3], 0] = np.nan; xyz[bad[1::3], 1] = np.inf; xyz[bad[2::3]] = -np.inf
    cloud, _po = _cloud(pkg, ctx, dev, [xyz], 0.05)
    got = _run(pkg, ctx, cloud, rs, rn)
    cloud.close()
    want = ref.iss3d(xyz, rs, rn)
    assert not got["saliency"][bad].any() and not got["eig"][bad].any() and not got["count"][bad].any()
    assert _check_object(got, 0, 0, n, xyz, want, tag="NaN") <= 7
    assert not np.isin(got["src"], bad).any() and len(got["src"]) > 10


def test_salient_radius_larger_than_the_object(pkg, gpu):
    """every point is a neighbour of every point: 2048 candidates per query, more than one block of the candidate sweep"""
    ctx, dev = gpu
    xyz = scenes.scene(0)
    cloud, _po = _cloud(pkg, ctx, dev, [xyz], 0.05)
    sal, eig, cnt = pkg.capi.iss3d_saliency(ctx, cloud, 2.0)
    cnt = cnt.cpu().numpy(); eig = eig.cpu().numpy()
    cloud.close()
    assert (cnt == len(xyz)).all()
    p = xyz.astype(np.float64)
    S, m = p.T @ p, p.sum(0)
    for i in range(0, len(xyz), 97):                                    # sum (p_j - q)(p_j - q)^T = S - m q^T - q m^T + n q q^T
        q = p[i]
        w = np.linalg.eigvalsh(S - np.outer(m, q) - np.outer(q, m) + len(p) * np.outer(q, q))
        assert np.abs(eig[i] - w[::-1]).max() <= ref.MARGIN * w[2]


def test_results_do_not_depend_on_the_cell_size_or_the_run(pkg, gpu):
    ctx, dev = gpu
    n, rs, rn, _seed = scenes.SCENES[0]
    xyz = scenes.scene(0)
    runs = []
    for cell in (0.25 * rs, 0.25 * rs, 4.0 * rs):                      # the same call twice, then a cloud with cells of four radii
        cloud, _po = _cloud(pkg, ctx, dev, [xyz], cell)
        runs.append(_run(pkg, ctx, cloud, rs, rn))
        cloud.close()
    for other in runs[1:]:
        for key in ("saliency", "eig"):
            assert np.array_equal(runs[0][key].view(np.uint64), other[key].view(np.uint64))
        for key in ("count", "off", "src"):
            assert np.array_equal(runs[0][key], other[key])
        assert np.array_equal(runs[0]["kxyz"].view(np.uint32), other["kxyz"].view(np.uint32))


def test_wave_mapping_gives_the_same_bits(pkg, gpu, monkeypatch):
    """ISMHIP_ISS3D_MAP=wave (read when a context is created): one wave per query instead of one thread per query. The scatter sums are
    order free, so the two kernels must agree bit for bit -- also with every point a neighbour (several candidate blocks per wave)."""
    ctx, dev = gpu
    monkeypatch.setenv("ISMHIP_ISS3D_MAP", "wave")
    ctx_w = pkg.capi.Ctx(0)
    monkeypatch.delenv("ISMHIP_ISS3D_MAP")
    objs = [scenes.scene(0), scenes.scene(2)[:65], scenes.scene(2)]
    for rs, rn in ((0.1, 0.06), (2.0, 0.06)):
        got = []
        for c in (ctx, ctx_w):
            cloud, _po = _cloud(pkg, c, dev, objs, 0.03)
            got.append(_run(pkg, c, cloud, rs, rn))
            cloud.close()
        for key in ("saliency", "eig"):
            assert np.array_equal(got[0][key].view(np.uint64), got[1][key].view(np.uint64)), (rs, key)
        for key in ("count", "off", "src"):
            assert np.array_equal(got[0][key], got[1][key]), (rs, key)
        if rs > 1:
            assert got[0]["count"][:2048].min() == 2048
        else:
            assert got[0]["off"][-1] > 100
    ctx_w.close()


def test_capacity_one_too_small_is_refused(pkg, gpu):
    ctx, dev = gpu
    n, rs, rn, _seed = scenes.SCENES[2]
    cloud, _po = _cloud(pkg, ctx, dev, [scenes.scene(2)], 0.05)
    ko, kx, _ky, _kz, _kc, _src = pkg.capi.iss3d_keypoints(ctx, cloud, rs, rn)
    m = int(ko[-1])
    assert m == len(kx) and m > 10
    ko2 = pkg.capi.iss3d_keypoints(ctx, cloud, rs, rn, capacity=m)[0]               # exactly enough
    assert np.array_equal(ko, ko2)
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*capacity"):
        pkg.capi.iss3d_keypoints(ctx, cloud, rs, rn, capacity=m - 1)
    cloud.close()


def test_bad_arguments_are_refused(pkg, gpu):
    ctx, dev = gpu
    cloud, _po = _cloud(pkg, ctx, dev, [scenes.small_cluster()], 0.05)
    for kw in (dict(salient_radius=0.0), dict(salient_radius=-1.0), dict(gamma21=0.0), dict(gamma32=-0.1), dict(min_neighbors=-1)):
        args = dict(salient_radius=0.1, gamma21=0.9, gamma32=0.9, min_neighbors=5); args.update(kw)
        with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\)"):
            pkg.capi.iss3d_saliency(ctx, cloud, **args)
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\)"):
        pkg.capi.iss3d_keypoints(ctx, cloud, 0.1, 0.0)
    cloud.close()


def test_empty_cloud(pkg, gpu):
    ctx, dev = gpu
    cloud, _po = _cloud(pkg, ctx, dev, [scenes.scene(0)[:0], scenes.scene(0)[:0]], 0.05)
    ko, kx, _ky, _kz, _kc, src = pkg.capi.iss3d_keypoints(ctx, cloud, 0.1, 0.05)
    assert np.array_equal(ko, [0, 0, 0]) and len(kx) == 0 and len(src) == 0
    sal, _eig, _cnt = pkg.capi.iss3d_saliency(ctx, cloud, 0.1)
    assert sal.numel() == 0
    cloud.close()


def test_timers_report_both_passes(pkg, gpu):
    ctx, dev = gpu
    n, rs, rn, _seed = scenes.SCENES[2]
    cloud, _po = _cloud(pkg, ctx, dev, [scenes.scene(2)], 0.05)
    ctx.timers_enable(True); ctx.timers_reset()
    pkg.capi.iss3d_keypoints(ctx, cloud, rs, rn)
    ctx.sync()
    for key in ("iss3d_saliency", "iss3d_nms"):
        ms, launches = ctx.timer(key)
        assert launches == 1 and ms > 0.0
    ctx.timers_enable(False)
    cloud.close()
