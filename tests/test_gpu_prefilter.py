"""Point-cloud pre-filters on the MI355X against the restatement in tests/prefilter_ref.py: the C ABI (ismhip_filter_statistical,
ismhip_filter_radius, ismhip_filter_passthrough_z, ismhip_compact_points) and the C++ host (train() / detectBatch() with the filters
enabled against the same calls, filters off, on clouds the restatement filtered)."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
import prefilter_ref as ref
from test_threshold_host import _last_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
MEAN_K, STDDEV_MUL = 20, 2.0

pytestmark = pytest.mark.gpu


def _contaminated(syn):
    """four classes x (2048, 16384) surface points, each with 3 % uniform outliers in the cube +-1.2 appended; then an object with fewer
    than MeanK + 1 points, one with exact duplicates and one with a few non-finite points. -> list of (xyz, n_surface)"""
    rng = np.random.default_rng(7)
    objs = []
    for cls in range(4):
        for n in (2048, 16384):
            xyz, _ = syn.make_object(cls, 1, cls, n_points=n)
            out = rng.uniform(-1.2, 1.2, size=(int(0.03 * n), 3)).astype(np.float32)
            objs.append((np.concatenate([xyz, out]).astype(np.float32), n))
    small, _ = syn.make_object(0, 2, 0, n_points=MEAN_K - 8)
    objs.append((small, len(small)))
    base, _ = syn.make_object(1, 2, 1, n_points=2048)
    dup = np.concatenate([base, base[::8], base[:40], base[:40]]).astype(np.float32)      # up to three copies of a point
    objs.append((dup, len(dup)))
    bad, _ = syn.make_object(2, 2, 2, n_points=2048)
    bad = bad.copy()
    bad[5, 0] = np.nan; bad[700, 1] = np.inf; bad[701, 2] = -np.inf; bad[2047] = np.nan; bad[0, 2] = np.nan
    objs.append((bad, len(bad)))
    return objs


@pytest.fixture(scope="module")
def batch(pkg):
    objs = _contaminated(pkg.synthetic)
    pt_off = np.zeros(len(objs) + 1, np.uint32)
    pt_off[1:] = np.cumsum([len(o[0]) for o in objs])
    xyz = np.concatenate([o[0] for o in objs])
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=xyz.shape).astype(np.float32)
    rgba = rng.integers(0, 1 << 24, len(xyz)).astype(np.int32)
    return dict(objs=objs, pt_off=pt_off, xyz=xyz, nrm=nrm, rgba=rgba)


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _cloud(pkg, ctx, dev, b, cell):
    t = [_dev(b["xyz"][:, i], dev) for i in range(3)] + [_dev(b["nrm"][:, i], dev) for i in range(3)]
    return pkg.capi.Cloud(ctx, b["pt_off"], *t, cell), t


def test_statistical_outlier_removal_matches_restatement(pkg, gpu, batch):
    ctx, dev = gpu
    capi = pkg.capi
    runs = []
    for cell in (0.08, 0.08, 0.23):                                 # the same call twice, then a cloud with another cell size
        cloud, _t = _cloud(pkg, ctx, dev, batch, cell)
        keep, md, thr = capi.filter_statistical(ctx, cloud, MEAN_K, STDDEV_MUL)
        ctx.sync()
        runs.append((keep.cpu().numpy().copy(), md.cpu().numpy().copy(), thr.copy()))
        cloud.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0])
        assert np.array_equal(runs[0][1].view(np.uint32), other[1].view(np.uint32))
        assert np.array_equal(runs[0][2].view(np.uint64), other[2].view(np.uint64))
    keep, md, thr = runs[0]
    po = batch["pt_off"]
    n_band = 0
    for o, (xyz, n_surf) in enumerate(batch["objs"]):
        b, e = int(po[o]), int(po[o + 1])
        k_ref, md_ref, thr_ref = ref.sor(xyz, MEAN_K, STDDEV_MUL)
        k_gpu, md_gpu, thr_gpu = keep[b:e].astype(bool), md[b:e], thr[o]
        fin = ref.finite(xyz)
        assert np.array_equal(np.isnan(md_gpu), np.isnan(md_ref))
        assert not k_gpu[~fin].any()
        if not np.isfinite(thr_ref):                                # fewer than MeanK + 1 finite points: kept whole
            assert np.isinf(thr_gpu) and thr_gpu > 0 and np.array_equal(k_gpu, fin)
            continue
        with np.errstate(invalid="ignore"):
            rel = np.abs(md_gpu[fin].astype(np.float64) - md_ref[fin]) / md_ref[fin]
        print("object %d: n %d mean_dist max rel err %.3g thr gpu %.9g ref %.9g" % (o, e - b, np.nanmax(rel), thr_gpu, thr_ref))
        assert np.nanmax(rel) <= 1e-6                               # nanmax: 0 / 0 where duplicates give a zero mean distance
        assert np.array_equal(md_gpu[fin][md_ref[fin] == 0], md_ref[fin][md_ref[fin] == 0])
        assert np.array_equal(k_gpu[fin], ~(md_gpu[fin].astype(np.float64) > thr_gpu))
        assert abs(thr_gpu - ref.sor_threshold(md_gpu, STDDEV_MUL)) <= 1e-9 * thr_gpu
        band = fin & (np.abs(np.nan_to_num(md_ref).astype(np.float64) - thr_ref) <= 1e-5 * thr_ref)
        n_band += int(band.sum())
        assert np.array_equal(k_gpu[~band], k_ref[~band])
        if o < 8:                                                   # the filter does what it is for: most outliers go, the surface stays
            removed = ~k_ref
            assert removed[:n_surf].sum() == 0 and removed[n_surf:].sum() >= 0.75 * (len(xyz) - n_surf)
    assert n_band == 0


def test_statistical_outlier_removal_mean_k_range(pkg, gpu, batch):
    ctx, dev = gpu
    capi = pkg.capi
    sel = [0, 2, 8, 9, 10]                                           # the 2048-point objects and the three special ones
    objs = [batch["objs"][i][0] for i in sel]
    pt_off = np.zeros(len(objs) + 1, np.uint32); pt_off[1:] = np.cumsum([len(x) for x in objs])
    xyz = np.concatenate(objs)
    b = dict(pt_off=pt_off, xyz=xyz, nrm=np.zeros_like(xyz))
    cloud, _t = _cloud(pkg, ctx, dev, b, 0.05)
    for k, mul in ((1, 1.0), (7, 0.5), (64, 1.0)):
        keep, md, thr = capi.filter_statistical(ctx, cloud, k, mul)
        keep, md = keep.cpu().numpy().astype(bool), md.cpu().numpy()
        for o, p in enumerate(objs):
            s, e = int(pt_off[o]), int(pt_off[o + 1])
            k_ref, md_ref, thr_ref = ref.sor(p, k, mul)
            fin = np.isfinite(md_ref)
            assert np.array_equal(np.isnan(md[s:e]), ~fin)
            if fin.any():
                with np.errstate(invalid="ignore"):
                    assert np.nanmax(np.abs(md[s:e][fin].astype(np.float64) - md_ref[fin]) / md_ref[fin]) <= 1e-6
                assert abs(thr[o] - thr_ref) <= 1e-6 * thr_ref
            near = fin & (np.abs(np.nan_to_num(md_ref).astype(np.float64) - thr_ref) <= 1e-5 * thr_ref)
            assert np.array_equal(keep[s:e][~near], k_ref[~near])
    with pytest.raises(capi.IsmHipError):
        capi.filter_statistical(ctx, cloud, 0, 1.0)
    with pytest.raises(capi.IsmHipError):
        capi.filter_statistical(ctx, cloud, 65, 1.0)
    cloud.close()


def test_radius_outlier_removal_equals_restatement(pkg, gpu, batch):
    ctx, dev = gpu
    capi = pkg.capi
    po = batch["pt_off"]
    kept = dropped = 0
    for radius, min_nb, cell in ((0.05, 10, 0.05), (0.1, 10, 0.02), (0.1, 40, 0.3)):
        cloud, _t = _cloud(pkg, ctx, dev, batch, cell)
        keep, cnt = capi.filter_radius(ctx, cloud, radius, min_nb, want_counts=True)
        keep_fast, _ = capi.filter_radius(ctx, cloud, radius, min_nb)          # no counts wanted: a query may stop once it is kept
        ctx.sync()
        keep, cnt, keep_fast = keep.cpu().numpy().astype(bool), cnt.cpu().numpy(), keep_fast.cpu().numpy().astype(bool)
        cloud.close()
        for o, (xyz, _n) in enumerate(batch["objs"]):
            b, e = int(po[o]), int(po[o + 1])
            k_ref, c_ref = ref.ror(xyz, radius, min_nb)
            assert np.array_equal(cnt[b:e], c_ref), (radius, o)
            assert np.array_equal(keep[b:e], k_ref) and np.array_equal(keep_fast[b:e], k_ref)
        kept += int(keep.sum()); dropped += int((~keep).sum())
    assert kept > 0.05 * (kept + dropped) and dropped > 0.05 * (kept + dropped)   # both outcomes, in quantity


def test_passthrough_and_compaction(pkg, gpu, batch):
    ctx, dev = gpu
    capi = pkg.capi
    po, xyz, nrm, rgba = batch["pt_off"], batch["xyz"], batch["nrm"], batch["rgba"]
    t = [_dev(xyz[:, i], dev) for i in range(3)] + [_dev(nrm[:, i], dev) for i in range(3)]
    c = _dev(rgba, dev)
    i_hi = int(np.nonzero((xyz[:, 2] > 0.1) & (xyz[:, 2] < 0.5))[0][0])
    z_hi = float(xyz[i_hi, 2])                                      # a limit that IS a coordinate of the data: inclusive
    keep = capi.filter_passthrough_z(ctx, t[0], t[1], t[2], -0.25, z_hi)
    k = keep.cpu().numpy().astype(bool)
    want = ref.passthrough_z(xyz, -0.25, z_hi)
    assert np.array_equal(k, want) and k[i_hi] and 0 < k.sum() < len(k)
    # an all-dropped and an all-kept object (object 10 keeps its non-finite points: the compaction only follows the mask)
    k[po[1]:po[2]] = False
    k[po[10]:po[11]] = True
    for with_color in (True, False):
        out = capi.compact_points(ctx, po, _dev(k.astype(np.uint8), dev), *t, rgba=c if with_color else None)
        new_off = out[0]
        counts = np.array([k[po[o]:po[o + 1]].sum() for o in range(len(po) - 1)])
        assert np.array_equal(new_off, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32))
        assert new_off[2] == new_off[1] and new_off[11] - new_off[10] == po[11] - po[10]
        src = [xyz[:, 0], xyz[:, 1], xyz[:, 2], nrm[:, 0], nrm[:, 1], nrm[:, 2]]
        for a in range(6):                                          # survivors in their order, every array travelling with its point
            assert np.array_equal(out[1 + a].cpu().numpy().view(np.uint32), np.ascontiguousarray(src[a][k]).view(np.uint32))
        if with_color:
            assert np.array_equal(out[7].cpu().numpy(), rgba[k])
        else:
            assert out[7] is None
    none = capi.compact_points(ctx, po, _dev(np.zeros(len(k), np.uint8), dev), *t)
    assert not none[0].any() and none[1].numel() == 0


# ---- the C++ host, end to end ---------------------------------------------------------------------------------------------------
def _host_cfg(**params):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Keypoints"]["Parameters"]["LeafSize"] = 0.2
    j["Parameters"].update(params)
    return j


def _dirty(ds, indices, seed):
    """objects of a synthetic split with 3 % uniform outliers (cube +-1.2, random unit normals) shuffled in between their points"""
    rng = np.random.default_rng(seed)
    out = []
    for i in indices:
        o = ds.get(i)
        n_out = int(0.03 * len(o["xyz"]))
        p = np.concatenate([o["xyz"], rng.uniform(-1.2, 1.2, size=(n_out, 3))]).astype(np.float32)
        nr = rng.normal(size=(n_out, 3)); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
        nrm = np.concatenate([o["normals"], nr]).astype(np.float32)
        perm = rng.permutation(len(p))
        out.append((p[perm], nrm[perm], o["label"]))
    return out


def _cat(objs):
    po = np.zeros(len(objs) + 1, np.uint32); po[1:] = np.cumsum([len(o[0]) for o in objs])
    return po, np.concatenate([o[0] for o in objs]), np.concatenate([o[1] for o in objs])


FILTER_SETS = [dict(UseStatisticalOutlierRemoval=True),
               dict(UseRadiusOutlierRemoval=True, OutlierRemovalRadius=0.1, OutlierRemovalMinNeighbors=6),
               dict(UseStatisticalOutlierRemoval=True, OutlierRemovalMeanK=12, OutlierRemovalStddevMul=1.5, UseRadiusOutlierRemoval=True,
                    OutlierRemovalRadius=0.1, OutlierRemovalMinNeighbors=6, CutoffDistanceZAxis=0.6)]


def _ref_filter(objs, p):
    out = []
    for xyz, nrm, label in objs:
        idx = ref.prefilter(xyz, use_sor=p.get("UseStatisticalOutlierRemoval", False), mean_k=p.get("OutlierRemovalMeanK", 20),
                            stddev_mul=p.get("OutlierRemovalStddevMul", 2.0), use_ror=p.get("UseRadiusOutlierRemoval", False),
                            radius=p.get("OutlierRemovalRadius", 0.005), min_neighbors=p.get("OutlierRemovalMinNeighbors", 10),
                            cutoff_z=p.get("CutoffDistanceZAxis", 0.0))
        out.append((xyz[idx], nrm[idx], label))
    return out


def test_host_detect_with_filters_equals_detect_on_filtered_clouds(pkg, gpu, tmp_path):
    syn = pkg.synthetic
    train = syn.Dataset(3, 9, split=0, n_points=4096, leaf=0.2)
    test = syn.Dataset(3, 6, split=1, n_points=4096, leaf=0.2)
    m = hb.Model()
    m.config_from_json(json.dumps(_host_cfg()))
    for i in sorted(range(9), key=lambda i: (train.label(i), i)):
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i)
    m.train()
    path = str(tmp_path / "clean.ism")
    m.write(path)
    m.close()
    saved = json.load(open(path))
    dirty = _dirty(test, range(6), 21)
    plain = hb.Model()
    plain.read(path)
    for n_set, params in enumerate(FILTER_SETS):
        saved["ObjectConfig"]["Parameters"].update(_host_cfg(**params)["Parameters"])
        p_on = str(tmp_path / ("filters%d.ism" % n_set))
        json.dump(saved, open(p_on, "w"))
        on = hb.Model()
        on.read(p_on)
        got = on.detect_batch(*_cat(dirty), max_maxima=8)
        f_on = _last_features(on, 1)
        on.close()
        clean = _ref_filter(dirty, params)
        assert all(0 < len(c[0]) < len(d[0]) for c, d in zip(clean, dirty))
        want = plain.detect_batch(*_cat(clean), max_maxima=8)
        f_off = _last_features(plain, 1)
        assert np.array_equal(f_on["off"], f_off["off"]) and len(f_on["desc"]) > 0
        for key in ("desc", "lrf", "kp"):
            assert np.array_equal(f_on[key].view(np.uint32), f_off[key].view(np.uint32)), (n_set, key)
        assert np.array_equal(got["n"], want["n"]) and (got["n"] > 0).all()
        for o in range(6):
            k = int(got["n"][o])
            assert np.array_equal(got["cls"][o, :k], want["cls"][o, :k])
            assert np.allclose(got["weight"][o, :k], want["weight"][o, :k], rtol=1e-5, atol=1e-7)
            assert np.allclose(got["pos"][o, :k], want["pos"][o, :k], rtol=0, atol=1e-5)
    # a batch in which the filters empty one object: that object gets no maxima, the others are as without it
    saved["ObjectConfig"]["Parameters"].update(_host_cfg(**FILTER_SETS[2])["Parameters"])
    json.dump(saved, open(str(tmp_path / "empty.ism"), "w"))
    on = hb.Model()
    on.read(str(tmp_path / "empty.ism"))
    behind = (dirty[0][0] * np.float32([1, 1, -1]) - np.float32([0, 0, 2])).astype(np.float32)     # all z < 0: the cut-off drops every point
    got = on.detect_batch(*_cat([dirty[1], (behind, dirty[0][1], 0), dirty[2]]), max_maxima=8)
    ref2 = plain.detect_batch(*_cat(_ref_filter([dirty[1], dirty[2]], FILTER_SETS[2])), max_maxima=8)
    assert got["n"][1] == 0 and np.array_equal(got["n"][[0, 2]], ref2["n"])
    assert np.array_equal(got["cls"][0, :got["n"][0]], ref2["cls"][0, :ref2["n"][0]])
    on.close()
    plain.close()


def test_host_train_with_sor_equals_train_on_filtered_clouds(pkg, gpu):
    syn = pkg.synthetic
    train = syn.Dataset(3, 6, split=0, n_points=4096, leaf=0.2)
    order = sorted(range(6), key=lambda i: (train.label(i), i))
    dirty = _dirty(train, order, 33)
    clean = _ref_filter(dirty, FILTER_SETS[0])
    feats = []
    for objs, params in ((dirty, FILTER_SETS[0]), (clean, {})):
        m = hb.Model()
        m.config_from_json(json.dumps(_host_cfg(**params)))
        for i, (xyz, nrm, label) in zip(order, objs):
            m.add_training(xyz, nrm, label, i)
        m.train()
        feats.append(_last_features(m, 0))
        m.close()
    assert len(feats[0]["desc"]) > 0
    for key in ("desc", "lrf", "kp", "cls", "model"):
        assert np.array_equal(feats[0][key].view(np.uint32), feats[1][key].view(np.uint32)), key
