"""VoxelGridCulling on the MI355X: ismhip_principal_curvatures, ismhip_culling_scores and ismhip_culling_select against the restatement
tests/culling_ref.py. Counts and the colour score are exact; curvature, pc1, pc2 and kpq lie within the bounds derived in culling_ref.py;
the selection is the restatement's selection applied to the device's own scores, bit for bit; scores and the kept set do not depend on
the run, the cell size or the order of the points."""
import functools

import numpy as np
import pytest

import culling_ref as ref
import culling_scenes as scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
LEAF = 0.2
MAX_DIST = 0.05


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def batch(name):
    if name == "generic":
        objs = [scenes.scene(k) for k in range(len(scenes.SCENES))]
    elif name == "sizes":
        objs = scenes.sized([0, 1, 2, 3, 63, 64, 65, 257])
    elif name == "gap":
        objs = scenes.sized([700, 0, 2048], seed=51)
    elif name == "holes":
        objs = [scenes.with_holes(scenes.scene(1)), scenes.with_holes(scenes.scene(2), seed=32)]
    elif name == "non_unit":
        objs = [scenes.non_unit(scenes.scene(2)), scenes.non_unit(scenes.scene(1), seed=42)]
    else:
        raise KeyError(name)
    return scenes.concat(objs)


class Device:
    """a batch on the device: the cloud, its voxel keypoints at `leaf` and whatever scores are asked for (numpy copies)"""

    def __init__(self, pkg, gpu, arrays, leaf=LEAF, cell=None):
        self.capi, (self.ctx, self.dev) = pkg.capi, gpu
        self.off, xyz, nrm, rgba = arrays
        self.leaf = leaf
        self.t = [T(xyz[:, i], self.dev) for i in range(3)] + [T(nrm[:, i], self.dev) for i in range(3)]
        self.rgba = T(rgba.view(np.int32), self.dev)
        self.cloud = self.capi.Cloud(self.ctx, self.off, *self.t, leaf * 0.5 if cell is None else cell, rgba=self.rgba)
        self.ko, self.kx, self.ky, self.kz, self.kc = self.capi.voxel_keypoints(self.ctx, self.off, *self.t[:3], leaf, rgba=self.rgba)
        self.kp = np.stack([N(self.kx), N(self.ky), N(self.kz)], 1).reshape(-1, 3)
        self.kp_rgba = N(self.kc).view(np.uint32)

    def curvatures(self):
        pc1, pc2, cnt = self.capi.principal_curvatures(self.ctx, self.cloud, self.leaf)
        self.pc1, self.pc2 = pc1, pc2
        return N(pc1), N(pc2), N(cnt)

    def scores(self, geometry, color="colordistance"):
        pc = (self.pc1, self.pc2) if geometry == "kpq" else (None, None)
        self.geo, self.col, cnt = self.capi.culling_scores(self.ctx, self.cloud, self.ko, self.kx, self.ky, self.kz, self.kc, self.leaf, geometry, color,
                                                           MAX_DIST, *pc)
        return N(self.geo), N(self.col), N(cnt)

    def select(self, **kw):
        r = self.capi.culling_select(self.ctx, self.ko, self.geo, self.col, self.kx, self.ky, self.kz, self.kc, **kw)
        return {k: (v if isinstance(v, np.ndarray) or v is None else N(v)) for k, v in r.items()}

    def close(self):
        self.cloud.close()


def objects(off, *arrays):
    for o in range(len(off) - 1):
        yield o, [a[int(off[o]):int(off[o + 1])] for a in arrays]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_within(label, got, want64, bound):
    """NaN exactly where the restatement has it; elsewhere |got - want| <= bound; prints the measured maximum in units of the bound"""
    got = np.asarray(got, np.float64)
    nan = np.isnan(want64)
    assert np.array_equal(np.isnan(got), nan), label
    if (~nan).any():
        err = np.abs(got[~nan] - want64[~nan])
        with np.errstate(all="ignore"):
            rel = np.where(bound[~nan] > 0, err / bound[~nan], np.where(err == 0, 0.0, np.inf))
        print("%s: %d values, max error %.3e, max error / bound %.3e" % (label, (~nan).sum(), err.max(), rel.max()))
        assert (err <= bound[~nan]).all(), label


def check_scores(name, d, arrays, rgb2lab, pc1, pc2, pcn, g_curv, col, cnt, g_kpq, pcs=None):
    """the principal curvatures and both geometry scores and the colour score of the Device d (on its own voxel keypoints, at its leaf)
    against the restatement, object by object: counts and the colour score exact, pc1, pc2, curvature and kpq within their derived bounds.
    pcs: ref.principal_curvatures per object where the caller has them -> the number of keypoints compared"""
    off, xyz, nrm, rgba = arrays
    lab = ref.lab_table(rgb2lab, rgba)
    kp_lab = ref.lab_table(rgb2lab, d.kp_rgba) if len(d.kp_rgba) else np.zeros((0, 3), f32)
    n_kp = 0
    for o, (p, nr, lb) in objects(off, xyz, nrm, lab):
        kb, ke = int(d.ko[o]), int(d.ko[o + 1])
        b, e = int(off[o]), int(off[o + 1])
        pc = ref.principal_curvatures(p, nr, d.leaf) if pcs is None else pcs[o]
        assert np.array_equal(pcn[b:e], pc["count"]), (name, o)
        check_within("%s object %d pc1" % (name, o), pc1[b:e], pc["pc1_64"], ref.pc_bound(pc["pc1_64"], pc["pc1_64"], pc["floor"]))
        check_within("%s object %d pc2" % (name, o), pc2[b:e], pc["pc2_64"], ref.pc_bound(pc["pc1_64"], pc["pc2_64"], pc["floor"]))
        if ke == kb:
            continue
        n_kp += ke - kb
        a = ref.scores(p, d.kp[kb:ke], d.leaf, "curvature", "colordistance", MAX_DIST, lab=lb, kp_lab=kp_lab[kb:ke])
        assert np.array_equal(cnt[kb:ke], a["count"]), (name, o)
        assert same_bits(col[kb:ke], a["color"]), (name, o)              # integer counts: bit-exact, NaN for an empty ball included
        nan = np.isnan(a["geo"])
        check_within("%s object %d curvature" % (name, o), g_curv[kb:ke], np.where(nan, np.nan, a["geo64"]), a["bound"])
        # kpq from the restatement's own curvatures; the bound carries both sides' pc error through the expression
        k = ref.scores(p, d.kp[kb:ke], d.leaf, "kpq", pc=pc)
        check_within("%s object %d kpq" % (name, o), g_kpq[kb:ke], np.where(np.isnan(k["geo"]), np.nan, k["geo64"]), k["bound"])
    return n_kp


@pytest.mark.parametrize("name", ["generic", "sizes", "gap", "holes", "non_unit"])
def test_scores_against_restatement(pkg, gpu, ora, name):
    off, xyz, nrm, rgba = batch(name)
    d = Device(pkg, gpu, batch(name))
    pc1, pc2, pcn = d.curvatures()
    g_curv, col, cnt = d.scores("curvature")
    g_kpq, col2, cnt2 = d.scores("kpq")
    d.ctx.sync()
    assert same_bits(col, col2) and same_bits(cnt, cnt2)
    n_kp = check_scores(name, d, batch(name), ora.rgb2lab, pc1, pc2, pcn, g_curv, col, cnt, g_kpq)
    print("%s: %d keypoints in %d objects" % (name, n_kp, len(off) - 1))
    assert n_kp >= 20
    d.close()


def test_empty_ball_and_non_finite_keypoint(pkg, gpu):
    d = Device(pkg, gpu, scenes.concat([scenes.scene(2)]))
    d.curvatures()
    kp = np.array([[5.0, 5.0, 5.0], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0]], f32)
    d.ko = np.array([0, 3], np.uint32)
    d.kx, d.ky, d.kz = (T(kp[:, i], d.dev) for i in range(3))
    d.kc = T(np.array([0x00C83C28] * 3, np.uint32).view(np.int32), d.dev)
    for method in ("curvature", "kpq"):
        g, c, n = d.scores(method)
        assert not n.any() and np.isnan(g).all() and np.isnan(c).all(), method
    g, c, n = d.scores("none", "none")
    assert not g.any() and not c.any() and not n.any()                     # unused scores are 0
    d.close()


COMBOS = [dict(combine="RequireCombinedList"), dict(combine="RequireOne"), dict(combine="RequireBoth"),
          dict(combine="RequireCombinedList", geometry_type="threshold", geometry_threshold=0.02),
          dict(combine="RequireBoth", color_type="threshold", color_threshold=0.3, cutoff_ratio=0.25),
          dict(color_on=False, cutoff_ratio=0.7), dict(geometry_on=False, cutoff_ratio=0.1)]
REF_KW = dict(geometry_on="geo_on", color_on="color_on", geometry_type="geo_type", color_type="color_type", geometry_threshold="geo_threshold",
              color_threshold="color_threshold", cutoff_ratio="ratio", combine="combine")


def check_selection(d, geo, col, kw, label):
    """the restatement's selection on the device's own scores against the device's: mask, thresholds, combined scores, compacted output"""
    r = d.select(**kw)
    new_off = [0]
    keep_all = np.zeros(len(geo), bool)
    for o in range(len(d.ko) - 1):
        kb, ke = int(d.ko[o]), int(d.ko[o + 1])
        want = ref.select(geo[kb:ke], col[kb:ke], **{REF_KW[k]: v for k, v in kw.items()})
        assert np.array_equal(r["keep"][kb:ke].astype(bool), want["keep"]), (label, o)
        assert same_bits(r["thresholds"][o], want["thresholds"]) or (np.isnan(want["thresholds"]).any() and
                                                                     np.array_equal(r["thresholds"][o], want["thresholds"], equal_nan=True)), (label, o)
        assert np.array_equal(r["combined"][kb:ke], want["combined"], equal_nan=True), (label, o)
        keep_all[kb:ke] = want["keep"]
        new_off.append(new_off[-1] + int(want["keep"].sum()))
    assert np.array_equal(r["kp_offsets"], np.asarray(new_off, np.uint32)), label
    got = np.stack([r["kx"], r["ky"], r["kz"]], 1).reshape(-1, 3)
    assert same_bits(got, d.kp[keep_all]), label                           # order kept
    assert same_bits(r["krgba"].view(np.uint32), d.kp_rgba[keep_all]), label
    return int(keep_all.sum())


@pytest.mark.parametrize("name,method", [("generic", "kpq"), ("generic", "curvature"), ("sizes", "curvature"), ("gap", "kpq"), ("holes", "kpq")])
def test_selection_on_device_scores(pkg, gpu, name, method):
    d = Device(pkg, gpu, batch(name))
    d.curvatures()
    geo, col, _ = d.scores(method)
    for kw in COMBOS:
        kept = check_selection(d, geo, col, kw, "%s %s %s" % (name, method, kw))
        print("%s %s %s: kept %d of %d" % (name, method, kw, kept, len(geo)))
    d.close()


def test_object_with_more_keypoints_than_a_workgroup(pkg, gpu):
    s = scenes.make(3000, 61)
    d = Device(pkg, gpu, scenes.concat([s, scenes.scene(2)]), leaf=0.03, cell=0.05)
    n0 = int(d.ko[1])
    print("keypoints per object", np.diff(d.ko).tolist())
    assert n0 > 4 * 256 and n0 % 256                                       # several workgroup-sized chunks and a ragged tail
    d.curvatures()
    geo, col, _ = d.scores("kpq")
    for kw in (dict(combine="RequireCombinedList"), dict(combine="RequireOne", cutoff_ratio=0.9), dict(color_on=False, cutoff_ratio=0.01)):
        check_selection(d, geo, col, kw, "large %s" % kw)
    d.close()


@pytest.mark.parametrize("case", scenes.SELECT_CASES, ids=[c["name"] for c in scenes.SELECT_CASES])
def test_hand_made_lists_through_select(pkg, gpu, case):
    capi, (ctx, dev) = pkg.capi, gpu
    n = len(case["g"])
    kp = np.arange(3 * n, dtype=f32).reshape(3, n)
    col = (np.arange(n) + 7).astype(np.int32)
    kw = {k2: case["kw"][k1] for k2, k1 in REF_KW.items() if k1 in case["kw"]}
    # the list as object 1 of three: an empty object in front, a one-entry object behind
    g3, c3 = T(np.concatenate([case["g"], [0.5]]).astype(f32), dev), T(np.concatenate([case["c"], [0.5]]).astype(f32), dev)
    kp3 = np.concatenate([kp, [[100.0], [101.0], [102.0]]], 1).astype(f32)
    r = capi.culling_select(ctx, [0, 0, n, n + 1], g3, c3, T(kp3[0], dev), T(kp3[1], dev), T(kp3[2], dev), T(np.concatenate([col, [99]]).astype(np.int32), dev), **kw)
    keep = np.asarray(case["keep"], bool)
    tail = int(ref.select([0.5], [0.5], **case["kw"])["keep"][0])           # a single entry whose combined score is 0: below FLT_MIN
    assert N(r["keep"])[:n].astype(bool).tolist() == case["keep"] and N(r["keep"])[n] == tail
    thr = N(r["thresholds"])
    assert np.array_equal(thr[1], np.asarray(case["thr"], f32), equal_nan=True)
    assert r["kp_offsets"].tolist() == [0, 0, int(keep.sum()), int(keep.sum()) + tail]
    m = int(keep.sum())
    assert same_bits(N(r["kx"])[:m], kp[0][keep]) and same_bits(N(r["kz"])[:m], kp[2][keep]) and same_bits(N(r["krgba"])[:m], col[keep])
    want = ref.select(case["g"], case["c"], **case["kw"])
    assert np.array_equal(N(r["combined"])[:n], want["combined"], equal_nan=True)


def test_invariance_to_run_cell_size_and_point_order(pkg, gpu):
    off, xyz, nrm, rgba = batch("generic")
    e0 = int(off[1])
    rev = (np.array([0, e0], np.uint32), xyz[:e0][::-1].copy(), nrm[:e0][::-1].copy(), rgba[:e0][::-1].copy())
    runs = []
    for arrays, cell in ((batch("generic"), None), (batch("generic"), None), (batch("generic"), LEAF / 4), (batch("generic"), LEAF * 4), (rev, None)):
        d = Device(pkg, gpu, arrays, cell=cell)
        pc1, pc2, pcn = d.curvatures()
        out = dict(kp=d.kp, ko=d.ko, pc1=pc1, pc2=pc2, pcn=pcn)
        for method in ("curvature", "kpq"):
            g, c, n = d.scores(method)
            sel = d.select(combine="RequireCombinedList")
            out[method] = (g, c, n, sel["keep"], sel["thresholds"], sel["kx"], sel["kp_offsets"])
        runs.append(out)
        d.close()
    base = runs[0]
    for r in runs[1:4]:
        assert same_bits(r["kp"], base["kp"]) and same_bits(r["pc1"], base["pc1"]) and same_bits(r["pc2"], base["pc2"]) and same_bits(r["pcn"], base["pcn"])
        for method in ("curvature", "kpq"):
            for a, b in zip(r[method], base[method]):
                assert same_bits(a, b), method
    r = runs[4]                                                            # object 0 with its points in reverse order
    k0 = int(base["ko"][1])
    assert same_bits(r["kp"], base["kp"][:k0])
    assert same_bits(r["pc1"][::-1], base["pc1"][:e0]) and same_bits(r["pc2"][::-1], base["pc2"][:e0])
    for method in ("curvature", "kpq"):
        g, c, n, keep, thr, kx, ko = r[method]
        bg, bc, bn, bkeep, bthr, bkx, bko = base[method]
        assert same_bits(g, bg[:k0]) and same_bits(c, bc[:k0]) and same_bits(n, bn[:k0]) and same_bits(keep, bkeep[:k0]) and same_bits(thr[0], bthr[0])
        assert same_bits(kx, bkx[:int(bko[1])])


def test_abi_cases(pkg, gpu):
    capi, (ctx, dev) = pkg.capi, gpu
    d = Device(pkg, gpu, batch("generic"))
    d.curvatures()
    geo, col, _ = d.scores("kpq")
    kept = int(ref_total_kept(d, geo, col))
    kw = dict(combine="RequireCombinedList")
    with pytest.raises(capi.IsmHipError, match="capacity too small"):
        capi.culling_select(ctx, d.ko, d.geo, d.col, d.kx, d.ky, d.kz, d.kc, capacity=kept - 1, **kw)
    r = capi.culling_select(ctx, d.ko, d.geo, d.col, d.kx, d.ky, d.kz, d.kc, capacity=kept, **kw)
    assert int(r["kp_offsets"][-1]) == kept
    for bad in (dict(cutoff_ratio=1.0), dict(cutoff_ratio=-0.1), dict(cutoff_ratio=float("nan"))):
        with pytest.raises(capi.IsmHipError, match="bad argument"):
            capi.culling_select(ctx, d.ko, d.geo, d.col, d.kx, d.ky, d.kz, d.kc, **bad)
    with pytest.raises(capi.IsmHipError, match="alias"):
        lib = capi.lib()
        import ctypes as C
        out = np.zeros(len(d.ko), np.uint32)
        ctx.check(lib.ismhip_culling_select(ctx._h, C.c_int(len(d.ko) - 1), capi._p(d.ko), capi._p(d.geo), capi._p(d.col), 1, 1, 0, 0, C.c_float(0), C.c_float(0),
                                            C.c_float(0.5), 2, capi._p(d.kx), capi._p(d.ky), capi._p(d.kz), capi._p(d.kc), C.c_uint32(len(geo)), capi._p(d.kx),
                                            capi._p(d.ky), capi._p(d.kz), capi._p(d.kc), None, None, None, capi._p(out)), "ismhip_culling_select")
    with pytest.raises(capi.IsmHipError, match="offsets"):
        capi.culling_select(ctx, d.ko[::-1].copy(), d.geo, d.col, d.kx, d.ky, d.kz, d.kc)
    with pytest.raises(capi.IsmHipError, match="bad argument"):
        capi.principal_curvatures(ctx, d.cloud, 0.0)
    with pytest.raises(capi.IsmHipError, match="bad argument"):
        capi.culling_scores(ctx, d.cloud, d.ko, d.kx, d.ky, d.kz, d.kc, -1.0, "curvature", "none")
    with pytest.raises(capi.IsmHipError, match="kpq needs pc1"):
        capi.culling_scores(ctx, d.cloud, d.ko, d.kx, d.ky, d.kz, d.kc, LEAF, "kpq", "none")
    with pytest.raises(ValueError, match="FilterMethodGeometry"):
        capi.culling_scores(ctx, d.cloud, d.ko, d.kx, d.ky, d.kz, d.kc, LEAF, "gaussian", "none")
    d.close()
    # a cloud without colours under colordistance is refused
    off, xyz, nrm, _ = batch("generic")
    t = [T(xyz[:, i], dev) for i in range(3)] + [T(nrm[:, i], dev) for i in range(3)]
    plain = capi.Cloud(ctx, off, *t, 0.1)
    with pytest.raises(capi.IsmHipError, match="needs a cloud with colours"):
        capi.culling_scores(ctx, plain, d.ko, d.kx, d.ky, d.kz, d.kc, LEAF, "none", "colordistance")
    with pytest.raises(capi.IsmHipError, match="needs a cloud with colours"):
        capi.voxel_culling_keypoints(ctx, plain, LEAF, color="colordistance")
    plain.close()


def ref_total_kept(d, geo, col):
    return sum(int(ref.select(geo[int(d.ko[o]):int(d.ko[o + 1])], col[int(d.ko[o]):int(d.ko[o + 1])])["keep"].sum()) for o in range(len(d.ko) - 1))


def test_empty_cloud_and_timers(pkg, gpu):
    import torch
    capi, (ctx, dev) = pkg.capi, gpu
    z = torch.zeros((1,), dtype=torch.float32, device=dev)                 # an empty batch still hands over valid pointers
    empty = capi.Cloud(ctx, [0, 0, 0], z, z, z, z, z, z, 0.1)
    pc1, pc2, cnt = capi.principal_curvatures(ctx, empty, 0.1)
    assert len(pc1) == 0
    none = z[:0]
    geo, col, cnt = capi.culling_scores(ctx, empty, [0, 0, 0], none, none, none, None, 0.1, "kpq", "none", 0.01, pc1, pc2)
    r = capi.culling_select(ctx, [0, 0, 0], geo, col, none, none, none, None, color_on=False)
    assert r["kp_offsets"].tolist() == [0, 0, 0] and len(r["kx"]) == 0
    assert np.array_equal(N(r["thresholds"]), np.full((2, 3), ref.FLT_MIN, f32))   # objects without keypoints: empty ranges, nothing set
    empty.close()
    d = Device(pkg, gpu, batch("generic"))
    ctx.timers_enable(True); ctx.timers_reset()
    ko, kx, ky, kz, kc = capi.voxel_culling_keypoints(ctx, d.cloud, LEAF, geometry="kpq", color="colordistance", max_similar_color_distance=MAX_DIST)
    ctx.sync()
    for name in ("culling_pc", "culling_scores", "culling_select"):
        ms, launches = ctx.timer(name)
        assert launches == 1 and ms > 0.0, name
    ctx.timers_enable(False)
    # the convenience call is the three entries in a row
    d.curvatures()
    geo, col, _ = d.scores("kpq")
    r = d.select(combine="RequireCombinedList")
    assert np.array_equal(ko, r["kp_offsets"]) and same_bits(N(kx), r["kx"]) and same_bits(N(kc), r["krgba"])
    assert 0 < int(ko[-1]) < len(geo)
    # both methods "none", or training with the filter disabled: the plain voxel grid, bit for bit
    for kw in (dict(), dict(geometry="kpq", is_training=True)):
        ko2, kx2, ky2, kz2, kc2 = capi.voxel_culling_keypoints(ctx, d.cloud, LEAF, **kw)
        assert np.array_equal(ko2, d.ko) and same_bits(N(kx2), N(d.kx)) and same_bits(N(kz2), N(d.kz)) and same_bits(N(kc2), N(d.kc))
    d.close()
