"""The CVFH region descriptor on the device (-m gpu): ismhip_global_cvfh through capi on the scenes of cvfh_scenes.py.

n_sel, centroid and radius bit-equal to ismhip_global_shot352's on the same regions. On the exact scenes the labels, the cluster count,
order and sizes equal the restatement's exactly; on the random scene every device cluster is a union of components of the DECIDED links
inside one component of the decided-plus-undecided links. Row centroid and normal within a bound derived below from the summation
arithmetic; the restatement's interval counts are then taken from the DEVICE's centroid and normal: lower <= count <= upper per bin,
block totals inside their intervals, at most 1 % of a scene's depositing points undecided. The float row is bit-equal to the device's own
counts divided by 47278.0f. Two calls, two grid cell sizes: the same bits. max_rows = 1: row 0 of the full call. More clusters than
max_rows: the count is reported unclipped and asking again returns every row. ismhip_global_vfh on the same regions still meets
vfh_ref.py as test_gpu_vfh.py holds it (its bits on the scenes of vfh_scenes.py are that file's to guard)."""
import numpy as np
import pytest

import cvfh_ref as cr
import cvfh_scenes as cs
import vfh_ref as vr
from test_gpu_frontend import Batch

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
CASES = {c["name"]: c for c in cs.all_cases()}
_runs = {}


def region_arrays(case):
    obj = [r[0] for r in case["regions"]]
    cen = [(0, 0, 0) if r[1] is None else r[1] for r in case["regions"]]
    rad = [-1.0 if r[2] is None else r[2] for r in case["regions"]]
    return np.asarray(obj, np.int32), np.asarray(cen, f32), np.asarray(rad, f32)


def run(pkg, gpu, name):
    """every call on a case, once -> dict of numpy outputs"""
    if name in _runs:
        return _runs[name]
    ctx, dev = gpu
    case = CASES[name]
    obj, cen, rad = region_arrays(case)
    stride = max(len(p) for p, _ in case["objs"])
    host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
    kw = dict(want_counts=True, **case["params"])
    out = {}
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), f32)] * len(case["objs"]), case["cell"])
    try:
        out["full"] = host(pkg.capi.global_cvfh(ctx, b.cloud, dev, obj, cen, rad, max_rows=case["max_rows"], label_stride=stride, **kw))
        out["again"] = host(pkg.capi.global_cvfh(ctx, b.cloud, dev, obj, cen, rad, max_rows=case["max_rows"], label_stride=stride, **kw))
        out["one"] = host(pkg.capi.global_cvfh(ctx, b.cloud, dev, obj, cen, rad, max_rows=1, **kw))
        most = int(out["full"]["n_clusters"].max())
        if most > case["max_rows"]:
            out["asked_again"] = host(pkg.capi.global_cvfh(ctx, b.cloud, dev, obj, cen, rad, max_rows=most, **kw))
        out["shot"] = host(pkg.capi.global_shot352(ctx, b.cloud, dev, obj, cen, rad))
        out["vfh"] = host(pkg.capi.global_vfh(ctx, b.cloud, dev, obj, cen, rad, want_counts=True))
        ctx.sync()
    finally:
        b.close()
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), f32)] * len(case["objs"]), case["cell"] * 1.7)
    try:
        out["other_cell"] = host(pkg.capi.global_cvfh(ctx, b.cloud, dev, obj, cen, rad, max_rows=case["max_rows"], label_stride=stride, **kw))
        ctx.sync()
    finally:
        b.close()
    _runs[name] = out
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_centroid_and_radius_are_shot352s(pkg, gpu, name):
    case, out = CASES[name], run(pkg, gpu, name)
    got, shot = out["full"], out["shot"]
    assert np.array_equal(got["n_sel"], shot["n_sel"])
    assert np.array_equal(bits(got["centroid"]), bits(shot["centroid"])) and np.array_equal(bits(got["radius"]), bits(shot["radius"]))
    for r, ref in enumerate(cs.reference(case)):
        assert int(got["n_sel"][r]) == len(ref["sel"]), (name, r)
        if len(ref["sel"]) == 0:
            assert np.isnan(got["centroid"][r]).all() and got["radius"][r] == 0 and got["n_clusters"][r] == 0
            assert np.isnan(got["desc"][r]).all() and (got["counts"][r] == 0).all() and (got["row_size"][r] == 0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_clusters_order_and_sizes(pkg, gpu, name):
    case, got = CASES[name], run(pkg, gpu, name)["full"]
    for r, ((o, _, _), ref) in enumerate(zip(case["regions"], cs.reference(case))):
        npts = len(case["objs"][o][0])
        lab = got["labels"][r]
        assert (lab[npts:] == cr.NONE).all()
        lab = lab[:npts]
        assert np.array_equal(lab == cr.NONE, ref["labels"] == cr.NONE), (name, r)
        sel = ref["sel"]
        if case["exact"]:
            assert np.array_equal(lab, ref["labels"]), (name, r, np.nonzero(lab != ref["labels"])[0][:10])
        else:
            # a device cluster is a union of decided components and lies inside one loose component
            for a, b in ((ref["labels"], lab), (lab, ref["labels_loose"])):
                fine, coarse = a[sel], b[sel]
                for f in np.unique(fine):
                    assert len(np.unique(coarse[fine == f])) == 1, (name, r, f)
            for v in np.unique(lab[sel]):                       # a label is its component's smallest original index
                assert np.nonzero(lab == v)[0].min() == v, (name, r, v)
        # kept clusters from the DEVICE's labels: ascending root, sizes; none kept: the fallback row
        roots, size = np.unique(lab[sel], return_counts=True) if len(sel) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        keep = size >= case["params"]["min_points"]
        want = list(zip(roots[keep].tolist(), size[keep].tolist())) or ([(cr.NONE, len(sel))] if len(sel) else [])
        assert int(got["n_clusters"][r]) == len(want), (name, r, want)
        k = min(len(want), case["max_rows"])
        assert got["row_size"][r][:k].tolist() == [s for _, s in want[:k]] and (got["row_size"][r][k:] == 0).all(), (name, r)
        if case["exact"]:
            assert [(c["root"], c["size"]) for c in ref["clusters"]] == want, (name, r)


def device_clusters(case, got, r):
    """the members of the device's kept clusters of region r from its labels, in row order"""
    o = case["regions"][r][0]
    ref = cs.reference(case)[r]
    lab = got["labels"][r][:len(case["objs"][o][0])]
    sel = ref["sel"]
    roots, size = np.unique(lab[sel], return_counts=True) if len(sel) else ([], [])
    kept = [np.nonzero(lab == v)[0] for v, s in zip(roots, size) if s >= case["params"]["min_points"]]
    return kept or ([sel] if len(sel) else [])


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_against_the_restatement(pkg, gpu, name):
    """Row centroid: a coordinate is rounded to a grid of 2^-48 of its bound (half a step each, so the mean moves by at most half a
    step: below 2^-40 for these scenes), then ONE cast to float: half an ulp. Bound: one ulp of the component + 2^-40.
    Row normal: components on a grid of 2^-46, the mean moves by at most 2^-47 per component, the normalisation divides by the mean's
    length (>= 0.1 in every scene, checked), then one cast: bound one ulp of 1.0 (1.2e-7) + 2^-40."""
    case, out = CASES[name], run(pkg, gpu, name)
    got = out["full"]
    deposits = undecided = 0
    for r, ((o, _, _), ref) in enumerate(zip(case["regions"], cs.reference(case))):
        P, N = case["objs"][o]
        sel = ref["sel"]
        pos_of = {int(i): k for k, i in enumerate(sel)}
        for k, members in enumerate(device_clusters(case, got, r)[:case["max_rows"]]):
            c64 = P[members].astype(f64).mean(0)
            nn = ref["normals"][[pos_of[int(i)] for i in members]]
            nn = nn[np.isfinite(nn).all(1)]
            c_dev, n_dev = got["row_centroid"][r, k], got["row_normal"][r, k]
            assert (np.abs(c_dev.astype(f64) - c64) <= np.spacing(np.abs(c64).astype(f32)).astype(f64) + 2.0 ** -40).all(), (name, r, k, c_dev, c64)
            if len(nn) == 0:
                assert np.isnan(n_dev).all() and np.isnan(got["desc"][r, k]).all()
                continue
            mean = nn.mean(0)
            assert np.linalg.norm(mean) >= 0.1
            n64 = mean / np.linalg.norm(mean)
            # re-estimated clustering normals are the device's own float32 casts of its eigenvectors: each within 2^-24 of the
            # restatement's per component (cvfh_ref.py's margin derivation), so is their mean
            slack = 2.0 ** -23 if ref["estimated"] else 0.0
            assert (np.abs(n_dev.astype(f64) - n64) <= float(np.spacing(f32(1.0))) + 2.0 ** -40 + slack / np.linalg.norm(mean)).all(), (name, r, k, n_dev, n64)
            want = cr.row_counts(P[sel], N[sel], c_dev, n_dev)
            counts = got["counts"][r, k].astype(np.int64)
            if want["m"] < 2:
                assert counts.sum() == 0 and np.isnan(got["desc"][r, k]).all()
                continue
            deposits += want["m"]; undecided += want["undecided"]
            print(f"{name} region {r} row {k}: m {want['m']}, {want['undecided']} undecided, {int((counts != want['counts']).sum())} bins off face value")
            assert (want["lower"] <= counts).all() and (counts <= want["upper"]).all(), (name, r, k, np.nonzero((want["lower"] > counts) | (counts > want["upper"]))[0])
            blocks = [counts[45 * j:45 * (j + 1)].sum() for j in range(4)] + [counts[180:].sum()]
            for j in range(5):
                assert want["total_lower"][j] <= blocks[j] <= want["total_upper"][j], (name, r, k, j)
            assert np.array_equal(bits(got["desc"][r, k]), bits(cr.row_of_counts(counts))), (name, r, k)
        n_rows = min(int(got["n_clusters"][r]), case["max_rows"])
        assert np.isnan(got["desc"][r, n_rows:]).all() and (got["counts"][r, n_rows:] == 0).all() and np.isnan(got["row_centroid"][r, n_rows:]).all()
    assert undecided <= 0.01 * deposits


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_calls_and_two_cell_sizes_give_the_same_bits(pkg, gpu, name):
    """n_sel, centroid and radius of a BALL region are k_global's fixed-order double sums over the cell-sorted span: they are held to
    'two calls', and to 'two cell sizes' only for whole-object regions; everything CVFH adds is held to both"""
    case, out = CASES[name], run(pkg, gpu, name)
    whole = np.array([r[2] is None for r in case["regions"]])
    for k in out["full"]:
        a, b, c = (np.ascontiguousarray(out[w][k]) for w in ("full", "again", "other_cell"))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, k)
        if k in ("centroid", "radius"):
            a, c = np.ascontiguousarray(a[whole]), np.ascontiguousarray(c[whole])
        assert np.array_equal(a.view(np.uint8), c.view(np.uint8)), (name, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_capacity_one_returns_row_zero_and_asking_again_returns_every_row(pkg, gpu, name):
    case, out = CASES[name], run(pkg, gpu, name)
    full, one = out["full"], out["one"]
    assert np.array_equal(full["n_clusters"], one["n_clusters"])
    for k in ("row_centroid", "row_normal", "row_size", "desc", "counts"):
        assert np.array_equal(np.ascontiguousarray(full[k][:, 0]).view(np.uint8), np.ascontiguousarray(one[k][:, 0]).view(np.uint8)), (name, k)
    if name == "many":
        assert full["n_clusters"].tolist() == [6, 5, 4] and "asked_again" in out
        more = out["asked_again"]
        assert more["desc"].shape == (3, 6, 308) and more["n_clusters"].tolist() == [6, 5, 4]
        for k in ("row_centroid", "row_normal", "row_size", "desc", "counts"):
            assert np.array_equal(np.ascontiguousarray(full[k]).view(np.uint8), np.ascontiguousarray(more[k][:, :4]).view(np.uint8)), k
        for r, n in enumerate([6, 5, 4]):
            assert np.isfinite(more["desc"][r, :n]).all() and np.isnan(more["desc"][r, n:]).all() and (more["row_size"][r, :n] == 30).all()
    else:
        assert "asked_again" not in out


@pytest.mark.parametrize("name", sorted(CASES))
def test_vfh_on_the_same_regions_still_meets_its_restatement(pkg, gpu, name):
    case, got = CASES[name], run(pkg, gpu, name)["vfh"]
    for r, ((o, _, _), ref) in enumerate(zip(case["regions"], cs.reference(case))):
        P, N = case["objs"][o]
        sel = ref["sel"]
        if len(sel) == 0:
            continue
        want = vr.vfh_counts(P[sel], N[sel], got["centroid"][r], got["normal_centroid"][r])
        counts = got["counts"][r].astype(np.int64)
        if want["m"] < 2:
            continue
        assert (want["lower"] <= counts).all() and (counts <= want["upper"]).all(), (name, r)
        assert np.array_equal(bits(got["desc"][r]), bits(vr.row_of_counts(counts, want["m"]))), (name, r)


def test_refusals(pkg, gpu):
    ctx, dev = gpu
    case = CASES["hand"]
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), f32)] * len(case["objs"]), case["cell"])
    try:
        for kw in (dict(viewpoint=(np.nan, 0, 0)), dict(cluster_tolerance=0.0), dict(min_points=0), dict(max_rows=0), dict(angle_threshold=0.0)):
            with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\)"):
                pkg.capi.global_cvfh(ctx, b.cloud, dev, [0], **kw)
        out = pkg.capi.global_cvfh(ctx, b.cloud, dev, [9, -1], want_counts=True)
        assert out["n_sel"].cpu().tolist() == [0, 0] and out["n_clusters"].cpu().tolist() == [0, 0] and bool(out["desc"].isnan().all())
        assert pkg.capi.global_cvfh(ctx, b.cloud, dev, [])["desc"].shape == (0, 4, 308)
    finally:
        b.close()
