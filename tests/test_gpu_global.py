"""Region (global) descriptors on the device (-m gpu): ismhip_global_short_shot / ismhip_global_shot352 through capi on the scenes of
global_scenes.py.

SHORT_SHOT_GLOBAL counts: the restatement global_ref.py takes the DEVICE's centroid, radius and frame as input (outputs of the same
call, held to the CPU oracle separately below) and returns an interval per bin: a point is undecided when a raw bin coordinate, the 1e-15
test, the ball test or the selection test lies within eps = 1e-9 (global_ref.EPS, the margin the local descriptor's scenes are held to)
of a decision. Required: lower <= counts <= upper per bin, the sum inside its interval, at most 1 % of a scene's points undecided, and
the float row bit-equal to float(c / sqrt(sum c^2)) taken in float64 from the device's own counts.
Centroid, radius, frame and the SHOT_GLOBAL rows: against the CPU oracle called with ONE keypoint at the device's centroid and both
radii equal to the device's radius, to the project's 1e-4 (frames 1e-5 as everywhere); whole-object centroid and radius bit-equal to
ismhip_cloud_centroids / ismhip_cloud_radii; n_sel exact."""
import numpy as np
import pytest

import frontend_scenes as fs
import global_ref as gr
import global_scenes as gs
from test_gpu_frontend import LRF_TOL, TOL, Batch, assert_close_nan

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in gs.all_cases()}
_runs = {}


def region_arrays(case):
    obj = [r[0] for r in case["regions"]]
    cen = [(0, 0, 0) if r[1] is None else r[1] for r in case["regions"]]
    rad = [-1.0 if r[2] is None else r[2] for r in case["regions"]]
    return np.asarray(obj, np.int32), np.asarray(cen, np.float32), np.asarray(rad, np.float32)


def run(pkg, gpu, name):
    """every entry on a case, once: -> dict(short=[per grid outputs as numpy], shot=..., again=..., cloud_centroid, cloud_radius)"""
    if name in _runs:
        return _runs[name]
    ctx, dev = gpu
    case = CASES[name]
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), np.float32)] * len(case["objs"]), case["cell"])
    try:
        obj, cen, rad = region_arrays(case)
        host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        out = dict(short=[], again=[])
        for bins, min_radius, log_radius in gs.GRIDS[name]:
            out["short"].append(host(pkg.capi.global_short_shot(ctx, b.cloud, dev, obj, cen, rad, bins, min_radius, log_radius, want_counts=True)))
            out["again"].append(host(pkg.capi.global_short_shot(ctx, b.cloud, dev, obj, cen, rad, bins, min_radius, log_radius, want_counts=True)))
        out["shot"] = host(pkg.capi.global_shot352(ctx, b.cloud, dev, obj, cen, rad))
        out["shot_again"] = host(pkg.capi.global_shot352(ctx, b.cloud, dev, obj, cen, rad))
        cc = pkg.capi.cloud_centroids(ctx, b.cloud, dev)
        out["cloud_centroid"] = cc.cpu().numpy()
        out["cloud_radius"] = pkg.capi.cloud_radii(ctx, b.cloud, cc).cpu().numpy()
        ctx.sync()
    finally:
        b.close()
    _runs[name] = out
    return out


def selected(case, region):
    """(points, normals) the region selects, by the restatement"""
    o, centre, radius = region
    p, n = gs.finite_points(case, o)
    if radius is None:
        return p, n
    d2, _ = gr._sqdist(p, centre)
    keep = d2 < gr.r2_of(radius)
    return p[keep], n[keep]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_centroid_and_radius(pkg, gpu, name, ora):
    """n_sel exact (a point exactly on the selection radius is out); the centroid to 1e-4 of the oracle's (and of the double mean); the
    radius bit-equal to the float maximum taken from the device's own centroid; whole objects bit-equal to the cloud's own entries;
    an empty selection: NaN centroid, radius 0, NaN frame and row"""
    case, out = CASES[name], run(pkg, gpu, name)
    for got in (out["short"][0], out["shot"]):
        for r, region in enumerate(case["regions"]):
            sel, _ = selected(case, region)
            assert int(got["n_sel"][r]) == len(sel), (name, r)
            if len(sel) == 0:
                assert np.isnan(got["centroid"][r]).all() and got["radius"][r] == 0
                assert np.isnan(got["lrf"][r]).all() and np.isnan(got["desc"][r]).all()
                continue
            c, _ = gr.centroid_radius(sel)
            oc = ora.centroids([0, len(sel)], sel[:, 0], sel[:, 1], sel[:, 2])[0]
            assert np.abs(got["centroid"][r] - oc).max() <= TOL and np.abs(got["centroid"][r] - c).max() <= TOL
            d2, _ = gr._sqdist(sel, got["centroid"][r])
            assert bits(got["radius"][r:r + 1])[0] == bits(np.float32([np.sqrt(d2.max())]))[0]
            if region[2] is None:
                o = region[0]
                assert np.array_equal(bits(got["centroid"][r]), bits(out["cloud_centroid"][o])), (name, r)
                if np.isinf(case["objs"][o][0]).any():
                    # ismhip_cloud_radii reads the caller's arrays: a NaN coordinate never compares greater there, an INFINITE one does
                    # (its radius is +inf); the region takes the finite points only, and is checked against the float maximum above
                    assert np.isinf(out["cloud_radius"][o])
                    continue
                assert bits(got["radius"][r:r + 1])[0] == bits(out["cloud_radius"][o:o + 1])[0], (name, r)
    if name == "mixed":
        assert int(out["shot"]["n_sel"][0]) == len(selected(case, case["regions"][0])[0])
        sel_b, _ = selected(case, case["regions"][0])
        assert not (sel_b == np.float32([-2.5, 0, 0])).all(1).any()             # the two points exactly on the radius are out
        assert (sel_b == np.float32([-3.0, 0.25, 0])).all(1).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_and_shot_rows_match_the_oracle(pkg, gpu, name, ora):
    """one keypoint at the device's centroid, both radii the device's radius, over the selected points: frame to 1e-5, SHOT-352 row to
    1e-4, NaN patterns exact (fewer than five neighbours); the tie scene's frame is decided by the five median neighbours of 20 000"""
    case, out = CASES[name], run(pkg, gpu, name)
    got = out["shot"]
    worst_f = worst_d = 0.0
    for r, region in enumerate(case["regions"]):
        sel, nrm = selected(case, region)
        if len(sel) == 0:
            continue
        c, R = got["centroid"][r], float(got["radius"][r])
        if not R > 0:
            assert np.isnan(got["lrf"][r]).all() and np.isnan(got["desc"][r]).all()
            continue
        args = ([0, len(sel)], sel[:, 0], sel[:, 1], sel[:, 2])
        kp = ([0, 1], c[0:1], c[1:2], c[2:3])
        frame = ora.shot_lrf(*args, *kp, R)
        assert_close_nan(got["lrf"][r:r + 1], frame, LRF_TOL)
        assert_close_nan(out["short"][0]["lrf"][r:r + 1], frame, LRF_TOL)
        desc, _ = ora.shot352(*args, nrm[:, 0], nrm[:, 1], nrm[:, 2], *kp, frame, R)
        assert_close_nan(got["desc"][r:r + 1], desc, TOL)
        if not np.isnan(frame).any():
            worst_f = max(worst_f, float(np.abs(got["lrf"][r] - frame[0]).max()))
        if not np.isnan(desc).any():
            worst_d = max(worst_d, float(np.abs(got["desc"][r] - desc[0]).max()))
    print(f"{name}: max |frame - oracle| {worst_f:.3g}, max |SHOT_GLOBAL - oracle| {worst_d:.3g}")
    if name == "sizes":
        nsel = got["n_sel"]
        assert np.isnan(got["lrf"][nsel < 5]).all() and np.isfinite(got["lrf"][nsel >= 63]).all()
    if name == "tie":
        p, _ = gs.finite_points(case, 0)
        d2, _ = gr._sqdist(p, got["centroid"][0])
        assert np.array_equal(got["centroid"][0], np.zeros(3, np.float32))
        assert fs.sign_sums(p[d2 < gr.r2_of(got["radius"][0])], got["lrf"][0]) == (0, 0)      # an exact tie on the device's own frame too


@pytest.mark.parametrize("name", sorted(CASES))
def test_short_shot_global_counts_lie_in_the_restatements_interval(pkg, gpu, name):
    case, out = CASES[name], run(pkg, gpu, name)
    n_scene = sum(len(gs.finite_points(case, o)[0]) for o in range(len(case["objs"])))
    for g, (bins, min_radius, log_radius) in enumerate(gs.GRIDS[name]):
        got = out["short"][g]
        D = bins[0] * bins[1] * bins[2]
        assert got["desc"].shape == (len(case["regions"]), D) and got["counts"].shape == (len(case["regions"]), D)
        undecided = 0
        for r, region in enumerate(case["regions"]):
            sel, _ = selected(case, region)
            counts = got["counts"][r].astype(np.int64)
            if len(sel) == 0 or np.isnan(got["lrf"][r]).any():
                assert counts.sum() == 0 and np.isnan(got["desc"][r]).all()
                continue
            o, centre, radius = region
            if radius is None:
                pts, sd2, sr2 = sel, None, None
            else:                                     # hand over both sides of the selection boundary: points within eps of it are undecided
                pts, _ = gs.finite_points(case, o)
                sd2, _ = gr._sqdist(pts, centre)
                sr2 = gr.r2_of(radius)
            want, lower, upper, und = gr.short_shot_global_counts(pts, got["centroid"][r], got["radius"][r], got["lrf"][r], bins, min_radius,
                                                                  log_radius, sel_d2=sd2, sel_r2=sr2)
            undecided += und
            print(f"{name} {bins} region {r}: {counts.sum()} counted, {und} undecided, {int((counts != want).sum())} bins off the face-value counts")
            assert (lower <= counts).all() and (counts <= upper).all(), (name, bins, r)
            assert lower.sum() <= counts.sum() <= lower.sum() + und
            row = gr.row_of_counts(counts)
            assert np.array_equal(bits(got["desc"][r]), bits(row)), (name, bins, r)
        assert undecided <= 0.01 * n_scene
    if name == "needle":
        c8 = out["short"][0]["counts"][0]
        # the needle crowds the bins round phi = 0 and +-180 (a handful of points beside the centroid fall elsewhere); one bin holds all
        assert c8[[0, 3, 4, 7]].sum() >= 0.99 * c8.sum() and out["short"][1]["counts"][0, 0] == c8.sum()
    if name == "shell":
        c = out["short"][0]["counts"][0]
        assert c[7] == c.sum() > 1900


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_calls_give_the_same_bits(pkg, gpu, name):
    out = run(pkg, gpu, name)
    pairs = list(zip(out["short"], out["again"])) + [(out["shot"], out["shot_again"])]
    for a, b in pairs:
        for k in a:
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (name, k)


def test_refusals(pkg, gpu):
    """bin counts outside 1 .. 256 and a logarithmic radius without a positive minimum are refused, as ismhip_short_shot refuses"""
    ctx, dev = gpu
    case = CASES["needle"]
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), np.float32)], case["cell"])
    try:
        for bins, code in (((0, 2, 8), "(-1)"), ((8, 8, 8), "(-4)"), ((2, -1, 8), "(-1)")):
            with pytest.raises(pkg.capi.IsmHipError, match=code.replace("(", r"\(").replace(")", r"\)")):
                pkg.capi.global_short_shot(ctx, b.cloud, dev, [0], bins=bins)
        with pytest.raises(pkg.capi.IsmHipError, match="logarithmic radius"):
            pkg.capi.global_short_shot(ctx, b.cloud, dev, [0], min_radius=0.0, log_radius=True)
        out = pkg.capi.global_short_shot(ctx, b.cloud, dev, [7, -1], bins=(2, 2, 8))          # objects that do not exist select nothing
        assert out["n_sel"].cpu().tolist() == [0, 0] and bool(out["desc"].isnan().all())
        assert pkg.capi.global_shot352(ctx, b.cloud, dev, [])["desc"].shape == (0, 352)
    finally:
        b.close()
