"""The VFH region descriptor on the device (-m gpu): ismhip_global_vfh through capi on the scenes of vfh_scenes.py.

n_sel exact; centroid and radius bit-equal to ismhip_global_shot352's on the same regions; the normal centroid within one float ulp of
the float64 mean of the finite normals. Counts: the restatement vfh_ref.py takes the DEVICE's centroid and normal centroid and returns an
interval per bin (a deposit within MARGIN = 1e-4 raw bin units of a decision is undecided): lower <= counts <= upper per bin, each
block's total inside its interval, at most 1 % of a scene's depositing points undecided. The float row is bit-equal to the products
taken in float64 from the device's own counts and m. NaN patterns exact, two calls the same bits."""
import numpy as np
import pytest

import vfh_ref as vr
import vfh_scenes as vs
from test_gpu_frontend import Batch

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in vs.all_cases()}
OTHER_VIEWPOINT = (0.5, -2.0, 1.0)
_runs, _refs = {}, {}


def region_arrays(case):
    obj = [r[0] for r in case["regions"]]
    cen = [(0, 0, 0) if r[1] is None else r[1] for r in case["regions"]]
    rad = [-1.0 if r[2] is None else r[2] for r in case["regions"]]
    return np.asarray(obj, np.int32), np.asarray(cen, np.float32), np.asarray(rad, np.float32)


def run(pkg, gpu, name):
    """every call on a case, once -> dict(vfh, again, filled, moved (another viewpoint), shot) of numpy outputs"""
    if name in _runs:
        return _runs[name]
    ctx, dev = gpu
    case = CASES[name]
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), np.float32)] * len(case["objs"]), case["cell"])
    try:
        obj, cen, rad = region_arrays(case)
        host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        out = dict(vfh=host(pkg.capi.global_vfh(ctx, b.cloud, dev, obj, cen, rad, want_counts=True)),
                   again=host(pkg.capi.global_vfh(ctx, b.cloud, dev, obj, cen, rad, want_counts=True)),
                   filled=host(pkg.capi.global_vfh(ctx, b.cloud, dev, obj, cen, rad, fill_size_component=True, want_counts=True)),
                   moved=host(pkg.capi.global_vfh(ctx, b.cloud, dev, obj, cen, rad, viewpoint=OTHER_VIEWPOINT, want_counts=True)),
                   nocounts=host(pkg.capi.global_vfh(ctx, b.cloud, dev, obj, cen, rad)),
                   shot=host(pkg.capi.global_shot352(ctx, b.cloud, dev, obj, cen, rad)))
        ctx.sync()
    finally:
        b.close()
    _runs[name] = out
    return out


def reference(name, key, got, viewpoint):
    """the restatement's intervals per region from the device's own centroid and normal centroid, once per (case, call)"""
    if (name, key) not in _refs:
        case = CASES[name]
        refs = []
        for r, region in enumerate(case["regions"]):
            p, n = vs.selected(case, region)
            refs.append(vr.vfh_counts(p, n, got["centroid"][r], got["normal_centroid"][r], viewpoint) if len(p) else None)
        _refs[(name, key)] = refs
    return _refs[(name, key)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_centroid_radius_and_normal_centroid(pkg, gpu, name):
    case, out = CASES[name], run(pkg, gpu, name)
    got, shot = out["vfh"], out["shot"]
    assert got["desc"].shape == (len(case["regions"]), 308) and got["counts"].shape == (len(case["regions"]), 308)
    assert np.array_equal(got["n_sel"], shot["n_sel"])
    assert np.array_equal(bits(got["centroid"]), bits(shot["centroid"])) and np.array_equal(bits(got["radius"]), bits(shot["radius"]))
    for r, region in enumerate(case["regions"]):
        p, n = vs.selected(case, region)
        assert int(got["n_sel"][r]) == len(p), (name, r)
        if len(p) == 0:
            assert np.isnan(got["centroid"][r]).all() and got["radius"][r] == 0 and np.isnan(got["normal_centroid"][r]).all()
            assert np.isnan(got["desc"][r]).all() and (got["counts"][r] == 0).all()
            continue
        nf = n[np.isfinite(n).all(1)].astype(np.float64)
        if len(nf) == 0:
            assert np.isnan(got["normal_centroid"][r]).all()
            continue
        mean = nf.sum(0) / len(nf)
        ulp = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
        assert (np.abs(got["normal_centroid"][r].astype(np.float64) - mean) <= ulp).all(), (name, r, got["normal_centroid"][r], mean)
    if name == "balls":
        assert got["n_sel"].tolist() == vs.BALL_SIZES
    if name == "centred":
        assert np.array_equal(got["centroid"][0], np.zeros(3, np.float32))
    if name == "plane":
        assert np.array_equal(bits(got["normal_centroid"][0]), bits(case["objs"][0][1][0]))


@pytest.mark.parametrize("key,viewpoint", [("vfh", (0, 0, 0)), ("moved", OTHER_VIEWPOINT)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_lie_in_the_restatements_interval_and_the_row_is_their_product(pkg, gpu, name, key, viewpoint):
    case, out = CASES[name], run(pkg, gpu, name)
    got = out[key]
    refs = reference(name, key, got, viewpoint)
    deposits = undecided = 0
    for r, region in enumerate(case["regions"]):
        ref = refs[r]
        counts = got["counts"][r].astype(np.int64)
        if ref is None or ref["m"] < 2:
            assert counts.sum() == 0 and np.isnan(got["desc"][r]).all(), (name, r)
            continue
        deposits += ref["m"]
        undecided += ref["undecided"]
        off = int((counts != ref["counts"]).sum())
        print(f"{name} {key} region {r}: m {ref['m']}, {ref['undecided']} undecided, {off} bins off the face-value counts")
        assert (ref["lower"] <= counts).all() and (counts <= ref["upper"]).all(), (name, r, np.nonzero((ref["lower"] > counts) | (counts > ref["upper"]))[0])
        blocks = [counts[45 * k:45 * (k + 1)].sum() for k in range(4)] + [counts[180:].sum()]
        for k in range(5):
            assert ref["total_lower"][k] <= blocks[k] <= ref["total_upper"][k], (name, r, k)
        assert np.array_equal(bits(got["desc"][r]), bits(vr.row_of_counts(counts, ref["m"]))), (name, r)
        assert np.array_equal(bits(out["filled"]["desc"][r]), bits(vr.row_of_counts(out["filled"]["counts"][r], ref["m"], True)))
    assert undecided <= 0.01 * deposits
    if name == "plane" and key == "vfh":
        c = got["counts"][0]
        assert c[180 + 115] == 4000 and c[22] == 4000 and c[45 + 22] == 4000 and c[90 + 22] == 4000
    if name == "centred" and key == "vfh":
        c = got["counts"][0]
        m = len(case["objs"][0][0])
        assert c[180:].sum() == m and c[:45].sum() == m - 1 and c[135:180].sum() == m - 1        # the centre point: rejected, but seen
    if name == "balls":
        nan_rows = np.isnan(got["desc"]).all(1)
        assert nan_rows.tolist() == [k < 2 for k in vs.BALL_SIZES] and not np.isnan(got["desc"][~nan_rows]).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_flag_and_the_viewpoint_change_only_their_own_blocks(pkg, gpu, name):
    out = run(pkg, gpu, name)
    a, f, mv = out["vfh"], out["filled"], out["moved"]
    assert np.array_equal(a["counts"], f["counts"])
    keep = np.r_[0:135, 180:308]
    assert np.array_equal(bits(a["desc"][:, keep]), bits(f["desc"][:, keep]))
    live = ~np.isnan(a["desc"][:, 0])
    assert (a["desc"][live][:, 135:180] == 0).all()
    if live.any():
        assert (f["desc"][live][:, 135:180].sum(1) > 0).all()
    assert np.array_equal(bits(a["desc"][:, :180]), bits(mv["desc"][:, :180])) and np.array_equal(a["counts"][:, :180], mv["counts"][:, :180])
    assert np.array_equal(bits(a["desc"]), bits(out["nocounts"]["desc"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_calls_give_the_same_bits(pkg, gpu, name):
    out = run(pkg, gpu, name)
    for k in out["vfh"]:
        assert np.array_equal(np.ascontiguousarray(out["vfh"][k]).view(np.uint8), np.ascontiguousarray(out["again"][k]).view(np.uint8)), (name, k)


def test_refusals(pkg, gpu):
    """a non-finite viewpoint is refused; objects that do not exist select nothing; no region: nothing is written"""
    ctx, dev = gpu
    case = CASES["plane"]
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), np.float32)], case["cell"])
    try:
        for vp in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
            with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*viewpoint"):
                pkg.capi.global_vfh(ctx, b.cloud, dev, [0], viewpoint=vp)
        out = pkg.capi.global_vfh(ctx, b.cloud, dev, [7, -1], want_counts=True)
        assert out["n_sel"].cpu().tolist() == [0, 0] and bool(out["desc"].isnan().all()) and bool(out["normal_centroid"].isnan().all())
        assert int(out["counts"].sum()) == 0
        assert pkg.capi.global_vfh(ctx, b.cloud, dev, [])["desc"].shape == (0, 308)
    finally:
        b.close()
