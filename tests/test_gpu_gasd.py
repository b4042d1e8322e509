"""The GASD region descriptor on the device (-m gpu): ismhip_global_gasd through capi on the scenes of gasd_scenes.py.

n_sel exact; centroid and radius bit-equal to ismhip_global_shot352's on the same regions. The frame: orthonormal, each axis an
eigenvector of the float64 covariance round the device's centroid to 4 * 2^-24 * lambda_max, its signs those of the float64 frame
wherever that decides. max_coord within two float ulps of the float64 maximum in the device's frame. Counts: the restatement gasd_ref.py
takes the DEVICE's centroid, frame and max_coord and returns an interval per bin (a deposit within MARGIN of a cell face is undecided):
lower <= counts <= upper per bin, each block's total inside its interval, at most 1 % of a scene's deposits undecided; the plane, which
lies on a z face by construction, is held on its z marginal. The float row is bit-equal to the products taken in float64 from the
device's own counts. The six-point scene and the coincident points match the float32 transcription bit for bit. NaN patterns exact, two
calls the same bits, the hue rule equal to its numpy float32 transcription on all 2^24 colours."""
import numpy as np
import pytest

import gasd_ref as ga
import gasd_scenes as gs
from test_gpu_frontend import Batch

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in gs.all_cases()}
_runs, _refs = {}, {}
U = 2.0 ** -24


def region_arrays(case):
    obj = [r[0] for r in case["regions"]]
    cen = [(0, 0, 0) if r[1] is None else r[1] for r in case["regions"]]
    rad = [-1.0 if r[2] is None else r[2] for r in case["regions"]]
    return np.asarray(obj, np.int32), np.asarray(cen, np.float32), np.asarray(rad, np.float32)


def run(pkg, gpu, name):
    """every call on a case, once -> dict(gasd, again, shape (without colour), nocounts, shot) of numpy outputs"""
    if name in _runs:
        return _runs[name]
    ctx, dev = gpu
    case = CASES[name]
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), np.float32)] * len(case["objs"]), case["cell"], rgba=case["rgba"])
    try:
        obj, cen, rad = region_arrays(case)
        host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        out = dict(gasd=host(pkg.capi.global_gasd(ctx, b.cloud, dev, obj, cen, rad, want_counts=True)),
                   again=host(pkg.capi.global_gasd(ctx, b.cloud, dev, obj, cen, rad, want_counts=True)),
                   shape=host(pkg.capi.global_gasd(ctx, b.cloud, dev, obj, cen, rad, with_color=False, want_counts=True)),
                   nocounts=host(pkg.capi.global_gasd(ctx, b.cloud, dev, obj, cen, rad)),
                   shot=host(pkg.capi.global_shot352(ctx, b.cloud, dev, obj, cen, rad)))
        ctx.sync()
    finally:
        b.close()
    _runs[name] = out
    return out


def reference(name, got):
    """per region (points, colours, the restatement's intervals from the device's own centroid, frame and max_coord), once per case"""
    if name not in _refs:
        case = CASES[name]
        refs = []
        for r, region in enumerate(case["regions"]):
            p, rgba = gs.selected(case, region)
            live = len(p) >= 2 and got["max_coord"][r] > 0 and np.isfinite(got["max_coord"][r])
            axes = (0, 1) if name == "plane" else (0, 1, 2)
            refs.append((p, rgba, ga.gasd_counts(p, rgba, got["centroid"][r], got["frame"][r], got["max_coord"][r], axes=axes) if live else None))
        _refs[name] = refs
    return _refs[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_centroid_and_radius(pkg, gpu, name):
    case, out = CASES[name], run(pkg, gpu, name)
    got, shot = out["gasd"], out["shot"]
    n = len(case["regions"])
    assert got["desc"].shape == (n, 984) and got["counts"].shape == (n, 984) and out["shape"]["desc"].shape == (n, 512)
    assert np.array_equal(got["n_sel"], shot["n_sel"])
    assert np.array_equal(bits(got["centroid"]), bits(shot["centroid"])) and np.array_equal(bits(got["radius"]), bits(shot["radius"]))
    for r, region in enumerate(case["regions"]):
        p, _ = gs.selected(case, region)
        assert int(got["n_sel"][r]) == len(p), (name, r)
        if len(p) == 0:
            assert np.isnan(got["centroid"][r]).all() and got["radius"][r] == 0
        if len(p) < 2:                                        # NaN frame, NaN max_coord, NaN row, zero counts
            assert np.isnan(got["frame"][r]).all() and np.isnan(got["max_coord"][r]) and np.isnan(got["desc"][r]).all()
            assert np.isnan(out["shape"]["desc"][r]).all() and (got["counts"][r] == 0).all()
    if name == "balls":
        assert got["n_sel"].tolist() == gs.BALL_SIZES
        nan_rows = np.isnan(got["desc"]).all(1)
        assert nan_rows.tolist() == [k < 2 for k in gs.BALL_SIZES] and not np.isnan(got["desc"][~nan_rows]).any()
        assert np.isnan(got["frame"]).all(1).tolist() == nan_rows.tolist() and np.isnan(got["max_coord"]).tolist() == nan_rows.tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_frame_and_max_coord(pkg, gpu, name):
    case, out = CASES[name], run(pkg, gpu, name)
    got = out["gasd"]
    worst_res = worst_mc = 0.0
    for r, region in enumerate(case["regions"]):
        p, _ = gs.selected(case, region)
        if len(p) < 2:
            continue
        F = got["frame"][r].reshape(3, 3).astype(np.float64)
        # orthonormal: three unit vectors each cast to float (sqrt(3) * 2^-24 off): a product of two is off by twice that and a second-order term
        assert np.abs(F @ F.T - np.eye(3)).max() <= 8 * U, (name, r)
        assert abs(np.linalg.det(F) - 1) <= 16 * U and F[2] @ [0.0, 0.0, 1.0] <= 0
        ref = ga.frame64(p, got["centroid"][r])
        lam = ref["w"][[2, 1, 0]]                              # x the largest, z the smallest
        lmax = max(float(ref["w"][2]), 0.0)
        for a in range(3):
            res = float(np.linalg.norm(ref["C"] @ F[a] - lam[a] * F[a]))
            worst_res = max(worst_res, res / lmax if lmax > 0 else 0.0)
            assert res <= 4 * U * lmax, (name, r, a, res, lmax)
        if not ref["degenerate"] and not ref["undecided"]:    # unique axes and a decided majority: the signs are the reference's,
            assert np.abs(F - ref["frame"]).max() <= 2 * U, (name, r, F, ref["frame"])      # the components one float cast away
        mc64 = ga.max_coord64(p, got["centroid"][r], got["frame"][r])
        err = abs(float(got["max_coord"][r]) - mc64)
        ulp = float(np.spacing(np.float32(mc64)))
        worst_mc = max(worst_mc, err / ulp if ulp > 0 else 0.0)
        assert err <= 2 * ulp, (name, r, got["max_coord"][r], mc64)
    print(f"{name}: worst |C a - lambda a| / lambda_max = {worst_res / U:.3f} * 2^-24 (bound 4), worst max_coord error {worst_mc:.3f} ulp (bound 2)")
    if name == "facing":                                       # mirrored in z: x and y mirrored, z mirrored AND negated
        a, b = got["frame"][0].reshape(3, 3), got["frame"][1].reshape(3, 3)
        m = np.float32([1, 1, -1])
        assert np.abs(b[0] - a[0] * m).max() < 1e-5 and np.abs(b[1] - a[1] * m).max() < 1e-5 and np.abs(b[2] + a[2] * m).max() < 1e-5
        assert a[2][2] < -0.9 and b[2][2] < -0.9
    if name == "ties":
        assert np.array_equal(got["frame"][0], np.float32([1, 0, 0, 0, -1, 0, 0, 0, -1])) and got["max_coord"][0] == 3.0
        assert np.array_equal(got["centroid"][0], np.zeros(3, np.float32))
    if name == "coincident":
        assert got["max_coord"][0] == 0.0 and np.isfinite(got["frame"][0]).all() and got["n_sel"][0] == 2
        assert np.array_equal(got["centroid"][0], gs.COINCIDENT) and got["radius"][0] == 0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_lie_in_the_restatements_interval_and_the_row_is_their_product(pkg, gpu, name):
    case, out = CASES[name], run(pkg, gpu, name)
    got = out["gasd"]
    deposits = undecided = 0
    for r, (p, rgba, ref) in enumerate(reference(name, got)):
        counts = got["counts"][r].astype(np.int64)
        if ref is None:
            assert counts.sum() == 0 and np.isnan(got["desc"][r]).all() and np.isnan(out["shape"]["desc"][r]).all(), (name, r)
            continue
        deposits += ref["deposits"]; undecided += ref["undecided"]
        held = ga.z_marginal(counts) if name == "plane" else counts
        off = int((held != ref["counts"]).sum())
        print(f"{name} region {r}: n {ref['n']}, {ref['undecided']} of {ref['deposits']} deposits undecided, {off} bins off the face-value counts")
        assert (ref["lower"] <= held).all() and (held <= ref["upper"]).all(), (name, r, np.nonzero((ref["lower"] > held) | (held > ref["upper"]))[0])
        totals = ga.block_totals(counts)
        for k in range(2):                                     # deposited = selected - dropped
            assert ref["total_lower"][k] <= totals[k] <= ref["total_upper"][k] <= ref["n"], (name, r, k)
        n_sel = int(got["n_sel"][r])
        assert np.array_equal(bits(got["desc"][r]), bits(ga.row_of_counts(counts, n_sel))), (name, r)
        short = out["shape"]
        assert np.array_equal(bits(short["desc"][r]), bits(ga.row_of_counts(short["counts"][r], n_sel, with_color=False))), (name, r)
        assert (short["desc"][r][216:] == 0).all() and (short["counts"][r][216:] == 0).all()
        assert np.array_equal(bits(short["desc"][r][:216]), bits(got["desc"][r][:216])) and np.array_equal(short["counts"][r][:216], counts[:216])
    if name != "ties":                                         # the six points sit on cell faces exactly: held bit for bit below
        assert undecided <= 0.01 * deposits
    for k in ("n_sel", "centroid", "radius", "frame", "max_coord"):
        assert np.array_equal(bits(got[k]), bits(out["shape"][k])), k
    assert np.array_equal(bits(got["desc"]), bits(out["nocounts"]["desc"]))


@pytest.mark.parametrize("name,r", [("ties", 0), ("coincident", 0)])
def test_the_exact_scenes_match_the_float32_transcription_bit_for_bit(pkg, gpu, name, r):
    case, out = CASES[name], run(pkg, gpu, name)
    got = out["gasd"]
    p, rgba = gs.selected(case, case["regions"][r])
    if name == "coincident":
        assert np.isnan(got["desc"][r]).all() and (got["counts"][r] == 0).all() and np.isnan(out["shape"]["desc"][r]).all()
        return
    shape, colour = ga.bins32(p, rgba, got["centroid"][r], got["frame"][r], got["max_coord"][r])
    want = np.bincount(np.concatenate([shape[shape >= 0], colour[colour >= 0]]), minlength=984)
    assert np.array_equal(got["counts"][r], want)
    assert sorted(np.nonzero(want)[0].tolist()) == sorted([21, 117, 141, 128, 130, 340, 632, 768, 709, 726])   # hand-derived: test_gasd_cpu.py
    assert np.array_equal(bits(got["desc"][r]), bits(ga.row_of_counts(want, 6)))
    assert np.array_equal(bits(out["shape"]["desc"][r]), bits(ga.row_of_counts(want, 6, with_color=False)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_calls_give_the_same_bits(pkg, gpu, name):
    out = run(pkg, gpu, name)
    for k in out["again"]:
        assert np.array_equal(np.ascontiguousarray(out["gasd"][k]).view(np.uint8), np.ascontiguousarray(out["again"][k]).view(np.uint8)), (name, k)


def test_the_hue_rule_on_every_colour(pkg, gpu):
    import torch
    ctx, dev = gpu
    got = pkg.capi.gasd_hue_bins(ctx, torch.arange(1 << 24, dtype=torch.int32, device=dev)).cpu().numpy()
    for a in range(0, 1 << 24, 1 << 22):
        want = ga.hue_bins32(np.arange(a, a + (1 << 22), dtype=np.uint32))
        assert np.array_equal(got[a:a + (1 << 22)], want), a
    assert got.max() == 11 and set(np.unique(got).tolist()) == set(range(12))
    high = pkg.capi.gasd_hue_bins(ctx, torch.tensor([0x7f00ff00, 0x0000ff00], dtype=torch.int32, device=dev)).cpu().tolist()
    assert high == [4, 4]                                      # bits 24..31 are ignored


def test_refusals(pkg, gpu):
    """a non-finite or zero view direction and with_color on a cloud without colours are refused; objects that do not exist select
    nothing; no region: nothing is written"""
    ctx, dev = gpu
    case = CASES["ramp"]
    plain = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), np.float32)], case["cell"])
    b = Batch(pkg, ctx, dev, case["objs"], [np.zeros((0, 3), np.float32)], case["cell"], rgba=case["rgba"])
    try:
        for vd in ((np.nan, 0, 1), (0, np.inf, 0), (0, 0, -np.inf), (0, 0, 0)):
            with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*view direction"):
                pkg.capi.global_gasd(ctx, b.cloud, dev, [0], view_direction=vd)
        with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*colour arrays missing"):
            pkg.capi.global_gasd(ctx, plain.cloud, dev, [0])
        short = pkg.capi.global_gasd(ctx, plain.cloud, dev, [0], with_color=False)
        full = pkg.capi.global_gasd(ctx, b.cloud, dev, [0])
        assert short["desc"].shape == (1, 512) and torch_equal_bits(short["desc"][:, :216], full["desc"][:, :216])
        flipped = pkg.capi.global_gasd(ctx, b.cloud, dev, [0], view_direction=(0, 0, -2.5))
        assert torch_equal_bits(-flipped["frame"][:, 6:], full["frame"][:, 6:]) and torch_equal_bits(flipped["frame"][:, :3], full["frame"][:, :3])
        out = pkg.capi.global_gasd(ctx, b.cloud, dev, [7, -1], want_counts=True)
        assert out["n_sel"].cpu().tolist() == [0, 0] and bool(out["desc"].isnan().all()) and bool(out["frame"].isnan().all())
        assert bool(out["max_coord"].isnan().all()) and int(out["counts"].sum()) == 0
        assert pkg.capi.global_gasd(ctx, b.cloud, dev, [])["desc"].shape == (0, 984)
    finally:
        b.close(); plain.close()


def torch_equal_bits(a, b):
    import torch
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
