"""GPU tests (-m gpu) of the vote-space maxima search (csrc/maxima.hip): the device against the CPU oracle on the scenes of
maxima_scenes.py, whose reach (tile seams, workspace path, table edges, capacities, iteration counts, rounding boundaries) is proved
without a GPU in test_maxima_cpu.py. Integers (n, cls, inst, n_votes, hence the order of the maxima) must be equal; floats keep the
project's bounds: weight, inst_weight, class_score 1e-4; mean-shift pos 2e-3; Hough pos 1e-4; bbox_size 1e-3; quaternions up to sign
2e-4 (5e-4 after the Merge filter). Every comparison prints its largest errors (pytest -s)."""
import numpy as np
import pytest

import hough_ref
import maxima_scenes as ms
from maxima_scenes import CB_KW, CHAIN_KW, ISO_KW, LAT_KW, TALLY_MS, assert_isolated, class_bin_scenes, isolated_closed_form, lattice_run

pytestmark = pytest.mark.gpu
TOL = 1e-4
MS_POS, HOUGH_POS = 2e-3, 1e-4


def dv(v, dev):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(a)).to(dev) for k, a in v.items()}


def host(out):
    return {k: a.cpu().numpy() for k, a in out.items()}


def compare(label, got, want, pos_tol, quat_tol=2e-4):
    got = host(got) if hasattr(got["n"], "cpu") else got
    for key in ("n", "cls", "inst", "n_votes"):
        assert np.array_equal(got[key], want[key]), (label, key)
    errs = {}
    for key, tol in (("weight", TOL), ("inst_weight", TOL), ("class_score", TOL), ("pos", pos_tol), ("bbox_size", 1e-3)):
        errs[key] = float(np.abs(got[key].astype(np.float64) - want[key]).max())
    if "bbox_quat" in want:
        a, b = got["bbox_quat"].astype(np.float64), want["bbox_quat"].astype(np.float64)
        errs["bbox_quat"] = float(np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1)).max())
    print("ERR", label, " ".join(f"{k}={e:.3e}" for k, e in errs.items()))
    for key, tol in (("weight", TOL), ("inst_weight", TOL), ("class_score", TOL), ("pos", pos_tol), ("bbox_size", 1e-3), ("bbox_quat", quat_tol)):
        if key in errs:
            assert errs[key] <= tol, (label, key, errs[key])            # NaN fails too
    return got


def same_bytes(label, a, b):
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), (label, key)


# ------------------------------------------------------------------------------------------------ Hough3D
@pytest.mark.parametrize("rel", [0.5, 1.0, 1.5])
@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interpolated"])
def test_lattice_matches_oracle(pkg, gpu, ora, interp, rel):
    """scene 1: the dyadic lattice on the 26 x 25 x 28 space: plateaus and steps across the tile seams of x, y and z, maxima in the
    first, the last and the partial bin, votes on a bin boundary, at min_coord and at max_coord, bins exactly at and one 64th below
    rel * max(H); rel > 1 counts as 1"""
    ctx, dev = gpu
    off, v, _ = ms.lattice()
    kw = dict(LAT_KW, use_interpolation=interp, rel_threshold=rel)
    compare(f"lattice-{interp}-{rel}", pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw), ora.hough3d_maxima(off, v, **kw), HOUGH_POS)
    ctx.sync()


@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interpolated"])
def test_lattice_at_the_three_tile_edges(pkg, gpu, ora, interp):
    """scene 2: the lattice alone (cap 128, tile edge 24), beside 1100 empty slots (cap 2048, edge 21) and beside 2049 (workspace
    path, edge 24): each run equals the oracle, and the lattice object's outputs are the same bytes in all three -- neither the
    table size, nor where the tiles are cut, nor where the votes are kept enters the arithmetic"""
    ctx, dev = gpu
    kw = dict(LAT_KW, use_interpolation=interp, rel_threshold=0.5)
    outs = {}
    for run in ("alone", "cap2048", "workspace"):
        off, v, _ = lattice_run(run)
        got = compare(f"lattice-{run}-{interp}", pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw), ora.hough3d_maxima(off, v, **kw), HOUGH_POS)
        assert got["n"][0] >= 38 and (run == "alone" or got["n"][1] == 0)
        outs[run] = ms.objects(got, slice(0, 1))
    ctx.sync()
    same_bytes("cap2048", outs["alone"], outs["cap2048"])
    same_bytes("workspace", outs["alone"], outs["workspace"])


@pytest.mark.parametrize("scene", ["lattice", "random"])
@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interpolated"])
def test_class_bins_match_oracle(pkg, gpu, ora, scene, interp):
    """scene 3: three classes with bins 0.125 / 0.25 / 0.5 in one non-cubic space (class_bin), exact lattice and random blobs"""
    ctx, dev = gpu
    off, v = class_bin_scenes()[scene]
    kw = dict(CB_KW, use_interpolation=interp)
    got = compare(f"class_bin-{scene}-{interp}", pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw), ora.hough3d_maxima(off, v, **kw), HOUGH_POS)
    assert set(got["cls"][got["cls"] >= 0].tolist()) == {0, 1, 2}
    ctx.sync()


def test_class_bins_with_merge_are_refused(pkg, gpu):
    ctx, dev = gpu
    off, v = ms.class_bin_lattice()
    with pytest.raises(pkg.capi.IsmHipError, match="Merge with per-class bin sizes not built"):
        pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **dict(CB_KW, max_filter=2))


@pytest.mark.parametrize("max_filter", [1, 2])
def test_hough_max_filters_match_oracle(pkg, gpu, ora, max_filter):
    """scene 4: Hough3D with MaxFilterType Simple on the colliding-classes scene and Merge (with AverageRotation) on the
    stacked-classes scene"""
    ctx, dev = gpu
    off, v = (ms.colliding_classes_scene if max_filter == 1 else ms.stacked_classes_scene)()
    kw = dict(n_classes=5, bin_size=0.5, rel_threshold=0.3, max_maxima=32, min_votes_threshold=2, max_filter=max_filter, average_rotation=max_filter == 2)
    compare(f"hough-filter-{max_filter}", pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw), ora.hough3d_maxima(off, v, **kw), HOUGH_POS, quat_tol=5e-4)
    ctx.sync()


def test_hough_truncation_is_reported_by_sync(pkg, gpu, ora):
    """scene 5: 128 maxima of one class are kept whole and equal the oracle; of 129 the kernel keeps 128 (which ones is up to the
    order of its atomics) and ismhip_sync reports a truncation once. ismhip_sync has ONE message for both capacities ("... 128 maxima per
    class or 1024 per object ..."), so the text does not tell which one was hit: n == 128 does"""
    ctx, dev = gpu
    kw = dict(n_classes=1, bin_size=0.25, rel_threshold=0.5, max_maxima=256)
    off, v = ms.isolated_bins(128)
    got = compare("hough-128", pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw), ora.hough3d_maxima(off, v, **kw), HOUGH_POS)
    ctx.sync()
    assert got["n"][0] == 128
    off, v = ms.isolated_bins(129)
    out = pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw)
    with pytest.raises(pkg.capi.IsmHipError, match="128 maxima per class"):
        ctx.sync()
    ctx.sync()
    assert int(out["n"][0]) == 128


# ------------------------------------------------------------------------------------------------ mean shift
@pytest.mark.parametrize("n_per_class,n_classes", [(7, 3), (128, 8), (128, 1)])
def test_isolated_votes_closed_form(pkg, gpu, n_per_class, n_classes):
    """scene 6: every vote its own maximum at its own position, one voter, weight 1 / N, classes ascending, slot order inside a
    class; 8 x 128 fills the per-object capacity (1024) and 128 the per-class capacity exactly: nothing is reported"""
    ctx, dev = gpu
    off, v = ms.isolated_votes(n_per_class, n_classes)
    out = host(pkg.capi.find_maxima(ctx, off, dv(v, dev), n_classes=n_classes, max_maxima=1100, **ISO_KW))
    ctx.sync()
    assert_isolated(out, isolated_closed_form(n_per_class, n_classes))


@pytest.mark.parametrize("n_per_class,n_classes,kept,message", [(120, 9, 1024, "1024 per object"), (129, 1, 128, "128 maxima per class")])
def test_mean_shift_caps_are_reported_by_sync(pkg, gpu, n_per_class, n_classes, kept, message):
    """scene 6, capacities: 9 x 120 maxima exceed 1024 per object (the first 1024 in class order are kept, normalised among
    themselves), 129 of one class exceed 128 per class; ismhip_sync reports a truncation once, with the same message for both (`message` is a
    part of it, not a discriminator): which capacity was hit shows in the closed form of what is kept"""
    ctx, dev = gpu
    off, v = ms.isolated_votes(n_per_class, n_classes)
    out = host(pkg.capi.find_maxima(ctx, off, dv(v, dev), n_classes=n_classes, max_maxima=1100, **ISO_KW))
    with pytest.raises(pkg.capi.IsmHipError, match=message):
        ctx.sync()
    ctx.sync()
    assert_isolated(out, isolated_closed_form(n_per_class, n_classes, limit=kept))


@pytest.mark.parametrize("max_iter,threshold", [(0, 0.0), (1, 0.0), (2, 0.0), (3, 0.0), (1000, 1e-1), (1000, 1e-3)])
def test_iteration_limits_match_oracle(pkg, gpu, ora, max_iter, threshold):
    """scene 7: three blobs whose maxima differ between consecutive max_iter (6, 3, 4, 3 of them): `diff > threshold && iter <=
    max_iter` has to stop where the oracle's does"""
    ctx, dev = gpu
    off, v = ms.three_blobs()
    kw = dict(n_classes=1, bandwidth=0.5, threshold=threshold, max_iter=max_iter, max_maxima=16)
    compare(f"blobs-{max_iter}-{threshold}", pkg.capi.find_maxima(ctx, off, dv(v, dev), **kw), ora.find_maxima(off, v, **kw), MS_POS)
    ctx.sync()


def test_chain_closed_form_counts_the_iterations(pkg, gpu):
    """scene 7, closed form: max_iter = m ends on the mean of the first min(m + 1, 4) votes of the chain"""
    ctx, dev = gpu
    off, v = ms.chain()
    tv = dv(v, dev)
    for m in range(6):
        out = host(pkg.capi.find_maxima(ctx, off, tv, max_iter=m, **CHAIN_KW))
        k = min(m, 3)
        assert out["n"][0] == 1 and out["n_votes"][0, 0] == min(k + 2, 4), m
        np.testing.assert_allclose(out["pos"][0, 0], ms.CHAIN[:k + 1].astype(np.float64).mean(0), atol=1e-6)
    ctx.sync()


def test_seed_cells_on_the_rounding_boundary(pkg, gpu, ora):
    """scene 8: x / cell exactly half-integral for both signs (floor(x + 0.5) seeds), SUPPRESS and the uniform kernel; a vote
    with two or three coordinates on the boundary is out of its own seed's reach: no maximum on either side"""
    ctx, dev = gpu
    kw = dict(n_classes=1, bandwidth=ms.SEED_H, kernel=1, suppression=1, max_maxima=32)
    off, v = ms.seed_boundary_rows()
    got = compare("seed-rows", pkg.capi.find_maxima(ctx, off, dv(v, dev), **kw), ora.find_maxima(off, v, **kw), MS_POS)
    assert got["n"][0] >= 6
    for nc in (2, 3):
        off, v = ms.seed_boundary_corner(nc)
        assert int(pkg.capi.find_maxima(ctx, off, dv(v, dev), **kw)["n"][0]) == 0 == ora.find_maxima(off, v, **kw)["n"][0]
    ctx.sync()


@pytest.mark.parametrize("voting", ["meanshift", "hough"])
@pytest.mark.parametrize("case", ms.TALLY_CASES)
def test_instance_tally(pkg, gpu, ora, case, voting):
    """scene 9: the instance hash table full (64 and 256 distinct ids in as many entries), probing 11 deep across the table's end,
    negative ids under the unsigned order, exactly equal sums, an instance of weight 0; one maximum holding every vote"""
    ctx, dev = gpu
    off, v = ms.tally(case)
    if voting == "meanshift":
        got = compare(f"tally-{case}-ms", pkg.capi.find_maxima(ctx, off, dv(v, dev), **TALLY_MS), ora.find_maxima(off, v, **TALLY_MS), MS_POS)
    else:
        kw = dict(n_classes=1, max_maxima=4, **ms.TALLY_HOUGH)
        got = compare(f"tally-{case}-hough", pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw), ora.hough3d_maxima(off, v, **kw), HOUGH_POS)
    ctx.sync()
    inst, _ = hough_ref.best_instance(v["inst"], v["weight"])
    assert got["n"][0] == 1 and got["n_votes"][0, 0] == len(v["weight"]) and got["inst"][0, 0] == inst and got["inst_weight"][0, 0] == 1.0


def test_zero_weight_members_keep_the_oracles_nan_pattern(pkg, gpu, ora):
    """a maximum whose members all weigh 0 divides by a zero weight sum in the reference: undefined, so no values are compared,
    only that the device has its NaNs exactly where the oracle has them (the box size) and the same integers"""
    ctx, dev = gpu
    off, v = ms.zero_weight_blob()
    got, want = host(pkg.capi.find_maxima(ctx, off, dv(v, dev), **TALLY_MS)), ora.find_maxima(off, v, **TALLY_MS)
    ctx.sync()
    for key in ("n", "cls", "inst", "n_votes"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("pos", "weight", "inst_weight", "bbox_size", "class_score"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    assert np.isnan(want["bbox_size"][0, 0]).all()


# ------------------------------------------------------------------------------------------------ both paths, many pairs
def _both_paths(pkg, gpu, ora, fn, name, kw, som):
    import torch
    ctx, dev = gpu
    (off, v), (off2, v2), cen, rad = ms.options_scene()
    n_obj = len(off) - 1
    extra = lambda k: dict(object_centroid=torch.as_tensor(cen[:k]).to(dev), object_radius=torch.as_tensor(rad[:k]).to(dev)) if som else {}
    lds = getattr(pkg.capi, fn)(ctx, off, dv(v, dev), **kw, **extra(n_obj))
    want = getattr(ora, fn)(off, v, **kw, **(dict(object_centroid=cen[:n_obj], object_radius=rad[:n_obj]) if som else {}))
    lds = compare(f"{fn}-{name}", lds, want, MS_POS if fn == "find_maxima" else HOUGH_POS, quat_tol=5e-4 if kw.get("max_filter") == 2 else 2e-4)
    work = host(getattr(pkg.capi, fn)(ctx, off2, dv(v2, dev), **kw, **extra(n_obj + 1)))
    ctx.sync()
    assert work["n"][n_obj] >= 1 or kw.get("suppression") == 2
    same_bytes(f"{fn}-{name}", lds, ms.objects(work, slice(0, n_obj)))
    return lds


@pytest.mark.parametrize("name", list(ms.MS_OPTIONS))
def test_mean_shift_options_on_both_paths(pkg, gpu, ora, name):
    """scene 10: every option set of the mean shift on the LDS path (held to the oracle) and, with an object of 2049 slots appended,
    on the workspace path, where the shared objects' outputs are the same bytes: the two instantiations do the same arithmetic on
    the same votes in the same order, only the home of the arrays differs"""
    got = _both_paths(pkg, gpu, ora, "find_maxima", name, dict(ms.MS_BASE, **ms.MS_OPTIONS[name]), name.startswith("som"))
    assert (got["n"].sum() == 0) == (name == "none")


@pytest.mark.parametrize("name", list(ms.HOUGH_OPTIONS))
def test_hough_options_on_both_paths(pkg, gpu, ora, name):
    """scene 10 for Hough3D: interpolation on and off, AverageRotation, both filters, per-class bins; LDS path against the oracle,
    workspace path byte-equal on the shared objects"""
    got = _both_paths(pkg, gpu, ora, "hough3d_maxima", name, dict(ms.HOUGH_BASE, **ms.HOUGH_OPTIONS[name]), False)
    assert got["n"].sum() >= 8


@pytest.mark.parametrize("voting", ["meanshift", "hough"])
def test_many_pairs_match_oracle(pkg, gpu, ora, voting):
    """scene 11: 1152 (object, class) pairs on the workspace path; the big object is the last one, so all of its 128 regions start
    at offsets from the second pass of k_work_offsets"""
    ctx, dev = gpu
    off, v = ms.many_pairs()
    if voting == "meanshift":
        kw = dict(n_classes=ms.MANY_CLASSES, bandwidth=0.5, max_maxima=160)
        got = compare("many-ms", pkg.capi.find_maxima(ctx, off, dv(v, dev), **kw), ora.find_maxima(off, v, **kw), MS_POS)
    else:
        kw = dict(n_classes=ms.MANY_CLASSES, bin_size=0.5, rel_threshold=0.5, max_maxima=160)
        got = compare("many-hough", pkg.capi.hough3d_maxima(ctx, off, dv(v, dev), **kw), ora.hough3d_maxima(off, v, **kw), HOUGH_POS)
    ctx.sync()
    assert got["n"][ms.MANY_BIG] == 128


@pytest.mark.parametrize("scene", ["lattice", "tally", "options"])
def test_two_calls_give_the_same_bytes(pkg, gpu, scene):
    """scene 12: the atomics of the accumulator, of the instance table and of the maxima list leave no trace in the outputs"""
    ctx, dev = gpu
    if scene == "lattice":
        off, v, _ = ms.lattice()
        call = lambda tv: pkg.capi.hough3d_maxima(ctx, off, tv, **dict(LAT_KW, use_interpolation=True, rel_threshold=0.5))
    elif scene == "tally":
        off, v = ms.tally("full256")
        call = lambda tv: pkg.capi.find_maxima(ctx, off, tv, **TALLY_MS)
    else:
        _, (off, v), _, _ = ms.options_scene()
        call = lambda tv: pkg.capi.find_maxima(ctx, off, tv, **dict(ms.MS_BASE, **ms.MS_OPTIONS["merge"]))
    tv = dv(v, dev)
    a = host(call(tv))
    b = host(call(tv))
    ctx.sync()
    assert a["n"].sum() >= 1
    same_bytes(scene, a, b)
