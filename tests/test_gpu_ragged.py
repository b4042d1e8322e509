"""GPU tests (-m gpu) of the ragged-array steps the stages share: the chunked block scan at its chunk edges and in its carry, the
stable compaction built on it, and the offsets check of the entry points. Everything here is exact integer work (or float data
moved unchanged), so every comparison is for equality; the expectations come from numpy (boolean indexing, cumsum), from the
construction of the scene, or from the CPU oracle -- never from the device.

Covered elsewhere: the in-place scan of the five-kernel grid build (test_gpu_grid_fused.py compares that build byte for byte with
the fused one; test_frontend_cpu.py proves that its scenes hold objects on both sides of the 1024-cell chunk)."""
import numpy as np
import pytest

import maxima_scenes as ms

pytestmark = pytest.mark.gpu

CHUNK = 256                                              # rows per pass of the per-object scan (k_scan_obj, k_vox_emit)
SIZES = [0, 1, 255, 256, 257, 512, 513, 769]             # rows per object: around one, two and three chunks
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
N = int(OFF[-1])
LOCAL = np.concatenate([np.arange(s) for s in SIZES])    # object-local row index
PATTERNS = ["all", "none", "last_of_chunk", "first_of_chunk", "random"]


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def keep_mask(pattern):
    if pattern == "all":
        return np.ones(N, bool)
    if pattern == "none":
        return np.zeros(N, bool)
    if pattern == "last_of_chunk":
        return LOCAL % CHUNK == CHUNK - 1
    if pattern == "first_of_chunk":
        return LOCAL % CHUNK == 0
    return np.random.default_rng(5).random(N) < 0.5


def kept_offsets(keep):
    return np.concatenate([[0], np.cumsum(keep)])[OFF].tolist()


# ------------------------------------------------------------------------------------------------ compaction
@pytest.fixture(scope="module")
def rows():
    """2563 feature rows (dim 33, LRF, keypoint) and as many points (xyz, normal, rgba): read-only"""
    rng = np.random.default_rng(3)
    return dict(desc=rng.random((N, 33)).astype(np.float32), lrf=rng.random((N, 9)).astype(np.float32), kp=rng.random((N, 3)).astype(np.float32),
                pts=rng.random((N, 6)).astype(np.float32), rgba=rng.integers(0, 1 << 24, N).astype(np.int32))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_feature_compaction_at_the_chunk_edges(pkg, gpu, rows, pattern):
    """compact_features and compact_descriptor_rows: a dropped row is NaN as a whole (even rows) or has a NaN first LRF component
    (odd rows), which both entry points flag"""
    ctx, dev = gpu
    keep = keep_mask(pattern)
    desc, lrf, kp = rows["desc"].copy(), rows["lrf"].copy(), rows["kp"]
    drop = np.nonzero(~keep)[0]
    desc[drop[drop % 2 == 0]] = np.nan
    lrf[drop[drop % 2 == 1], 0] = np.nan
    for fn in (pkg.capi.compact_features, pkg.capi.compact_descriptor_rows):
        a = (T(desc, dev), T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev))
        off, d, l, x, y, z, src = fn(ctx, OFF, *a)
        assert off.tolist() == kept_offsets(keep), fn.__name__
        assert np.array_equal(src.cpu().numpy(), np.nonzero(keep)[0]), fn.__name__
        for got, want in ((d, desc), (l, lrf), (x, kp[:, 0]), (y, kp[:, 1]), (z, kp[:, 2])):
            assert got.cpu().numpy().tobytes() == want[keep].tobytes(), fn.__name__
        if pattern == "all" and fn is pkg.capi.compact_descriptor_rows:      # nothing dropped: the inputs come back, uncopied
            assert [t.data_ptr() for t in (d, l, x, y, z)] == [t.data_ptr() for t in a]


@pytest.mark.parametrize("with_rgba", [True, False], ids=["rgba", "plain"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_point_compaction_at_the_chunk_edges(pkg, gpu, rows, pattern, with_rgba):
    """filter_normals (a dropped point has a NaN in one component of its normal) and compact_points (the keep mask itself)"""
    ctx, dev = gpu
    keep = keep_mask(pattern)
    pts, rgba = rows["pts"], rows["rgba"]
    nan_normals = pts.copy()
    drop = np.nonzero(~keep)[0]
    nan_normals[drop, 3 + drop % 3] = np.nan
    cols = lambda a: [T(a[:, j], dev) for j in range(6)]
    kw = dict(rgba=T(rgba, dev)) if with_rgba else {}
    for name, got, src in (("filter_normals", pkg.capi.filter_normals(ctx, OFF, *cols(nan_normals), **kw), nan_normals),
                           ("compact_points", pkg.capi.compact_points(ctx, OFF, T(keep.astype(np.uint8), dev), *cols(pts), **kw), pts)):
        assert got[0].tolist() == kept_offsets(keep), name
        for j in range(6):
            assert got[1 + j].cpu().numpy().tobytes() == src[keep, j].tobytes(), (name, j)
        if with_rgba:
            assert np.array_equal(got[7].cpu().numpy(), rgba[keep]), name
        else:
            assert got[7] is None


# ------------------------------------------------------------------------------------------------ voxel emit
LEAF = 0.25
VOXEL_TABLES = [        # occupied entries of each object's voxel table (the table ends at the last one), first entry of the table
    ([0], 0),
    ([0, 7, 100, 255], -3),
    ([0, 1, 128, 255, 256], 40),
    ([0, 255, 256, 300, 511, 512, 767, 768, 1000, 1024], -600),
]


@pytest.mark.parametrize("color", [True, False], ids=["rgba", "plain"])
def test_voxel_emit_at_the_chunk_edges(pkg, gpu, color):
    """objects on a dyadic lattice along x, one point per occupied voxel, tables of 1, 256, 257 and 1025 entries with the first and
    the last entry, 255, 256, 511, 512 and 1024 occupied and empty entries between: the centroid of a voxel is its point bit for bit
    (and its colour that point's), so the keypoints are the points in ascending voxel index, whatever order they arrive in"""
    ctx, dev = gpu
    rng = np.random.default_rng(9)
    xs, want_x, cols, want_c = [], [], [], []
    for occupied, first in VOXEL_TABLES:
        x = ((np.asarray(occupied) + first + 0.5) * LEAF).astype(np.float32)
        c = rng.integers(0, 1 << 24, len(x)).astype(np.int32)
        p = rng.permutation(len(x))
        want_x.append(x); want_c.append(c); xs.append(x[p]); cols.append(c[p])
    assert [o[-1] + 1 for o, _ in VOXEL_TABLES] == [1, 256, 257, 1025]
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint32)
    x = np.concatenate(xs)
    y, z = np.full_like(x, 0.5 * LEAF), np.full_like(x, -1.5 * LEAF)
    ko, kx, ky, kz, kc = pkg.capi.voxel_keypoints(ctx, off, T(x, dev), T(y, dev), T(z, dev), LEAF, rgba=T(np.concatenate(cols), dev) if color else None)
    assert ko.tolist() == off.tolist()
    assert kx.cpu().numpy().tobytes() == np.concatenate(want_x).tobytes()
    assert ky.cpu().numpy().tobytes() == y.tobytes() and kz.cpu().numpy().tobytes() == z.tobytes()
    if color:
        assert np.array_equal(kc.cpu().numpy(), np.concatenate(want_c))
    else:
        assert kc is None


# ------------------------------------------------------------------------------------------------ training CSR
DUPLICATES = [(3, 700), (4, 1021), (5, 1026), (1022, 1030), (1027, 1500), (1100, 2040)]      # row b is a copy of row a < b


@pytest.mark.parametrize("clean_up", [True, False], ids=["clean_up", "keep_all"])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_train_csr_at_the_chunk_edges(pkg, gpu, ora, n, clean_up):
    """train_activate with the features as their own codewords and k = 1: every row activates itself, a copy activates the lower
    row, so a copied word has two votes and its copy none -- with clean_up both go, on either side of word 1024 once n allows it"""
    ctx, dev = gpu
    rng = np.random.default_rng(n)
    feats = rng.random((n, 33)).astype(np.float32)
    dup = [(a, b) for a, b in DUPLICATES if b < n]
    for a, b in dup:
        feats[b] = feats[a]
    cls = np.sort(rng.integers(0, 4, n)).astype(np.uint32)
    model = (cls * 10 + rng.integers(0, 3, n)).astype(np.uint32)
    model = np.concatenate([np.sort(model[cls == c]) for c in range(4)])
    A = rng.normal(size=(n, 3, 3)); Q, _ = np.linalg.qr(A); Q[np.linalg.det(Q) < 0, 2] *= -1
    lrf = Q.reshape(n, 9).astype(np.float32); kp = rng.normal(size=(n, 3)).astype(np.float32)
    centre = rng.normal(size=(40, 3)).astype(np.float32)[model]
    got = pkg.capi.train_activate(ctx, 0, T(feats, dev), T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), cls, model, centre,
                                  k=1, clean_up=clean_up, n_classes=4)
    want = ora.activate(0, feats, lrf, kp, cls, model, centre, k=1, clean_up=clean_up, n_classes=4)
    for key in ("word_src", "vote_offsets", "vote_feature"):
        assert np.array_equal(got[key], want[key]), key
    np.testing.assert_allclose(got["vote_xyz"], want["vote_xyz"], atol=2e-6)
    np.testing.assert_allclose(got["vote_weight"], want["vote_weight"], atol=2e-6)
    np.testing.assert_allclose(got["vote_class_weight"], want["vote_class_weight"], rtol=1e-6, atol=1e-12)
    assert np.array_equal(got["class_sigma"], want["class_sigma"])
    gone = {a for a, _ in dup} | {b for _, b in dup}
    kept = sorted(set(range(n)) - (gone if clean_up else {b for _, b in dup}))
    assert want["word_src"].tolist() == kept                                   # the scene does what it was built for
    if n > 1025:
        assert clean_up is False or (min(gone) < 1024 < max(gone))


# ------------------------------------------------------------------------------------------------ big-object workspace
def test_workspace_offsets_at_the_chunk_edge(pkg, gpu, ora):
    """find_maxima on 5 objects x 205 classes = 1025 (object, class) pairs with a 2100-slot object: the workspace regions are laid
    out by k_work_offsets 1024 pairs at a time, and the last pair's region starts at the carry of all the others
    (test_maxima_cpu.py proves it of the scene). Compared with the oracle as test_gpu_maxima.py compares its capacity scenes."""
    from test_gpu_maxima import MS_POS, compare, dv
    ctx, dev = gpu
    off, v = ms.chunk_edge_pairs()
    kw = dict(n_classes=ms.EDGE_CLASSES, bandwidth=0.5, max_maxima=256)
    got = compare("chunk-edge", pkg.capi.find_maxima(ctx, off, dv(v, dev), **kw), ora.find_maxima(off, v, **kw), MS_POS)
    ctx.sync()
    assert got["n"][0] == ms.EDGE_CLASSES and {ms.EDGE_CLASSES - 2, ms.EDGE_CLASSES - 1} <= set(got["cls"][4, :got["n"][4]].tolist())


# ------------------------------------------------------------------------------------------------ offsets checks
def test_offsets_are_checked_by_every_entry_point(pkg, gpu):
    """a non-monotone offsets array raises "offsets not monotone" from every entry point that takes one; shot_lrf and
    voxel_keypoints also insist on offsets that start at 0"""
    import torch
    ctx, dev = gpu
    capi = pkg.capi
    rng = np.random.default_rng(1)
    p = [T(rng.random(16).astype(np.float32), dev) for _ in range(6)]
    rgba = torch.zeros(16, dtype=torch.int32, device=dev)
    cloud = capi.Cloud(ctx, [0, 8, 16], *p, 0.2, rgba=rgba)
    bad = np.array([0, 8, 4], np.uint32)
    k = [t[:8] for t in p[:3]]
    lrf = torch.zeros((8, 9), dtype=torch.float32, device=dev)
    off, votes = ms.isolated_votes(7, 3)
    votes = {key: T(a, dev) for key, a in votes.items()}
    calls = dict(
        shot_lrf=lambda: capi.shot_lrf(ctx, cloud, bad, *k, 0.3),
        shot352=lambda: capi.shot352(ctx, cloud, bad, *k, lrf, 0.3),
        cshot1344=lambda: capi.cshot1344(ctx, cloud, bad, *k, rgba[:8], lrf, 0.3),
        fpfh33=lambda: capi.fpfh33(ctx, cloud, bad, *k, 0.3),
        compact_features=lambda: capi.compact_features(ctx, bad, torch.zeros((8, 33), device=dev), lrf, *k),
        compact_descriptor_rows=lambda: capi.compact_descriptor_rows(ctx, bad, torch.zeros((8, 33), device=dev), lrf, *k),
        filter_normals=lambda: capi.filter_normals(ctx, bad, *p),
        compact_points=lambda: capi.compact_points(ctx, bad, torch.ones(16, dtype=torch.uint8, device=dev), *p),
        voxel_keypoints=lambda: capi.voxel_keypoints(ctx, bad, *p[:3], 0.5),
        find_maxima=lambda: capi.find_maxima(ctx, bad, votes, n_classes=3, bandwidth=0.5),
        hough3d_maxima=lambda: capi.hough3d_maxima(ctx, bad, votes, n_classes=3, bin_size=0.5),
        ransac_filter=lambda: capi.ransac_filter(ctx, bad, torch.zeros((8, 3), device=dev), torch.zeros((8, 3), device=dev), 0.1),
        ransac_hypothesis=lambda: capi.ransac_hypothesis(ctx, bad, torch.zeros((8, 3), device=dev), torch.zeros((8, 3), device=dev), 0.1, 0),
    )
    for name, call in calls.items():
        who = "compact_features" if name == "compact_descriptor_rows" else name      # the two share their driver and its messages
        with pytest.raises(capi.IsmHipError, match=f"{who}: offsets not monotone"):
            call()
    with pytest.raises(capi.IsmHipError, match="shot_lrf: offsets must start at 0"):
        capi.shot_lrf(ctx, cloud, np.array([1, 4, 8], np.uint32), *k, 0.3)
    with pytest.raises(capi.IsmHipError, match="voxel_keypoints: offsets must start at 0"):
        capi.voxel_keypoints(ctx, np.array([1, 4, 8], np.uint32), *p[:3], 0.5)
    cloud.close()
