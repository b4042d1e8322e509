"""Runs without a GPU: proves that the scenes of test_gpu_frontend.py reach the kernel paths they are built for (grid_model is a
host model of the device grid and of ball_for_each), that the planted ties and boundaries are real, and holds the oracle's
SHOT-352 against an independent float64 restatement (shot_ref) on exactly those boundaries.

Path thresholds come from the kernel sources (grid_model.K). Conditions that rest on the model's approximate float rounding carry
a 1.5x margin; conditions on exact counts (mirror clouds, clusters, the lattice) are asserted exactly."""
import numpy as np
import pytest

import frontend_scenes as fs
import grid_model as gm
import shot_ref

K = gm.K
MARGIN = 1.5


def test_kernel_constants_are_what_the_scenes_were_built_for():
    assert K["ROW_BATCH"] == 64 and K["ROWS_CAP"] == 4096 and K["GRID_MAXDIM"] == 32 and K["GRID_XFRAC"] == 3
    assert K["TIE_LDS_KEYS"] == 8192 and K["TIE_REG_KEYS"] == 20 and K["TIE_BLOCKS"] == 1024
    assert K["GRID_FUSED_MAX_PTS"] == 65536 and K["QUEUE"] == 128


@pytest.mark.parametrize("far", [False, True], ids=["origin", "far"])
@pytest.mark.parametrize("n_surface", [fs.FUSED_SURFACE, fs.WIDE_SURFACE])
def test_dense_object_reaches_row_batches_and_windows(n_surface, far):
    p, _, kp = fs.dense_object(n_surface)
    if far:
        p, kp = fs.translated(p, kp)
    g = gm.Grid(p, fs.DENSE_CELL)
    assert g.dim.tolist() == [31, 24, 14]
    sw = [g.sweep(q, fs.DENSE_RADIUS) for q in kp]
    rows_min, cap_min = MARGIN * K["ROW_BATCH"], MARGIN * K["ROWS_CAP"]
    assert sum(s["rows"] >= rows_min for s in sw) >= 20                      # a second row batch
    assert sum(max(s["batches"]) >= cap_min for s in sw) >= 8                # a second candidate window inside one batch
    assert sum(s["longest_row"] >= cap_min for s in sw) >= 8                 # ONE row longer than a window: its end mark lands in a later one
    assert min(s["rows"] for s in sw) >= 2 * K["ROW_BATCH"] + 1              # in fact every keypoint sweeps three batches


def test_build_sizes_straddle_the_fused_limit():
    assert fs.FUSED_SURFACE + 20000 <= K["GRID_FUSED_MAX_PTS"] < fs.WIDE_SURFACE + 20000
    for ns in (fs.FUSED_SURFACE, fs.WIDE_SURFACE):
        b = fs.wide_batch(ns, with_color=False)
        sizes = [len(o[0]) for o in b["objs"]]
        assert max(sizes) == ns + 20000 and 0 in sizes and 4 in sizes
        assert len(sizes) >= 9 and len(sizes) % 8 != 0                       # XCD block map with padding blocks
        assert len(set(len(k) for k in b["kps"])) >= 6                       # uneven keypoint counts
    far = b["objs"][3][0]
    assert np.abs(far).min(0).max() >= 1000                                  # where |q| * 4e-7 exceeds r * 1e-5 in ball_cells


def test_grid_build_scenes_lie_on_both_sides_of_the_scan_chunk():
    """the five-kernel grid build scans an object's cell counts 1024 at a time (k_scan): the batches that test_gpu_grid_fused.py
    compares byte for byte hold objects that need one pass, objects that need three or more, and the largest table there is"""
    import test_gpu_grid_fused as gf
    for seed in (11, 12, 13):                                                # the seeds of its comparisons
        cells = [int(gm.Grid(p, gf.CELL).dim.prod()) for p, _ in gf._objects(np.random.default_rng(seed))]
        assert min(cells) <= 1024 and sum(1024 < c < 2049 for c in cells) >= 1 and sum(c >= 2049 for c in cells) >= 3
        assert max(cells) > 28 * 1024                                        # 29 carries in one object


@pytest.mark.parametrize("xfrac", [None] + fs.XFRACS)
def test_thin_batch_changes_its_grid_with_the_x_fraction(xfrac):
    """the scene of the ISMHIP_GRID_XFRAC cases: below the per-axis cap on x at every tested fraction, so each value builds another
    grid than the default, and the dense paths are still taken on each of them"""
    b = fs.thin_batch()
    default = K["GRID_XFRAC"]
    assert default not in fs.XFRACS
    for o in (0, 1, 2, 3):
        g, g0 = gm.Grid(b["objs"][o][0], fs.THIN_CELL, xfrac=xfrac), gm.Grid(b["objs"][o][0], fs.THIN_CELL)
        v = xfrac or default
        assert g.dim[0] < K["GRID_MAXDIM"] - 1 and abs(float(g.cell[0]) * v / fs.THIN_CELL - 1) < 1e-6       # not capped: the cell asked for
        if xfrac:
            assert g.dim[0] != g0.dim[0] and g.cell[0] != g0.cell[0] and g.dim[1:].tolist() == g0.dim[1:].tolist()
    for o in (0, 1):
        g = gm.Grid(b["objs"][o][0], fs.THIN_CELL, xfrac=xfrac)
        sw = [g.sweep(q, fs.THIN_RADIUS) for q in b["kps"][o]]
        assert sum(s["rows"] >= MARGIN * K["ROW_BATCH"] for s in sw) >= 20
        assert sum(max(s["batches"]) >= MARGIN * K["ROWS_CAP"] for s in sw) >= 8
        assert sum(s["longest_row"] >= MARGIN * K["ROWS_CAP"] for s in sw) >= 8


def test_fpfh_clump_fills_a_second_window():
    p, _, kp = fs.fpfh_clump_object()
    g = gm.Grid(p, fs.DENSE_CELL)
    clump = p[6000:]
    d = np.sqrt(((clump[None].astype(np.float64) - kp[:, None]) ** 2).sum(-1))
    assert ((d < fs.FPFH_CLUMP_RADIUS).sum(1) >= 500).all()                  # every keypoint marks hundreds of clump points for k_spfh
    near = clump[(d < fs.FPFH_CLUMP_RADIUS).any(0)][::25]
    sw = [g.sweep(q, fs.FPFH_CLUMP_RADIUS) for q in near]
    assert len(sw) >= 20 and min(max(s["batches"]) for s in sw) >= MARGIN * K["ROWS_CAP"]


def test_fpfh_and_normal_sweeps_take_a_second_row_batch():
    b = fs.wide_batch(fs.FUSED_SURFACE, with_color=False)
    g = gm.Grid(b["objs"][fs.FPFH_OBJECT][0], fs.DENSE_CELL)
    kp = b["fpfh_kps"][fs.FPFH_OBJECT]
    assert len(kp) == 12
    rows = [g.sweep(q, fs.FPFH_RADIUS)["rows"] for q in kp]
    assert min(rows) >= MARGIN * K["ROW_BATCH"], rows
    # k_spfh sweeps the ball of every NEIGHBOUR of a keypoint: those next to the keypoint see the same rows
    p = b["objs"][fs.FPFH_OBJECT][0]
    near = p[((p - kp[0]) ** 2).sum(1) < 0.05 ** 2]
    assert len(near) >= 5 and min(g.sweep(q, fs.FPFH_RADIUS)["rows"] for q in near) >= MARGIN * K["ROW_BATCH"]
    sc = fs.normals_scene()
    g = gm.Grid(sc[0], fs.NORMALS_CELL)
    rows = np.array([g.sweep(q, fs.NORMALS_RADIUS)["rows"] for q in sc[0][:6000:100]])
    assert (rows >= MARGIN * K["ROW_BATCH"]).sum() >= 20, rows                # every point is a query of k_pca_normals


@pytest.mark.parametrize("m", fs.MIRROR_M)
def test_mirror_clouds_tie_both_signs(ora, m):
    pts = fs.mirror_cloud(m)
    d2 = (pts.astype(np.float64) ** 2).sum(1)
    assert len(pts) == 2 * m and d2.max() < (0.9 * fs.MIRROR_RADIUS) ** 2 and d2.min() > 0    # the neighbourhood is the whole cloud
    z = np.zeros(1, np.float32)
    f = ora.shot_lrf(np.array([0, 2 * m], np.uint32), *fs.cols(pts), np.array([0, 1], np.uint32), z, z, z, fs.MIRROR_RADIUS)
    assert np.isfinite(f).all()
    assert fs.sign_sums(pts, f[0]) == (0, 0)                                 # real ties: the median neighbours decide x AND z


def test_mirror_sizes_straddle_every_key_store():
    reg, lds = 64 * K["TIE_REG_KEYS"], K["TIE_LDS_KEYS"]
    n = [2 * m for m in fs.MIRROR_M]
    assert n == [800, 1280, 1282, 3000, 8192, 8194, 12000]
    assert reg in n and reg + 2 in n and lds in n and lds + 2 in n           # the last size of a store and the first of the next
    assert any(x < reg for x in n) and any(reg + 2 < x < lds for x in n) and any(x > lds + 2 for x in n)
    assert fs.QUEUE_KEYPOINTS > K["TIE_BLOCKS"]                              # more ties than tie workgroups: the work-queue loop runs


@pytest.mark.parametrize("frame", range(3))
def test_lattice_sits_on_every_hard_decision(frame):
    fr = fs.LATTICE_FRAMES[frame]
    R = fr.reshape(3, 3).astype(np.float64)
    assert np.array_equal(R @ R.T, np.eye(3)) and np.linalg.det(R) == 1      # an exact signed permutation
    p, n = fs.lattice(fr)
    want = {0.25: dict(n=27, x0=9, y0=9, z0=9, diag=15, shell=6, on_radius=6),
            0.5: dict(n=251, x0=45, y0=45, z0=45, diag=55, shell=6, on_radius=6),
            0.75: dict(n=673, x0=81, y0=81, z0=81, diag=129, shell=30, on_radius=24)}
    for r in fs.LATTICE_RADII:
        assert fs.lattice_census(p, fr, r) == want[r]
    cos = n @ fr.reshape(3, 3)[2]                                            # float32, exact: the frame is a signed permutation
    edges = np.float32(fs.COS_EDGES)
    inside = (p.astype(np.float64) ** 2).sum(1) < 0.25
    for e in edges:                                                          # at radius 0.5 every edge is met from below, on it and from above
        got = set(cos[inside][np.abs(cos[inside] - e) < 1e-6].tolist())
        assert got == {float(np.nextafter(e, np.float32(-2))), float(e), float(np.nextafter(e, np.float32(2)))}, (e, got)


def test_lattice_colours_sit_on_the_colour_bin_edges(ora):
    found = fs.edge_colors(ora.rgb2lab, fs.EDGE_KP_COLOR, fs.EDGE_COLORS)
    assert [c for c, _, _ in found] == fs.EDGE_COLORS                        # every listed colour sits on an edge
    assert fs.edge_colors(ora.rgb2lab, fs.EDGE_KP_COLOR, range(1000, 1200)) == []   # ... which ordinary colours do not
    seen = {(k, side) for _, k, side in found}
    assert {v for _, v in seen} == {0, 1, 2} and len({k for k, _ in seen}) >= 12
    assert sum({(k, 0), (k, 1), (k, 2)} <= seen for k in range(1, 30)) >= 1      # one edge met from below, on it and from above
    p, _ = fs.lattice(fs.LATTICE_FRAMES[0])
    rgba = fs.lattice_colors(p)
    inside = ((p.astype(np.float64) ** 2).sum(1) < min(fs.LATTICE_RADII) ** 2) & ((p != 0).any(1))
    assert inside.sum() == 26 and set(rgba[inside].tolist()) == set(fs.EDGE_COLORS[:26])
    assert set(fs.EDGE_COLORS) <= set(rgba.tolist())


def test_queue_clusters_have_exact_counts():
    pts, _, kps, frames, counts = fs.queue_clusters()
    assert counts.tolist() == fs.QUEUE_COUNTS + [5]
    assert K["QUEUE"] // 2 in counts and K["QUEUE"] in counts                # one drain exactly when 64 are queued; 127 / 128 / 129: two drains and the wrap of the ring's head
    d = np.sqrt(((pts[None].astype(np.float64) - kps[:, None].astype(np.float64)) ** 2).sum(-1))
    inside = d < fs.QUEUE_RADIUS
    assert inside.sum(1).tolist() == counts.tolist() and (inside.sum(0) == 1).all()
    assert d[inside].max() < 0.9 * fs.QUEUE_RADIUS and d[~inside].min() > 2 * fs.QUEUE_RADIUS
    assert (d[-1] == 0).sum() == 1                                           # the last cluster holds its keypoint
    for f in frames:
        R = f.reshape(3, 3).astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6


def test_fpfh_edge_objects_put_f3_on_the_edges(ora):
    objs, kps = fs.fpfh_edge_objects()
    assert len(objs) == 30
    seen = set()
    for (p, n) in objs:
        for q in (1, 2, 3):
            for a, b in ((0, q), (q, 0)):                                    # the centre as source and as target: the same f3
                ok, f = ora.pair_features(p[a], n[a], p[b], n[b])
                assert ok and f[2] == n[0, 0], (f, n[0])
                t1, t2 = 11 * (f[0] + np.pi) / (2 * np.pi), 11 * (f[1] + 1) / 2
                assert min(t1 - np.floor(t1), np.ceil(t1) - t1, t2 - np.floor(t2), np.ceil(t2) - t2) > 0.01
        t3 = 11 * (float(n[0, 0]) + 1) / 2
        assert abs(t3 - round(t3)) < 1e-5                                    # well inside the guard band of the fast bins (1e-4)
        seen.add((int(round(t3)), np.sign(t3 - round(t3))))
        ok, f = ora.pair_features(p[1], n[1], p[2], n[2])
        assert ok and abs(11 * (f[2] + 1) / 2 - 5.5) < 1e-6
    assert {j for j, _ in seen} == set(range(1, 11)) and len(seen) >= 20     # every edge, from both sides


# ---------------------------------------------------------------------------------------------- the oracle against the restatement
def test_oracle_shot352_matches_the_restatement_on_the_boundary_lattice(ora):
    """Measured maximum over 3 frames x 3 radii: 3.0e-8 (neighbour counts equal); bound = 10x. Any hard decision taken differently
    moves whole interpolation weights between bins: >= 1e-3 after normalisation."""
    z = np.zeros(1, np.float32)
    worst = 0.0
    for fr in fs.LATTICE_FRAMES:
        p, n = fs.lattice(fr)
        for r in fs.LATTICE_RADII:
            od, oc = ora.shot352(np.array([0, len(p)], np.uint32), *fs.cols(p), *fs.cols(n), np.array([0, 1], np.uint32), z, z, z, fr.reshape(1, 9), r)
            rd, rc, _ = shot_ref.shot352(p, n, np.zeros(3), fr, r)
            assert oc[0] == rc
            worst = max(worst, float(np.abs(od[0] - rd).max()))
    print("lattice: oracle vs restatement", worst)
    assert worst <= 3e-7, worst


def test_oracle_shot352_matches_the_restatement_on_dense_balls(ora):
    """Keypoints 0, 5 (beside the clump, ~24 000 neighbours) and 20 (surface, ~6 700) of the dense object, oracle frames.
    Measured maximum 4.0e-7 (the oracle accumulates in float like the reference, the restatement in float64); bound = 10x."""
    p, n, kp = fs.dense_object(fs.FUSED_SURFACE)
    sel = kp[[0, 5, 20]]
    po, ko = np.array([0, len(p)], np.uint32), np.array([0, 3], np.uint32)
    lrf = ora.shot_lrf(po, *fs.cols(p), ko, *fs.cols(sel), fs.DENSE_RADIUS)
    od, oc = ora.shot352(po, *fs.cols(p), *fs.cols(n), ko, *fs.cols(sel), lrf, fs.DENSE_RADIUS)
    worst = 0.0
    for i in range(3):
        rd, rc, _ = shot_ref.shot352(p, n, sel[i], lrf[i], fs.DENSE_RADIUS)
        assert rc == oc[i] and rc > 5000
        worst = max(worst, float(np.abs(od[i] - rd).max()))
    print("dense: oracle vs restatement", worst)
    assert worst <= 4e-6, worst
