"""Runs without a GPU: proves, through maxima_model (a host model of maxima.hip's launch decisions) and the oracle, that every scene
of maxima_scenes.py reaches the path test_gpu_maxima.py runs it for, and holds the oracle to an independent float64 restatement of
the Hough space (hough_ref) and to closed forms on the exact scenes. Each proof is stated once, in its test's docstring.

Mutation check (on a scratch copy of the oracle, never committed; each edit alone, this file run against the edited library).
cnt[0] and cnt[1] exchanged in the bin index of ismref_hough3d_maxima, three ways: in the accumulation only (the plain index and the
interpolation stride), in the accumulation and the neighbour lookup, and consistently in accumulation, decode and lookup -- each
fails test_lattice_oracle_matches_hough_ref at every rel (the consistent one only because of the (25, 14, 14) / (0, 15, 14) pair);
>= for > in the neighbour test fails it at rel 0.5 and fails test_class_bins_oracle_matches_hough_ref[lattice]; <= for < in
`v < thr` fails it at every rel; `iter <= max_iter + 1` (one more mean-shift iteration) fails
test_chain_closed_form_counts_the_iterations and test_three_blobs_tell_iteration_counts_apart."""
import numpy as np
import pytest

import hough_ref
import maxima_model as mm
import maxima_scenes as ms

K = mm.K
INT_KEYS = ("n", "cls", "inst", "n_votes")
FLOAT_KEYS = ("pos", "weight", "inst_weight", "bbox_size", "class_score")


def same_as_ref(got, ref, atol=1e-6):
    """integers equal; floats within float32 rounding of the float64 restatement (the inputs make every SUM exact, the final
    divisions round once)"""
    for key in INT_KEYS:
        assert np.array_equal(got[key], ref[key]), key
    for key in FLOAT_KEYS:
        np.testing.assert_allclose(got[key], ref[key], atol=atol, rtol=0, err_msg=key)


def test_kernel_constants_are_what_the_scenes_were_built_for():
    assert K == dict(LDS_SLOTS=2048, MAXM=1024, MAXM_C=128, MAXC=256)
    assert mm.pow2_cap(0) == 64 and mm.pow2_cap(64) == 64 and mm.pow2_cap(65) == 128
    assert [mm.hough_tile_edge(c, False) for c in (64, 1024, 2048)] == [24, 24, 21] and mm.hough_tile_edge(4096, True) == 24


# ------------------------------------------------------------------------------------------------ Hough3D
@pytest.mark.parametrize("run,cap,big,edge,seam", [("alone", 128, False, 24, 22), ("cap2048", 2048, False, 21, 19), ("workspace", 4096, True, 24, 22)])
def test_lattice_has_pairs_on_the_seams_of_every_tile_edge(run, cap, big, edge, seam):
    """the three runs of the lattice take cap <= 1024 / cap 2048 / the workspace path, hence tile edges 24 / 21 / 24; the lattice's
    reachable-bin box is the whole non-cubic space, cut once per axis, at bin 22 or 19; on each of the three axes a plateau pair and
    two steps (up and down) have their bins on either side of exactly that seam"""
    off, v, R = ms.lattice_run(run)
    assert mm.launch(off) == (cap, big) and mm.hough_tile_edge(cap, big) == edge
    cnt = hough_ref.bin_counts(ms.LAT_MIN, ms.LAT_MAX, ms.LAT_BIN)
    assert tuple(cnt) == ms.LAT_CNT and len(set(cnt)) == 3
    assert (ms.LAT_MAX[1] - ms.LAT_MIN[1]) / ms.LAT_BIN % 1 != 0                       # the last y bin is a partial one
    sel = v["cls"] == 0
    bins = [b for b in (hough_ref.vote_bin(p, ms.LAT_MIN, ms.LAT_BIN, cnt) for p in v["pos"][sel]) if b is not None]
    assert len(bins) == sel.sum() - 1                                                  # only the vote at max_coord is outside
    lo, hi = mm.reachable_box(bins, cnt)
    assert lo == [0, 0, 0] and hi == [c - 1 for c in cnt]
    nt, seams = mm.hough_tiles(lo, hi, edge)
    assert nt == [2, 2, 2] and seams == [[seam]] * 3
    for d in range(3):
        for kind, want in (("plateau", 1), ("step", 2)):
            on = [(a, b) for a, b in R[kind] if abs(a[d] - b[d]) == 1 and {a[d], b[d]} == {seam - 1, seam}]
            assert len(on) == want, (d, kind)
    if big:
        counts = mm.class_counts(off, v["cls"], 2)
        assert mm.class_caps(counts)[0].tolist() == [mm.pow2_cap(sel.sum()), 64] and counts[1].tolist() == [0, 0]


@pytest.mark.parametrize("rel", [0.5, 1.0, 1.5])
@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interpolated"])
def test_lattice_oracle_matches_hough_ref(ora, interp, rel):
    """the oracle equals the float64 restatement on the lattice (integers exactly, floats to 1e-6), every accumulator value is a
    multiple of 2^-12 (exact in double and in 2^-40 fixed point), and the planted relations hold in the restatement: plateau pairs
    are two maxima of equal value, of a step only the higher bin is one, the bins exactly at rel * max(H) are kept and those one
    64th below are dropped, the bin-0 and last-bin maxima exist, the boundary vote makes a plateau of two under interpolation and
    one bin without, the vote at min_coord counts (1/8 of it under interpolation), a centred vote is no voter of a neighbour"""
    off, v, R = ms.lattice()
    kw = dict(ms.LAT_KW, use_interpolation=interp, rel_threshold=rel)
    got, ref = ora.hough3d_maxima(off, v, **kw), hough_ref.hough3d_maxima(off, v, **kw)
    same_as_ref(got, ref)
    sel = v["cls"] == 0
    cnt, H = hough_ref.accumulate(v["pos"][sel].astype(np.float64), v["weight"][sel].astype(np.float64), ms.LAT_MIN, ms.LAT_MAX, ms.LAT_BIN, interp)
    assert all(e[0] * 4096 == int(e[0] * 4096) for e in H.values())
    assert max(e[0] for e in H.values()) == 2.0
    maxima = {b for c, b, _ in ref["bins"][0] if c == 0}
    assert len(ref["bins"][0]) == ref["n"][0] < ms.LAT_MAXIMA                          # nothing cut by the output capacity
    idx = ms.lattice_bin_index
    val = lambda b: H[idx(b)][0] if idx(b) in H else 0.0
    is_max = lambda b: idx(b) in maxima
    eff = min(rel, 1.0)
    for a, b in R["plateau"]:
        assert val(a) == val(b) == 1.0 and is_max(a) == is_max(b) == (eff == 0.5)
    for low, high in R["step"]:
        assert val(low) == 1.0 < val(high) == 1.25 and not is_max(low) and is_max(high) == (eff == 0.5)
    for b, at in R["kept"]:
        assert val(b) == at * 2.0 and is_max(b) == (at >= eff)
    for b, at in R["dropped"]:
        assert val(b) == at * 2.0 - 1 / 64 and is_max(b) == (at > eff)
    for b in R["first"] + R["last"]:
        assert val(b) == 1.0 and is_max(b) == (eff == 0.5)
        assert len(H[idx(b)][1]) == 1
        assert not [i for i in H if i != idx(b) and max(abs(i % 26 - b[0]), abs(i // 26 % 25 - b[1]), abs(i // 650 - b[2])) <= 1]
    lo, hi = R["boundary"]
    assert (val(lo), val(hi)) == ((1.0, 1.0) if interp else (0.0, 2.0)) and is_max(hi) == (not interp or eff == 0.5) and is_max(lo) == (interp and eff == 0.5)
    assert val(R["corner"]) == (0.125 if interp else 1.0)


@pytest.mark.parametrize("scene", ["lattice", "random"])
@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interpolated"])
def test_class_bins_oracle_matches_hough_ref(ora, scene, interp):
    """three classes with three bin sizes in one space have three different, non-cubic bin grids, every class has maxima, and the
    oracle equals the restatement (on the lattice to 1e-6, on the random scene to float32 rounding of its sums: 1e-5)"""
    off, v = ms.class_bin_scenes()[scene]
    grids = [tuple(hough_ref.bin_counts(ms.LAT_MIN, ms.LAT_MAX, b)) for b in ms.CB_BINS]
    assert len(set(grids)) == 3 and all(len(set(g)) >= 2 for g in grids)
    kw = dict(ms.CB_KW, use_interpolation=interp)
    got, ref = ora.hough3d_maxima(off, v, **kw), hough_ref.hough3d_maxima(off, v, **kw)
    same_as_ref(got, ref, atol=1e-6 if scene == "lattice" else 1e-5)
    assert set(got["cls"][got["cls"] >= 0].tolist()) == {0, 1, 2} and got["n"].max() < 32


def test_hough_filters_remove_maxima_on_the_colliding_scenes(ora):
    """on the colliding-classes scene MaxFilterType Simple, and on the stacked-classes scene Merge, leave fewer Hough3D maxima than
    no filter does: the filters have something to do there"""
    for scene, flt in ((ms.colliding_classes_scene, 1), (ms.stacked_classes_scene, 2)):
        off, v = scene()
        kw = dict(n_classes=5, bin_size=0.5, rel_threshold=0.3, max_maxima=32, min_votes_threshold=2)
        plain, filt = ora.hough3d_maxima(off, v, **kw), ora.hough3d_maxima(off, v, max_filter=flt, **kw)
        assert filt["n"].sum() < plain["n"].sum() and plain["n"].max() < 32, flt


@pytest.mark.parametrize("n", [128, 129])
def test_isolated_bins_are_one_maximum_each(ora, n):
    """n unit votes sit in n distinct bins no two of which are 26-neighbours, so the oracle finds n maxima of one class: exactly the
    per-class capacity, and one more"""
    off, v = ms.isolated_bins(n)
    cnt = hough_ref.bin_counts((-5,) * 3, (5,) * 3, 0.25)
    b = np.asarray([hough_ref.vote_bin(p, (-5,) * 3, 0.25, cnt) for p in v["pos"]])
    cheb = np.abs(b[:, None] - b[None]).max(-1) + 2 * np.eye(n, dtype=np.int64)
    assert cheb.min() >= 2
    got = ora.hough3d_maxima(off, v, n_classes=1, bin_size=0.25, rel_threshold=0.5, max_maxima=256)
    assert got["n"][0] == n and (n == K["MAXM_C"] or n == K["MAXM_C"] + 1)


# ------------------------------------------------------------------------------------------------ mean shift
@pytest.mark.parametrize("n_per_class,n_classes", [(7, 3), (128, 8), (120, 9), (128, 1), (129, 1)])
def test_isolated_votes_closed_form(ora, n_per_class, n_classes):
    """votes 16 bandwidths apart under the uniform kernel: the oracle returns every vote as its own maximum at its own position,
    one voter, weight 1 / N, classes ascending and slot order within a class. 8 x 128 is exactly the per-object capacity, 9 x 120
    exceeds it on the LDS path with cap 2048, 128 / 129 of one class meet and exceed the per-class capacity"""
    off, v = ms.isolated_votes(n_per_class, n_classes)
    total = n_per_class * n_classes
    out = ora.find_maxima(off, v, n_classes=n_classes, max_maxima=1100, **ms.ISO_KW)
    ms.assert_isolated(out, ms.isolated_closed_form(n_per_class, n_classes))
    d = np.abs(v["pos"][:, None, 0] - v["pos"][None, :, 0])
    assert d[(v["cls"][:, None] == v["cls"][None]) & (d > 0)].min() >= 10 * ms.ISO_H
    cap, big = mm.launch(off)
    assert not big and cap == mm.pow2_cap(total)
    if (n_per_class, n_classes) == (128, 8):
        assert total == K["MAXM"] and n_per_class == K["MAXM_C"]
    if (n_per_class, n_classes) == (120, 9):
        assert total > K["MAXM"] and n_per_class < K["MAXM_C"] and cap == 2048


def test_three_blobs_tell_iteration_counts_apart(ora):
    """with threshold 0 the oracle's maxima for max_iter 0, 1, 2, 3 differ pairwise between consecutive values, in number or by more
    than ten times the position tolerance (2e-2): one iteration more or fewer on the device cannot pass the parity test"""
    off, v = ms.three_blobs()
    outs = [ora.find_maxima(off, v, n_classes=1, bandwidth=0.5, threshold=0.0, max_iter=k, max_maxima=16) for k in range(5)]
    for a, b in zip(outs, outs[1:]):
        assert a["n"][0] != b["n"][0] or np.abs(a["pos"] - b["pos"]).max() > 2e-2
    assert [int(o["n"][0]) for o in outs[:4]] == [6, 3, 4, 3]


def test_chain_closed_form_counts_the_iterations(ora):
    """four unit votes, uniform kernel, h = 1: of the seeds (cell centres of the votes) only the one at the origin has a vote in
    range, vote 0 alone; from the mean of votes 0..k-1 exactly the votes 0..k are in range (margins > 0.01 in d^2), so step k ends
    on the mean of the first k votes and max_iter = m gives the mean of the first min(m + 1, 4), with the voters that this centre
    sees. The oracle follows this closed form for m = 0..5: an off-by-one in `iter <= max_iter` cannot."""
    off, v = ms.chain()
    P = ms.CHAIN.astype(np.float64)
    cell = 2 * ms.CHAIN_H / np.sqrt(2.0)
    seeds = np.unique(np.floor(P / cell + 0.5), axis=0) * cell
    assert len(seeds) == 2
    d2 = lambda q: ((P - q) ** 2).sum(1)
    seen = [np.flatnonzero(d2(s) < 1.0).tolist() for s in seeds]
    assert sorted(seen) == [[], [0]]
    means = [P[:k].mean(0) for k in range(1, 5)]
    for k, c in enumerate(means):
        want = list(range(min(k + 2, 4)))
        assert np.flatnonzero(d2(c) < 1.0 - 0.01).tolist() == want and np.flatnonzero(d2(c) < 1.0 + 0.01).tolist() == want
    assert min(np.abs(a - b).max() for a, b in zip(means, means[1:])) > 2e-2
    for m in range(6):
        out = ora.find_maxima(off, v, max_iter=m, **ms.CHAIN_KW)
        k = min(m, 3)
        assert out["n"][0] == 1 and out["n_votes"][0, 0] == min(k + 2, 4)
        np.testing.assert_allclose(out["pos"][0, 0], means[k], atol=1e-6)


def test_seed_rows_sit_on_the_rounding_boundary(ora):
    """(h * 2) / sqrtf(2) is exactly 0.5 in float32 for h = float32(0.35355338); every vote of the rows has x / 0.5 exactly
    half-integral, negative and positive, and y, z on cell centres; the oracle's seeds for them are the cells k + 1 (round half up,
    both signs), and it finds maxima. A vote with two or three coordinates on the boundary is out of its seed's range: no maxima"""
    h = np.float32(ms.SEED_H)
    cell = np.float32(np.float32(h * np.float32(2)) / np.sqrt(np.float32(2)))
    assert cell == np.float32(0.5)
    off, v = ms.seed_boundary_rows()
    q = v["pos"] / cell
    assert (q[:, 0] % 1 == 0.5).all() and (q[:, 1:] % 1 == 0).all() and (q[:, 0] < 0).any() and (q[:, 0] > 0).any()
    sp, _ = ora.create_seeds(v["pos"], v["weight"], float(cell))
    want = np.unique(np.stack([np.floor(q[:, 0]) + 1, q[:, 1], q[:, 2]], 1), axis=0) * 0.5
    assert sorted(map(tuple, sp.tolist())) == sorted(map(tuple, want.tolist()))
    out = ora.find_maxima(off, v, n_classes=1, bandwidth=ms.SEED_H, kernel=1, suppression=1, max_maxima=32)
    assert 6 <= out["n"][0] < 32
    h2 = np.float32(np.float64(h) * np.float64(h))
    for nc, d2 in ((2, 0.125), (3, 0.1875)):
        off1, v1 = ms.seed_boundary_corner(nc)
        assert not np.float32(d2) < h2
        assert ora.find_maxima(off1, v1, n_classes=1, bandwidth=ms.SEED_H, kernel=1, suppression=1, max_maxima=4)["n"][0] == 0


@pytest.mark.parametrize("case", ms.TALLY_CASES)
def test_tally_scenes_reach_the_table_edges_and_follow_the_rule(ora, case):
    """full64 / full256: as many distinct ids as the table has entries; collide: twelve ids with one first probe slot within 6 of
    the table's end, so the chain wraps to slot 0 and probes 11 deep; negative / equal: the two best sums are exactly equal and the
    lower unsigned id is expected; zero: an instance of weight 0 is present. In every case the blob is one maximum holding all
    votes, and the oracle's instance and instance weight follow the rule (largest sum, lowest unsigned id among equals), through
    mean shift and through a one-bin Hough space"""
    off, v = ms.tally(case)
    n = len(v["weight"])
    cap, big = mm.launch(off)
    ids = v["inst"]
    slot_of, longest, wrapped = mm.probe_table(ids, cap)
    assert not big and int(0x80000000 - (1 << 32)) not in ids.tolist()
    if case.startswith("full"):
        assert n == cap == len(slot_of)
    if case == "collide":
        assert len({mm.first_probe(i, cap) for i in ids}) == 1 and mm.first_probe(ids[0], cap) >= cap - 6
        assert len(slot_of) == 12 and longest == 11 and wrapped
    sums = {}
    for i, w in zip(ids.tolist(), v["weight"].tolist()):
        sums[i] = sums.get(i, 0.0) + w
    top = sorted(sums.values())[-2:]
    if case in ("negative", "equal") or case.startswith("full"):
        assert top[0] == top[1]
    if case == "negative":
        assert {i for i in sums if sums[i] == top[1]} == {-7, 7}
    if case == "zero":
        assert min(sums.values()) == 0.0
    inst, iw = hough_ref.best_instance(ids, v["weight"])
    assert inst == {"negative": 7, "equal": 4, "zero": 1}.get(case, inst)
    for out in (ora.find_maxima(off, v, **ms.TALLY_MS), ora.hough3d_maxima(off, v, n_classes=1, max_maxima=4, **ms.TALLY_HOUGH)):
        assert out["n"][0] == 1 and out["n_votes"][0, 0] == n and out["inst"][0, 0] == inst
        assert out["inst_weight"][0, 0] == 1.0 and out["weight"][0, 0] == 1.0          # normalised over the one maximum


def test_zero_weight_blob_is_the_undefined_case(ora):
    """all members of weight 0: the oracle (as the reference) divides by the zero weight sum, so its box size is NaN while every
    other output is finite -- the pattern test_gpu_maxima pins; Hough3D finds nothing in an empty accumulator"""
    off, v = ms.zero_weight_blob()
    out = ora.find_maxima(off, v, **ms.TALLY_MS)
    assert out["n"][0] == 1 and np.isnan(out["bbox_size"][0, 0]).all()
    assert all(np.isfinite(out[k]).all() for k in ("pos", "weight", "inst_weight", "class_score"))
    assert ora.hough3d_maxima(off, v, n_classes=1, max_maxima=4, **ms.TALLY_HOUGH)["n"][0] == 0


# ------------------------------------------------------------------------------------------------ both paths, many pairs
def test_options_scene_takes_both_paths_and_every_option_bites(ora):
    """the scene alone takes the LDS path, with the 2049-slot object appended the workspace path, and the first seven objects are the
    same votes in both calls; on the scene, every option set changes the oracle's answer against the default (so a kernel that
    ignored the option would fail), suppression NONE gives no maxima, and both filters remove maxima"""
    (off, v), (off2, v2), cen, rad = ms.options_scene()
    assert mm.launch(off) == (mm.pow2_cap(np.diff(off.astype(np.int64)).max()), False) and mm.launch(off2) == (4096, True)
    n_obj, n = len(off) - 1, len(v["weight"])
    assert np.array_equal(off2[:n_obj + 1], off) and all(np.array_equal(v2[k][:n], v[k]) for k in v) and off2[-1] - off2[-2] == K["LDS_SLOTS"] + 1
    assert (mm.class_counts(off2, v2["cls"], ms.OPT_CLASSES)[-1] > 256).all()             # the big object's tables are larger than any LDS-path cap here
    som = dict(object_centroid=cen[:n_obj], object_radius=rad[:n_obj])
    base = ora.find_maxima(off, v, **ms.MS_BASE)
    assert base["n"].sum() >= 10
    for name, opt in ms.MS_OPTIONS.items():
        kw = dict(ms.MS_BASE, **opt)
        out = ora.find_maxima(off, v, **kw, **(som if name.startswith("som") else {}))
        if name == "none":
            assert out["n"].sum() == 0
        elif name in ("simple", "merge", "merge_class_bandwidth"):
            assert out["n"].sum() < ora.find_maxima(off, v, **dict(kw, max_filter=0))["n"].sum(), name
        elif name == "rotation":
            assert np.abs(out["bbox_quat"][:, :, 1:]).max() > 0.1
        elif name not in ("average", "suppress"):
            assert not np.array_equal(out["n"], base["n"]) or np.abs(out["pos"] - base["pos"]).max() > 2e-2 or np.abs(out["weight"] - base["weight"]).max() > 1e-3, name
    hbase = ora.hough3d_maxima(off, v, **ms.HOUGH_BASE)
    assert hbase["n"].sum() >= 10
    for name, opt in ms.HOUGH_OPTIONS.items():
        kw = dict(ms.HOUGH_BASE, **opt)
        out = ora.hough3d_maxima(off, v, **kw)
        if name in ("simple", "merge"):
            assert out["n"].sum() < ora.hough3d_maxima(off, v, **dict(kw, max_filter=0))["n"].sum(), name
        elif name in ("plain", "class_bin"):
            assert not np.array_equal(out["n"], hbase["n"]) or np.abs(out["weight"] - hbase["weight"]).max() > 1e-3, name


def test_many_pairs_need_the_second_chunk_of_the_offsets(ora):
    """9 x 128 = 1152 (object, class) pairs exceed one pass of k_work_offsets; object 8 alone exceeds the LDS slots, so the call takes
    the workspace path, and all its pairs (1024..1151) get their offsets in the second pass, on top of the carry of the first; every
    one of its regions is used (18 votes -> 64 slots). The oracle finds one maximum per class there and dozens on the small objects"""
    off, v = ms.many_pairs()
    cap, big = mm.launch(off)
    sizes = np.diff(off.astype(np.int64))
    assert big and sizes.tolist() == [200] * 8 + [2304]
    counts = mm.class_counts(off, v["cls"], ms.MANY_CLASSES)
    assert counts.size == 1152 > mm.OFFSET_CHUNK
    offs, chunk = mm.work_offsets(counts)
    assert (chunk[ms.MANY_BIG] == 1).all() and (chunk[:ms.MANY_BIG] == 0).all() and (counts[ms.MANY_BIG] == 18).all()
    carry = int(np.where(counts[:8] > 0, 64, 0).sum())
    assert offs[ms.MANY_BIG].tolist() == [carry + 64 * c for c in range(128)] and carry > 0
    for out in (ora.find_maxima(off, v, n_classes=128, bandwidth=0.5, max_maxima=160),
                ora.hough3d_maxima(off, v, n_classes=128, bin_size=0.5, rel_threshold=0.5, max_maxima=160)):
        assert out["n"][ms.MANY_BIG] == 128 and sorted(out["cls"][ms.MANY_BIG, :128].tolist()) == list(range(128))
        assert out["n"][:8].min() >= 40 and out["n"].max() < 160


def test_chunk_edge_pairs_put_one_pair_past_the_first_pass(ora):
    """5 x 205 = 1025 pairs: the last one, (4, 204), is the only entry of the second pass of k_work_offsets and its region starts at
    the sum of all the others; object 0 sends the call down the workspace path; both pairs beside the edge hold votes and a maximum"""
    off, v = ms.chunk_edge_pairs()
    cap, big = mm.launch(off)
    assert big and np.diff(off.astype(np.int64)).tolist() == ms.EDGE_SIZES
    counts = mm.class_counts(off, v["cls"], ms.EDGE_CLASSES)
    assert counts.size == mm.OFFSET_CHUNK + 1
    offs, chunk = mm.work_offsets(counts)
    assert chunk.ravel().tolist() == [0] * mm.OFFSET_CHUNK + [1] and counts[4, -2:].min() >= 40
    assert offs[4, -1] == offs[4, -2] + 64 and offs[4, -1] == sum(0 if c == 0 else max(64, 1 << int(c - 1).bit_length()) for c in counts.ravel()[:-1].tolist())
    out = ora.find_maxima(off, v, n_classes=ms.EDGE_CLASSES, bandwidth=0.5, max_maxima=256)
    assert out["n"][0] == ms.EDGE_CLASSES and {ms.EDGE_CLASSES - 2, ms.EDGE_CLASSES - 1} <= set(out["cls"][4, :out["n"][4]].tolist())

