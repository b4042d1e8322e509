"""GPU tests of the RANSAC vote filter (Voting.RansacVoteFiltering): the primitive ismhip_ransac_filter against planted
answers and against the numpy restatement (tests/ransac_ref.py) on the same draws, its edge cases, the filter inside
ismhip_find_maxima_ransac / ismhip_hough3d_maxima_ransac on synthetic vote arrays, the vote keypoint gathers, and the C++ host against the
Python harness with the reference's configuration keys."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import host_binding as hb
import ransac_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
THR = 0.1
SEED = 12345
# Fragility margin of the parity test: a cluster is left out when the restatement saw a d^2 within relative BETA of thr^2 in any
# hypothesis it evaluated. BETA = 100 x the largest relative difference of d^2 between the library's arithmetic and the restatement
# over the 300 parity clusters, hypotheses 0 .. 47 and every cluster's best one (14 700 hypotheses): 9.82e-13. Provenance: that
# figure is of csrc/ransac.h's model and scoring functions compiled for the host (same source and order of operations,
# -ffp-contract=off; double +, -, x, /, sqrt are correctly rounded on host and device alike). The parity test takes the same figure
# from the device through ismhip_ransac_hypothesis over the same hypothesis set, prints it, and fails if 100 x it exceeds BETA.
BETA = 9.82e-11


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q); w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def planted_cluster(rng, n, ni, thr=THR, R=None, t=None):
    """ni inliers under an exact rigid motion (rounded to float), n - ni outliers displaced by 10 .. 20 thresholds"""
    S = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    R = _rot(rng) if R is None else R
    t = rng.uniform(-2, 2, 3) if t is None else t
    T = S.astype(np.float64) @ R.T + t
    out = np.arange(n) >= ni
    u = rng.normal(size=(int(out.sum()), 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    T[out] += u * rng.uniform(10 * thr, 20 * thr, (int(out.sum()), 1))
    return S, T.astype(np.float32), ~out, R, t


def planted_clusters(count=200, seed=1):
    rng = np.random.default_rng(seed)
    cl = []
    for _ in range(count):
        n = int(rng.integers(8, 401)); ratio = rng.uniform(0.15, 0.9)
        cl.append(planted_cluster(rng, n, max(4, int(ratio * n))))
    return cl


def noisy_clusters(count=300, seed=2, thr=THR):
    """inlier noise sigma = 0.3 thr, outliers uniform within +-10 thr"""
    rng = np.random.default_rng(seed)
    cl = []
    for _ in range(count):
        n = int(rng.integers(8, 401)); ratio = rng.uniform(0.2, 0.9); ni = max(4, int(ratio * n))
        S = rng.uniform(-1, 1, (n, 3)).astype(np.float32); R = _rot(rng); t = rng.uniform(-2, 2, 3)
        T = S.astype(np.float64) @ R.T + t + rng.normal(size=(n, 3)) * (0.3 * thr)
        out = np.arange(n) >= ni
        T[out] += rng.uniform(-10 * thr, 10 * thr, (int(out.sum()), 3))
        cl.append((S, T.astype(np.float32), ~out, R, t))
    return cl


def _csr(clusters):
    import torch
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in clusters])]).astype(np.uint32)
    S = np.concatenate([c[0] for c in clusters]).astype(np.float32); T = np.concatenate([c[1] for c in clusters]).astype(np.float32)
    return off, torch.from_numpy(S), torch.from_numpy(T)


def run_filter(pkg, gpu, clusters, thr=THR, **kw):
    ctx, dev = gpu
    off, S, T = _csr(clusters)
    out = pkg.capi.ransac_filter(ctx, off, S.to(dev), T.to(dev), thr, **kw)
    ctx.sync()
    return off, {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def d2_gap(pkg, gpu, clusters, hyps, thr=THR, seed=SEED):
    """largest |d2_library - d2_restatement| / max(d2_restatement, thr^2) over the given hypotheses of every cluster"""
    ctx, dev = gpu
    off, S, T = _csr(clusters)
    Sd, Td = S.to(dev), T.to(dev)
    thr2 = float(np.float32(thr)) ** 2
    worst, n_cmp = 0.0, 0
    for h in hyps:
        hv = np.asarray(h if np.ndim(h) else [h] * len(clusters), np.int32)
        out = pkg.capi.ransac_hypothesis(ctx, off, Sd, Td, thr, hv, seed=seed)
        ctx.sync()
        d2, valid = out["d2"].cpu().numpy(), out["valid"].cpu().numpy()
        for c, cl in enumerate(clusters):
            ref = rr.hypothesis(cl[0], cl[1], thr, seed, int(hv[c]))
            assert bool(valid[c]) == bool(ref["valid"]), (c, int(hv[c]))
            if not ref["valid"] or ref["degenerate"]:
                continue
            got = d2[off[c]:off[c + 1]]
            worst = max(worst, float((np.abs(got - ref["d2"]) / np.maximum(ref["d2"], thr2)).max()))
            n_cmp += 1
    print("d2 gap: largest relative difference %.3e over %d hypotheses" % (worst, n_cmp))
    return worst


def _assert_transform(tf, R, t, tol):
    assert np.abs(tf[:3, :3].astype(np.float64) - R).max() < tol and np.abs(tf[:3, 3].astype(np.float64) - t).max() < tol, (tf, R, t)
    assert np.array_equal(tf[3], np.array([0, 0, 0, 1], np.float32))


def test_planted_sets_are_recovered_exactly(pkg, gpu):
    cl = planted_clusters()
    off, out = run_filter(pkg, gpu, cl)
    its = out["iterations"]
    print("planted sets: iterations min/median/max", its.min(), int(np.median(its)), its.max())
    for c, (S, T, inl, R, t) in enumerate(cl):
        assert out["kept"][c] == 1 and out["n_inliers"][c] == inl.sum(), c
        assert np.array_equal(out["inlier"][off[c]:off[c + 1]].astype(bool), inl), c
        _assert_transform(out["transform"][c], R, t, 1e-3)           # three float-rounded points, possibly a flat triangle, carry it
        ref = rr.hypothesis(S, T, THR, SEED, int(out["best_hypothesis"][c]))
        _assert_transform(out["transform"][c], ref["R"], ref["t"], 1e-6)
        assert 0 <= out["best_hypothesis"][c] < out["iterations"][c] <= 10001
    assert its.max() < 10000                                          # the sequential stop is exercised far below the cap


def test_parity_with_the_restatement_on_the_same_draws(pkg, gpu):
    cl = noisy_clusters()
    off, out = run_filter(pkg, gpu, cl)
    refs = [rr.ransac(S, T, THR, SEED, beta=BETA) for S, T, *_ in cl]
    fragile = [c for c, r in enumerate(refs) if r["fragile"]]
    print("parity: fragile clusters", len(fragile), "of", len(cl), "; hypotheses evaluated by the restatement", sum(r["evaluated"] for r in refs))
    assert len(fragile) <= 0.02 * len(cl)
    for c, r in enumerate(refs):
        if r["fragile"]:
            continue
        assert out["kept"][c] == int(r["kept"]) and out["best_hypothesis"][c] == r["best_i"] and out["iterations"][c] == r["iterations"], c
        assert out["n_inliers"][c] == r["n_inliers"], c
        assert np.array_equal(out["inlier"][off[c]:off[c + 1]].astype(bool), r["mask"]), c
        if r["kept"]:
            _assert_transform(out["transform"][c], r["R"], r["t"], 1e-6)
    # the margin's provenance still holds: the library's d^2 differs from the restatement's by far less than BETA
    gap = d2_gap(pkg, gpu, cl, list(range(48)) + [np.maximum(out["best_hypothesis"], 0)])
    assert gap * 100 <= BETA * 1.01, gap


def test_edge_cases_of_the_primitive(pkg, gpu):
    rng = np.random.default_rng(3)
    few = planted_cluster(rng, 2, 2)                                  # n < 3
    ident = planted_cluster(rng, 60, 40, R=np.eye(3), t=np.zeros(3)) # identity pose: found, then dropped
    S_eq = np.tile(rng.uniform(-1, 1, (1, 3)).astype(np.float32), (30, 1))
    equal = (S_eq, rng.uniform(-1, 1, (30, 3)).astype(np.float32), np.zeros(30, bool), None, None)     # no good sample
    big = planted_cluster(rng, 5000, 2600)                            # beyond anything LDS-resident: tiles
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, bool), None, None)
    normal = planted_cluster(rng, 120, 70)
    cl = [few, ident, equal, big, empty, normal]
    off, out = run_filter(pkg, gpu, cl)
    assert out["kept"].tolist() == [0, 0, 0, 1, 0, 1]
    assert out["iterations"][0] == 0 and out["iterations"][2] == 0 and out["best_hypothesis"][2] == -1 and out["best_hypothesis"][1] >= 0
    assert not out["inlier"][off[0]:off[3]].any()
    assert np.array_equal(out["inlier"][off[3]:off[4]].astype(bool), big[2]) and out["n_inliers"][3] == 2600
    assert np.array_equal(out["inlier"][off[5]:off[6]].astype(bool), normal[2])
    for c in (0, 1, 2, 4):
        assert np.array_equal(out["transform"][c], np.eye(4, dtype=np.float32))
    r = rr.ransac(big[0], big[1], THR, SEED)
    assert r["kept"] and out["best_hypothesis"][3] == r["best_i"] and out["iterations"][3] == r["iterations"]
    # threshold <= 0: nothing is an inlier -> dropped
    for thr in (0.0, -0.1):
        _, o2 = run_filter(pkg, gpu, [normal], thr=thr)
        assert o2["kept"][0] == 0 and not o2["inlier"].any()
    # same seed: bit-equal; another seed: the planted set again, by another hypothesis sequence
    _, a = run_filter(pkg, gpu, cl, seed=777)
    _, b = run_filter(pkg, gpu, cl, seed=777)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["inlier"][off[5]:off[6]].astype(bool), normal[2]) and np.array_equal(a["inlier"][off[3]:off[4]].astype(bool), big[2])
    assert a["kept"].tolist() == [0, 0, 0, 1, 0, 1]
    # max_iterations caps the sequential loop at i <= max_iterations
    _, c0 = run_filter(pkg, gpu, [normal], max_iterations=0)
    assert c0["iterations"][0] == 1 and c0["best_hypothesis"][0] == 0
    # counters: clusters seen / kept, and the chunks never run fewer hypotheses than the sequential loop needs
    ctx = gpu[0]
    ctx.timers_reset()
    _, o3 = run_filter(pkg, gpu, cl)
    assert ctx.timer("ransac_clusters")[0] == len(cl) and ctx.timer("ransac_clusters_kept")[0] == 2
    assert ctx.timer("ransac_hypotheses_needed")[0] == o3["iterations"].sum()
    assert ctx.timer("ransac_hypotheses_evaluated")[0] >= ctx.timer("ransac_hypotheses_needed")[0]


# ---- the filter inside the maxima search ------------------------------------------------------------------------------------------
H_BW = 0.5          # mean-shift bandwidth h; Hough bins of edge 4 h whose centres are the cluster centres
MIN_VOTES = 6


def _vote_scene(seed=5, pad=17):
    assert pad >= 17
    """8 objects x 3 classes x 2 tight clusters (spread <= 0.3 h, centres >= 4 h apart and in non-adjacent Hough bins). Every cluster's
    votes carry planted inlier / outlier keypoint pairs; per (object, class) the second cluster is, in turn, in the identity pose,
    left with fewer inliers than MinVotesThreshold, or ordinary. Votes of an object are shuffled over its slots, with empty slots."""
    rng = np.random.default_rng(seed)
    prng = np.random.default_rng([seed, 99])               # the slot shuffle draws from its own stream: the votes do not depend on pad
    objs, slot_off = [], [0]
    pos, w, cls, inst, kp, kpt, cid = [], [], [], [], [], [], []
    plan = []
    for o in range(8):
        rows = []
        for c in range(3):
            for j in range(2):
                centre = np.array([-4.0 if j == 0 else 2.0, -4.0 + 2.0 * c, -2.0 + 2.0 * ((o + c) % 3)])
                kind = "normal" if j == 0 else ("identity", "few", "normal")[(o + c) % 3]
                ni = 12 + 2 * (c * 2 + j) + (o % 2)
                no = ni - 3                                        # outliers carry instance 9: more votes than either inlier instance
                if kind == "few":
                    ni, no = 4, 9                                  # 13 votes pass MinVotesThreshold = 6 before the filter, 4 inliers do not after
                R, t = (np.eye(3), np.zeros(3)) if kind == "identity" else (None, None)
                S, T, inl, _, _ = planted_cluster(rng, ni + no, ni, R=R, t=t)
                p = centre + rng.uniform(-0.15 * H_BW, 0.15 * H_BW, (ni + no, 3))
                instv = np.where(inl, np.where(np.arange(ni + no) < (ni * 3) // 5, 5, 2), 9)
                k = len(plan)
                plan.append(dict(o=o, c=c, kind=kind, ni=ni, n=ni + no, centre=centre))
                for i in range(ni + no):
                    rows.append((p[i], 1.0, c, instv[i], T[i], S[i], k, bool(inl[i])))
        for _ in range(17):                                    # empty slots (class -1) among the votes
            rows.append((np.zeros(3), 0.0, -1, -1, np.zeros(3), np.zeros(3), -1, False))
        perm = prng.permutation(len(rows))
        # pad - 17 further empty slots at the object's end: the votes keep their relative order whatever pad is
        for r in [rows[i] for i in perm] + [(np.zeros(3), 0.0, -1, -1, np.zeros(3), np.zeros(3), -1, False)] * (pad - 17):
            pos.append(r[0]); w.append(r[1]); cls.append(r[2]); inst.append(r[3]); kp.append(r[4]); kpt.append(r[5]); cid.append((r[6], r[7]))
        slot_off.append(len(pos))
    return dict(slot_off=np.asarray(slot_off, np.uint32), pos=np.asarray(pos, np.float32), weight=np.asarray(w, np.float32), cls=np.asarray(cls, np.int32),
                inst=np.asarray(inst, np.int32), kp=np.asarray(kp, np.float32), kpt=np.asarray(kpt, np.float32), cluster=np.asarray([c[0] for c in cid]),
                planted_inlier=np.asarray([c[1] for c in cid]), plan=plan)


def _to_dev(sc, dev):
    import torch
    votes = {k: torch.from_numpy(sc[k]).to(dev) for k in ("pos", "weight", "cls", "inst")}
    ransac = dict(vote_keypoint=torch.from_numpy(sc["kp"]).to(dev), vote_keypoint_training=torch.from_numpy(sc["kpt"]).to(dev), inlier_threshold=THR)
    return votes, ransac


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


def _expected_maxima(sc, plain, members_of, kernel_w, thr_of=lambda cls: THR):
    """numpy rebuild of the filtered result from the unfiltered maxima: members -> restatement in slot order -> inlier sums -> the
    Voting::findMaxima tail (stable sort by weight, normalise). members_of(o, m) -> slot indices; kernel_w(o, m, slots) -> float32 weights"""
    exp, n_filter_kept = [], 0
    for o in range(len(sc["slot_off"]) - 1):
        rows = []
        for m in range(plain["n"][o]):
            slots = members_of(o, m)
            wv = kernel_w(o, m, slots)
            if len(slots) < MIN_VOTES:
                continue
            r = rr.ransac(sc["kpt"][slots], sc["kp"][slots], thr_of(int(plain["cls"][o, m])), SEED)
            n_filter_kept += int(r["kept"])
            if not r["kept"] or r["n_inliers"] < MIN_VOTES:
                continue
            keep = slots[r["mask"]]
            wk = wv[r["mask"]]
            tally = {}
            for s, x in zip(keep, wk):
                tally[int(sc["inst"][s])] = tally.get(int(sc["inst"][s]), 0.0) + float(x)
            best_inst = max(sorted(tally), key=lambda i: tally[i])
            rows.append(dict(cls=int(plain["cls"][o, m]), pos=plain["pos"][o, m], w=float(wk.astype(np.float64).sum()), n=len(keep), inst=best_inst,
                             slots=keep))
        exp.append(rows)
    return exp, n_filter_kept


def _check_maxima(got, exp, plain_order_key):
    for o, rows in enumerate(exp):
        # the maxima come out class by class and are then stably sorted by weight (descending)
        rows = sorted(rows, key=plain_order_key)
        order = sorted(range(len(rows)), key=lambda i: -rows[i]["w"])
        tot = sum(r["w"] for r in rows)
        assert got["n"][o] == len(rows), (o, got["n"][o], len(rows))
        for k, i in enumerate(order):
            r = rows[i]
            assert got["cls"][o, k] == r["cls"] and got["inst"][o, k] == r["inst"] and got["n_votes"][o, k] == r["n"], (o, k)
            assert abs(got["weight"][o, k] - r["w"] / tot) < 1e-4, (o, k, got["weight"][o, k], r["w"] / tot)
            assert np.array_equal(got["pos"][o, k], r["pos"]), (o, k)


@pytest.mark.parametrize("kernel", ["uniform", "gaussian"])
def test_filter_inside_find_maxima(pkg, gpu, kernel):
    ctx, dev = gpu
    capi = pkg.capi
    sc = _vote_scene()
    votes, ransac = _to_dev(sc, dev)
    kw = dict(kernel=capi.KERNEL_UNIFORM if kernel == "uniform" else capi.KERNEL_GAUSSIAN, min_votes_threshold=MIN_VOTES, max_maxima=16)
    plain = _np(capi.find_maxima(ctx, sc["slot_off"], votes, 3, H_BW, **kw))
    votes, ransac = _to_dev(sc, dev)                                 # find_maxima reweights nothing in the caller's arrays; fresh copies anyway
    ctx.timers_reset()
    got = _np(capi.find_maxima(ctx, sc["slot_off"], votes, 3, H_BW, ransac=ransac, **kw))
    ctx.sync()
    assert (plain["n"] == 6).all()                                   # one maximum per planted cluster before the filter
    h = np.float32(H_BW); h2 = np.float32(float(h) * float(h)); hh = h * h

    def d2_to(o, m, slots):
        p = plain["pos"][o, m]; v = sc["pos"][slots]
        r = np.zeros(len(slots), np.float32)
        for a in range(3):
            d = v[:, a] - p[a]; r = r + d * d
        return r

    def members_of(o, m):
        s = np.arange(sc["slot_off"][o], sc["slot_off"][o + 1])
        s = s[sc["cls"][s] == plain["cls"][o, m]]
        d2 = d2_to(o, m, s)
        assert (np.abs(np.sqrt(d2.astype(np.float64)) - H_BW) > 1e-5 * H_BW).all()     # no vote on the edge of the radius h
        return s[d2 < h2]

    def kernel_w(o, m, slots):
        if kernel == "uniform":
            return sc["weight"][slots]
        return (np.exp(np.float32(-0.5) * (d2_to(o, m, slots) / hh)).astype(np.float32) * sc["weight"][slots]).astype(np.float32)

    exp, n_filter_kept = _expected_maxima(sc, plain, members_of, kernel_w)
    _check_maxima(got, exp, lambda r: r["cls"])
    # the planted design: identity-pose and under-threshold clusters are gone, every other maximum holds exactly its planted inliers
    n_normal = {o: sum(1 for p in sc["plan"] if p["o"] == o and p["kind"] == "normal") for o in range(8)}
    for o, rows in enumerate(exp):
        assert len(rows) == n_normal[o]
        for r in rows:
            assert sc["planted_inlier"][r["slots"]].all()
            k = sc["cluster"][r["slots"][0]]
            assert r["n"] == sc["plan"][k]["ni"] and r["inst"] == 5           # unfiltered, instance 9 (the outliers) would win
            if kernel == "uniform":
                assert r["w"] == r["n"]
    assert ctx.timer("ransac_clusters")[0] == 48 and ctx.timer("ransac_clusters_kept")[0] == n_filter_kept
    assert n_filter_kept >= sum(len(r) for r in exp)                 # the under-threshold clusters pass the filter and fail MinVotesThreshold after it
    # the transforms of the surviving maxima are rigid motions, none the identity
    tf = got["transform"]
    for o in range(8):
        for k in range(got["n"][o]):
            Rm = tf[o, k, :3, :3].astype(np.float64)
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-5 and np.linalg.det(Rm) > 0.999 and not np.allclose(tf[o, k], np.eye(4), atol=1e-3)


def test_filter_inside_hough3d_maxima(pkg, gpu):
    ctx, dev = gpu
    capi = pkg.capi
    sc = _vote_scene()
    votes, ransac = _to_dev(sc, dev)
    kw = dict(use_interpolation=False, rel_threshold=0.01, min_votes_threshold=MIN_VOTES, max_maxima=16)
    plain = _np(capi.hough3d_maxima(ctx, sc["slot_off"], votes, 3, 4 * H_BW, **kw))
    got = _np(capi.hough3d_maxima(ctx, sc["slot_off"], votes, 3, 4 * H_BW, ransac=ransac, **kw))
    ctx.sync()
    assert (plain["n"] == 6).all()

    def members_of(o, m):
        s = np.arange(sc["slot_off"][o], sc["slot_off"][o + 1])
        s = s[sc["cls"][s] == plain["cls"][o, m]]
        s = s[(np.floor((sc["pos"][s].astype(np.float64) + 5.0) / (4 * H_BW)) == np.floor((plain["pos"][o, m].astype(np.float64) + 5.0) / (4 * H_BW))).all(1)]
        assert len(s) == plain["n_votes"][o, m]
        return s

    exp, _ = _expected_maxima(sc, plain, members_of, lambda o, m, slots: sc["weight"][slots])
    _check_maxima(got, exp, lambda r: r["cls"])
    assert sum(len(r) for r in exp) == sum(1 for p in sc["plan"] if p["kind"] == "normal")


def test_vote_keypoints_match_a_numpy_gather(pkg, gpu):
    import torch
    ctx, dev = gpu
    capi = pkg.capi
    rng = np.random.default_rng(9)
    nw, dim, nq, k = 40, 8, 25, 3
    nv = rng.integers(0, 4, nw); nv[0] = 3
    voff = np.concatenate([[0], np.cumsum(nv)]).astype(np.uint32)
    n_votes = int(voff[-1])
    cb = capi.Codebook(ctx, rng.normal(size=(nw, dim)).astype(np.float32), voff, rng.normal(size=(n_votes, 3)).astype(np.float32),
                       rng.integers(0, 2, n_votes).astype(np.uint32), np.arange(n_votes, dtype=np.uint32), 2, np.ones(2, np.float32))
    wkp = rng.normal(size=(nw, 3)).astype(np.float32)
    kxyz = rng.normal(size=(nq, 3)).astype(np.float32)
    kx, ky, kz = (torch.from_numpy(np.ascontiguousarray(kxyz[:, a])).to(dev) for a in range(3))
    idx = rng.integers(-1, nw, (nq, k)).astype(np.int32)
    with pytest.raises(capi.IsmHipError):                            # no training keypoints yet
        capi.vote_keypoints(ctx, cb, kx, ky, kz, torch.from_numpy(idx).to(dev))
    cb.set_word_keypoint(wkp)
    maxv = cb.max_votes

    def gather(feat, words):
        a = np.zeros((len(words) * maxv, 3), np.float32); b = np.zeros_like(a)
        for t, (f, c) in enumerate(zip(feat, words)):
            if c >= 0:
                a[t * maxv:t * maxv + nv[c]] = kxyz[f]; b[t * maxv:t * maxv + nv[c]] = wkp[c]
        return a, b
    vkp, vkpt = capi.vote_keypoints(ctx, cb, kx, ky, kz, torch.from_numpy(idx).to(dev))
    ea, eb = gather(np.repeat(np.arange(nq), k), idx.ravel())
    assert np.array_equal(vkp.cpu().numpy(), ea) and np.array_equal(vkpt.cpu().numpy(), eb)
    cnt = rng.integers(0, 5, nq)
    aoff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    aidx = rng.integers(0, nw, int(aoff[-1])).astype(np.int32)
    vkp, vkpt = capi.vote_keypoints_csr(ctx, cb, kx, ky, kz, aoff, torch.from_numpy(aidx).to(dev))
    ea, eb = gather(np.repeat(np.arange(nq), cnt), aidx)
    assert np.array_equal(vkp.cpu().numpy(), ea) and np.array_equal(vkpt.cpu().numpy(), eb)
    cb.close()


# ---- through the layers -----------------------------------------------------------------------------------------------------------
def _host_counter(m, name):
    v = C.c_double(0.0)
    assert m.L.ism3d_device_timer(m.h, name.encode(), C.byref(v)) == 0
    return v.value


def _host_detect_keypoints(m):
    """the keypoints the host's last detectBatch() kept, per object: (kp_off [n_obj+1], kp [n, 3])"""
    dim, n_obj = C.c_int(), C.c_int()
    n = m.L.ism3d_last_features(m.h, 1, C.byref(dim), C.byref(n_obj), None, None, None, None, None, None, None)
    assert n > 0
    off = np.zeros(n_obj.value + 1, np.uint32); kxyz = np.zeros((n, 3), np.float32)
    assert m.L.ism3d_last_features(m.h, 1, None, None, C.c_void_p(off.ctypes.data), None, None, C.c_void_p(kxyz.ctypes.data), None, None, None) == n
    return off, kxyz


def _host_cfg(**voting):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Voting"]["Parameters"].update(voting)
    return json.dumps(j)


def _rotated_batch(pkg, test, indices, seed=11):
    rng = np.random.default_rng(seed)
    objs = []
    for i in indices:
        o = test.get(i)
        R = _rot(rng).astype(np.float32)
        xyz = np.ascontiguousarray((o["xyz"] @ R.T).astype(np.float32)); nrm = np.ascontiguousarray((o["normals"] @ R.T).astype(np.float32))
        objs.append(dict(xyz=xyz, normals=nrm, kp=pkg.synthetic.voxel_grid(xyz, 0.2), label=o["label"]))
    pt_off = np.concatenate([[0], np.cumsum([len(o["xyz"]) for o in objs])]).astype(np.uint32)
    kp_off = np.concatenate([[0], np.cumsum([len(o["kp"]) for o in objs])]).astype(np.uint32)
    return dict(pt_off=pt_off, kp_off=kp_off, xyz=np.concatenate([o["xyz"] for o in objs]), normals=np.concatenate([o["normals"] for o in objs]),
                kp=np.concatenate([o["kp"] for o in objs]), labels=np.array([o["label"] for o in objs], np.int32))


@pytest.mark.parametrize("voting", ["MeanShift", "Hough3D"])
def test_host_and_python_harness_agree_with_ransac_vote_filtering(pkg, gpu, voting):
    ctx, dev = gpu
    syn = pkg.synthetic
    train = syn.Dataset(3, 9, split=0, n_points=4096, leaf=0.2); test = syn.Dataset(3, 6, split=1, n_points=4096, leaf=0.2)
    order = sorted(range(9), key=lambda i: (train.label(i), i))
    nb = _rotated_batch(pkg, test, range(6))
    results = {}
    for on in (True, False):
        vp = {"MinThreshold": 0.0, "MinVotesThreshold": 1, "BestK": -1, "Bandwidth": 0.6, "RansacInlierThreshold": 0.15}
        kw = dict(n_classes=3, max_maxima=16, voting=voting, ransac_inlier_threshold=0.15)
        if on:
            vp["RansacVoteFiltering"] = True; kw["ransac_vote_filtering"] = True
        j = json.loads(_host_cfg(**vp))
        if voting == "Hough3D":
            j["Children"]["Voting"]["Type"] = "Hough3D"
            j["Children"]["Voting"]["Parameters"].update(BinSize=[0.6, 0.6, 0.6], RelThreshold=0.3)
            kw.update(hough_bin_size=0.6, hough_rel_threshold=0.3)
        m = hb.Model()
        m.config_from_json(json.dumps(j))
        for i in order:
            o = train.get(i)
            m.add_training(o["xyz"], o["normals"], o["label"], i)
        m.train()
        # The filter compares d^2 with thr^2, so the two sides must see the SAME keypoints, not keypoints equal to 1e-7 (the host's
        # voxel grid runs on the device, the harness's in numpy): the harness takes the host's codebook (training keypoints included)
        # and describes the keypoints the host's detectBatch() kept.
        rec = pkg.pipeline.Recognizer(ctx, pkg.pipeline.IsmConfig(**kw))
        cbh = m.codebook_all()
        rec.load_codebook({k: cbh[k] for k in ("words", "vote_offsets", "vote_xyz", "vote_class", "vote_instance", "class_sigma", "word_weight",
                                               "vote_weight", "vote_class_weight", "word_class", "word_keypoint")})
        ctx.timers_reset()
        got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16)
        kp_off, kp = _host_detect_keypoints(m)
        want = rec.detect(pkg.pipeline.DeviceBatch(dict(nb, kp_off=kp_off, kp=kp), dev))
        ctx.sync()
        assert np.array_equal(want["_keep"][0]["off"], kp_off)           # every keypoint the host kept is kept again
        wn = want["n"].cpu().numpy()
        assert np.array_equal(got["n_total"], wn), (got["n_total"], wn)
        for o in range(6):
            k = int(wn[o])
            assert np.array_equal(got["cls"][o, :k], want["cls"][o, :k].cpu().numpy())
            np.testing.assert_allclose(got["weight"][o, :k], want["weight"][o, :k].cpu().numpy(), atol=1e-4)
            assert np.array_equal(got["n_votes"][o, :k], want["n_votes"][o, :k].cpu().numpy())
        clusters = (_host_counter(m, "ransac_clusters"), ctx.timer("ransac_clusters")[0])
        if on:
            assert clusters[0] > 0 and clusters[0] == clusters[1]
            assert "transform" in want
        else:                                                        # key absent: the entry points of before, no filter anywhere
            assert clusters == (0.0, 0.0) and "transform" not in want
        results[on] = (wn.copy(), want["n_votes"].cpu().numpy().copy())
        m.close()
    # the filter only ever removes votes and maxima
    assert results[True][0].sum() <= results[False][0].sum() and results[True][0].sum() > 0


# ---- per-class thresholds, and objects beyond the LDS-resident size -------------------------------------------------------------------
def _uniform_members(sc, plain):
    h = np.float32(H_BW); h2 = np.float32(float(h) * float(h))

    def members_of(o, m):
        s = np.arange(sc["slot_off"][o], sc["slot_off"][o + 1])
        s = s[sc["cls"][s] == plain["cls"][o, m]]
        r = np.zeros(len(s), np.float32)
        for a in range(3):
            d = sc["pos"][s][:, a] - plain["pos"][o, m][a]; r = r + d * d
        return s[r < h2]
    return members_of


def test_per_class_inlier_thresholds_reach_the_right_class(pkg, gpu):
    """class 0 keeps the scene's threshold, class 1 gets 0 (every cluster dropped), class 2 thirty times as much (outliers 10 .. 20
    thresholds away become inliers): a threshold read for the wrong class changes the integer answer. The scalar is a decoy."""
    ctx, dev = gpu
    capi = pkg.capi
    sc = _vote_scene()
    votes, ransac = _to_dev(sc, dev)
    cthr = np.array([THR, 0.0, 30 * THR], np.float32)
    ransac.update(inlier_threshold=-1.0, class_inlier_threshold=cthr)
    kw = dict(kernel=capi.KERNEL_UNIFORM, min_votes_threshold=MIN_VOTES, max_maxima=16)
    plain = _np(capi.find_maxima(ctx, sc["slot_off"], votes, 3, H_BW, **kw))
    got = _np(capi.find_maxima(ctx, sc["slot_off"], votes, 3, H_BW, ransac=ransac, **kw))
    ctx.sync()
    exp, _ = _expected_maxima(sc, plain, _uniform_members(sc, plain), lambda o, m, slots: sc["weight"][slots], thr_of=lambda c: float(cthr[c]))
    _check_maxima(got, exp, lambda r: r["cls"])
    for o, rows in enumerate(exp):
        assert not any(r["cls"] == 1 for r in rows) and any(r["cls"] == 0 for r in rows)
        for r in rows:
            k = sc["cluster"][r["slots"][0]]
            if r["cls"] == 0:
                assert r["n"] == sc["plan"][k]["ni"]
            else:
                assert r["n"] > sc["plan"][k]["ni"]                  # the wide threshold takes outliers in


@pytest.mark.parametrize("voting", ["meanshift", "hough3d"])
def test_filter_on_objects_with_more_slots_than_fit_lds(pkg, gpu, voting):
    """the same scene with 2 100 empty slots per object (> 2 048: the vote arrays of the maxima kernels live in the HBM workspace):
    identical maxima, in the same order, as the LDS-resident kernels give on the small scene"""
    ctx, dev = gpu
    capi = pkg.capi
    res = []
    for pad in (17, 2100):
        sc = _vote_scene(pad=pad)
        assert (np.diff(sc["slot_off"].astype(np.int64)) > 2048).all() == (pad > 17)
        votes, ransac = _to_dev(sc, dev)
        if voting == "meanshift":
            got = capi.find_maxima(ctx, sc["slot_off"], votes, 3, H_BW, kernel=capi.KERNEL_GAUSSIAN, min_votes_threshold=MIN_VOTES, max_maxima=16, ransac=ransac)
        else:
            got = capi.hough3d_maxima(ctx, sc["slot_off"], votes, 3, 4 * H_BW, use_interpolation=False, rel_threshold=0.01, min_votes_threshold=MIN_VOTES,
                                      max_maxima=16, ransac=ransac)
        ctx.sync()
        res.append(_np(got))
    a, b = res
    assert a["n"].sum() == 32 and np.array_equal(a["n"], b["n"])
    for k in ("cls", "inst", "n_votes", "pos", "transform"):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(a["weight"], b["weight"], atol=1e-6)
