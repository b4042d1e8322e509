"""Inputs that fix every activation of the codebook stage, built to sit on its decisions (train.hip, k_cast_votes in
codebook.hip). A training scene is a dict of the arguments of codebook_ref.train_from_lists / capi.train_activate_lists (no kNN
between the input and the code under test) with `pins`, one line on what it holds still. scene(name) and reference(name) are
cached; test_codebook_cpu.py proves both before test_gpu_codebook.py runs the device on them."""
import functools

import numpy as np

import codebook_ref as cr

f32 = np.float32
RANKS_M = (1, 2, 3, 4, 63, 64, 65, 127, 128, 2047, 2048, 2049)       # TR_MAXM = 2048 of train.hip: 2049 takes k_tr_weights_big
HUB_M = 32768                                                        # TR_MAXM_BIG: the last size built
SIGMA_DIMS = (1, 3, 33, 35, 64, 352)
CSR_WORDS = (1023, 1024, 1025, 2049)
CENTRE = np.array([0.25, 0.5, -0.125], f32)
IDENTITY = np.eye(3, dtype=f32).reshape(9)


def lattice_rows(n):
    """n distinct rows of dim 4 with small integer entries: a feature that copies row w has functor value 0 to it and >= 1 to others"""
    w = np.arange(n)
    return np.stack([w % 64, (w // 64) % 64, w // 4096, np.ones(n)], 1).astype(f32)


def line_positions(m, extent=1.2):
    """m keypoint abscissae p_j = h (j + c j^2), h = extent / m, c = 1.6 / m^2. From vote i the neighbour t places to the right lies
    2 h c t^2 further than the one t places to the left: between 0.2 h and 0.8 h for the t in [m/4, m/2] a median can fall on, so no two
    weights near a median are closer than 0.2 h in distance, while a uniform line would make them equal in pairs."""
    j = np.arange(m, dtype=np.float64)
    return ((extent / m) * (j + (1.6 / m ** 2) * j * j)).astype(f32)


def one_word_each(word_of_feature, n_words, kp, lrf=None, centre=None, cls=None, model=None, n_classes=1, pins=""):
    """every feature activates exactly one codeword: its descriptor is a copy of that codeword's row, so the CPU oracle's own k = 1
    search reproduces the activation and the scene can be given to ora.activate"""
    word_of_feature = np.asarray(word_of_feature, np.int64)
    n = len(word_of_feature)
    cw = lattice_rows(n_words)
    return dict(metric=0, desc=cw[word_of_feature].copy(), codewords=cw, kp=np.asarray(kp, f32),
                lrf=np.tile(IDENTITY, (n, 1)) if lrf is None else np.asarray(lrf, f32).reshape(n, 9),
                centre=np.tile(CENTRE, (n, 1)) if centre is None else np.asarray(centre, f32),
                cls=np.zeros(n, np.uint32) if cls is None else np.asarray(cls, np.uint32),
                model=np.zeros(n, np.uint32) if model is None else np.asarray(model, np.uint32),
                act_off=np.arange(n + 1, dtype=np.int64), act_idx=word_of_feature.astype(np.int32), n_classes=n_classes,
                oracle_k1=True, pins=pins)


def on_the_line(ms, extent=1.2):
    word = np.concatenate([np.full(m, e) for e, m in enumerate(ms)])
    x = np.concatenate([line_positions(m, extent) for m in ms])
    return word, np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)


def ranks():
    word, kp = on_the_line(RANKS_M)
    return one_word_each(word, len(RANKS_M), kp, cls=word, model=np.arange(len(word)) // 64, n_classes=len(RANKS_M),
                         pins="median ranks of words with 1 .. 2049 votes: m == 1, even, odd, the 64-lane stride, and TR_MAXM = 2048 between "
                              "the wave kernel and k_tr_weights_big; identity frames, one centre, one class per word")


def ties():
    """(word, keypoints): coincident keypoints (every weight 1), an equilateral triangle and a regular tetrahedron (every weight but
    the vote's own equal), two far clusters (weights underflow to exactly 0.0f: e^-144), a 2^-16 line (weights round to exactly 1.0f)"""
    groups = [np.zeros((4, 3)), np.zeros((5, 3)),
              np.array([[0, 0, 0], [0.5, 0, 0], [0.25, 0.4330127, 0]]),
              np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) * 0.125,
              np.array([[0, 0, 0], [0, 0, 0], [6, 0, 0], [6, 0, 0]]), np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 6, 0], [0, 6, 0]]),
              np.array([[0, 0, 6]] * 1 + [[0, 0, 0]] * 2),
              np.arange(4)[:, None] * np.array([[2.0 ** -16, 0, 0]]), np.arange(5)[:, None] * np.array([[0, 2.0 ** -16, 0]])]
    word = np.concatenate([np.full(len(g), e) for e, g in enumerate(groups)])
    s = one_word_each(word, len(groups), np.concatenate(groups), pins="medians among equal weights, weights of exactly 0.0f and exactly "
                      "1.0f, even and odd m: the bisection must return the tied value itself")
    s["groups"] = [len(g) for g in groups]
    return s


def hub(m=HUB_M):
    word, kp = on_the_line((m,))
    s = one_word_each(word, 2, kp, model=np.arange(m) // 256, pins=f"one word with {m} votes: TR_MAXM_BIG = 32768 is the last size "
                      "built, 32769 is refused")
    s["oracle_k1"] = False          # the oracle evaluates all m^2 weights and cannot sample
    return s


def signed_permutations():
    """the 24 proper (det +1) signed permutation matrices: traces 3, 1, 0 and -1 and every tie of the diagonal"""
    out = []
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    m = np.zeros((3, 3))
                    for r, (c, s) in enumerate(zip(p, (sx, sy, sz))):
                        m[r, c] = s
                    if round(np.linalg.det(m)) == 1:
                        out.append(m)
    assert len(out) == 24
    return out


def small_rotation(rng, angle):
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * k @ k


def frame_list():
    """24 signed permutations, then 48 rotations within 1e-3 of a tie: of trace 0 (the 120-degree turns, whose diagonal is all equal
    too) and of m00 == m11 at trace -1 (half turns about a face diagonal)"""
    rng = np.random.default_rng(7)
    perms = signed_permutations()
    near = []
    t0 = [m for m in perms if np.trace(m) == 0]
    half = [m for m in perms if np.trace(m) == -1 and np.count_nonzero(np.diag(m)) == 1]
    for i in range(32):
        near.append(t0[i % len(t0)] @ small_rotation(rng, rng.uniform(1e-6, 1e-3)))
    for i in range(16):
        near.append(half[i % len(half)] @ small_rotation(rng, rng.uniform(1e-6, 1e-3)))
    return np.stack(perms + near).astype(f32).reshape(-1, 9), len(perms)


def frames():
    lrf, n_exact = frame_list()
    n = len(lrf)
    rng = np.random.default_rng(8)
    kp = (rng.integers(-64, 65, (n, 3)) / 64.0).astype(f32)                      # dyadic: centre - kp is exact in float32
    centre = np.tile(np.array([0.5, -0.25, 0.125], f32), (n, 1))
    s = one_word_each(np.arange(n) // 6, n // 6, kp, lrf=lrf, centre=centre, pins="rot_quaternion: trace > 0 strict (120-degree turns "
                      "have trace exactly 0), strict diagonal comparisons (ties go to i = 0), rotations within 1e-3 of each tie on "
                      "both sides; words of 6 votes mix the frames in rotateBack")
    s["n_permutations"] = n_exact
    return s


def sigma(metric, dim, seed=5):
    """classes (size: lists / models): 0 (1: one list of 2), 1 (3: lists 0, 3, ..; single-feature models), 2 (4: lists 1, 0, 5; the
    first model has 3 features, more than the sample of 2), 3 (15: lists of 1; single-feature models), 4 (16: lists 3, 2: the word
    sample stops after the second feature with 5 > 4 words; models of 2), 5 (17: first list 4 = the whole sample; models of 3),
    6 (empty), 7 (4: every list empty -> -0.0), 8 (1: one list of 1 -> one distance -> 0 / 0)"""
    rng = np.random.default_rng(seed + 31 * dim + metric)
    sizes = [1, 3, 4, 15, 16, 17, 0, 4, 1]
    lead = {0: [2], 1: [0, 3], 2: [1, 0, 5], 3: [1] * 15, 4: [3, 2], 5: [4], 7: [0, 0, 0, 0], 8: [1]}
    models = {0: 1, 1: 1, 2: 3, 3: 1, 4: 2, 5: 3, 7: 2, 8: 1}
    cls, model, lens = [], [], []
    for c, nc in enumerate(sizes):
        ln = list(lead.get(c, []))[:nc]
        ln += list(rng.integers(0, 6, nc - len(ln)))
        lens += ln; cls += [c] * nc
        model += [c * 100 + i // models.get(c, 1) for i in range(nc)]
    n = len(cls)
    ncw = 40
    desc = rng.random((n, dim)).astype(f32); cw = rng.random((ncw, dim)).astype(f32)
    if dim >= 3:                                                     # chi-square: columns where x + y == 0, and single zero entries
        desc[:, 1::3] = 0; cw[:, 1::3] = 0
        desc[::2, 0] = 0
    else:
        desc[::3] = 0; cw[::4] = 0
    act_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    act_idx = rng.integers(0, ncw, act_off[-1]).astype(np.int32)
    kp = (rng.integers(-64, 65, (n, 3)) / 64.0).astype(f32)
    lrf = frame_list()[0][rng.integers(0, 24, n)]
    return dict(metric=metric, desc=desc, codewords=cw, kp=kp, lrf=lrf, centre=np.tile(CENTRE, (n, 1)), cls=np.asarray(cls, np.uint32),
                model=np.asarray(model, np.uint32), act_off=act_off, act_idx=act_idx, n_classes=len(sizes), oracle_k1=False,
                pins="the sigma^2 sample: int(sqrt(n_c)) at 1, 3, 4, 15, 16, 17, the word count checked before each whole list, features "
                     "in whole models, an empty class, empty sampled lists (-0.0), one distance (NaN); wave_functor at this dim")


def csr(n_codewords, seed=3):
    rng = np.random.default_rng(seed + n_codewords)
    pool = np.unique(np.concatenate([[0, 1, 2, 511, 1021, 1022, n_codewords - 2, n_codewords - 1], rng.integers(0, n_codewords, 12)]))
    lens = [0, 0, 3, 1, 0, 0, 0, 2, 4, 1, 0, 0, 0, 5, 2, 1, 3, 0, 2, 1, 4, 0, 0, 0, 2, 3, 1, 2, 0, 0]       # empty at both ends, runs of three
    n = len(lens)
    act_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    act_idx = rng.choice(pool, act_off[-1]).astype(np.int32)
    act_idx[act_off[8]:act_off[8] + 2] = pool[len(pool) // 2]                      # feature 8 activates the same word twice: two votes
    act_idx[act_off[2]] = 0; act_idx[act_off[25]] = n_codewords - 1                 # the first and the last word are used
    dim = 8
    cls = (np.arange(n) >= 14).astype(np.uint32)
    return dict(metric=0, desc=rng.random((n, dim)).astype(f32), codewords=rng.random((n_codewords, dim)).astype(f32),
                kp=(rng.integers(-64, 65, (n, 3)) / 64.0).astype(f32), lrf=frame_list()[0][rng.integers(0, 72, n)],
                centre=np.tile(CENTRE, (n, 1)), cls=cls, model=(np.arange(n) // 5).astype(np.uint32), act_off=act_off, act_idx=act_idx,
                n_classes=2, oracle_k1=False,
                pins=f"the CSR build over {n_codewords} codewords: the scan's carry across 1024-entry blocks, empty lists at both ends and in "
                     "runs of three (the binary search of k_tr_votes), a feature that activates one word twice")


def term3():
    """classes 0, 1, 2 over words 0..3; the LAST word of every class holds another share of it than the first and than the largest"""
    words = [0, 0, 0, 1, 3, 3] + [0, 1, 1, 2] + [1, 2, 2, 2, 3]
    cls = [0] * 6 + [1] * 4 + [2] * 5
    n = len(words)
    rng = np.random.default_rng(12)
    return one_word_each(words, 4, (rng.integers(-64, 65, (n, 3)) / 64.0).astype(f32), cls=cls, model=np.arange(n) // 2, n_classes=3,
                         pins="m_term3 is keyed by class: the last word holding the class wins, not the first and not the largest")


def cleanup():
    """through train_activate (k = 1, clean-up on), codewords = the features: class 0 has distinct descriptors (words of one vote, kept),
    class 1 consists of three pairs and a triple of equal descriptors: the lowest row of each gets 2 or 3 votes, the others 0, all dropped"""
    cw = lattice_rows(16)
    rows = [0, 1, 2, 3, 4] + [5, 5, 6, 6, 7, 7, 8, 8, 8]
    n = len(rows)
    rng = np.random.default_rng(13)
    return dict(metric=0, desc=cw[rows].copy(), codewords=None, kp=(rng.integers(-64, 65, (n, 3)) / 64.0).astype(f32),
                lrf=frame_list()[0][:n], centre=np.tile(CENTRE, (n, 1)), cls=np.asarray([0] * 5 + [1] * 9, np.uint32),
                model=(np.arange(n) // 3).astype(np.uint32), n_classes=2, k=1, clean_up=True,
                act_off=np.arange(n + 1, dtype=np.int64), act_idx=np.asarray([0, 1, 2, 3, 4, 5, 5, 7, 7, 9, 9, 11, 11, 11], np.int32),
                oracle_k1=True, pins="the K = 1 clean-up keeps words with exactly one vote and drops 0, 2 and 3; every vote of class 1 is cleaned away")


def _named():
    out = dict(ranks=ranks, ties=ties, hub=hub, frames=frames, term3=term3, cleanup=cleanup)
    for metric in (0, 1):
        for dim in SIGMA_DIMS:
            out[f"sigma-{'chi2' if metric else 'l2'}-{dim}"] = functools.partial(sigma, metric, dim)
    out["sigma-l2-1344"] = functools.partial(sigma, 0, 1344)
    for ncw in CSR_WORDS:
        out[f"csr-{ncw}"] = functools.partial(csr, ncw)
    return out


SCENES = _named()
TRAIN_ARGS = ("metric", "desc", "lrf", "kp", "cls", "model", "centre", "act_off", "act_idx", "n_classes")


@functools.lru_cache(maxsize=None)
def scene(name):
    s = SCENES[name]()
    assert s["pins"]
    return s


@functools.lru_cache(maxsize=None)
def reference(name):
    s = scene(name)
    return cr.train_from_lists(*[s[k] for k in TRAIN_ARGS], codewords=s["codewords"], clean_up=s.get("clean_up", False))


# ----------------------------------------------------------------------------------------------------------- vote casting
def votes_edges():
    """a codebook of 6 words (0 and 5 without votes, word 1 with max_votes = 4 votes of classes 0, 1, 2 and 5 >= n_classes) and a CSR of
    activations whose functor values sit on, one float above and one float below 2 sigma of every class. class_sigma = [0.5, NaN, 0.25].
    Features 0..9 hold the boundary cases under a mix of frames; features 10..33 hold the 24 signed permutations and cast live votes,
    whose bbox quaternion b * q carries the SIGN of q: that is what tells `trace > 0` and the strict diagonal comparisons from lax ones
    (the rotated position cannot)."""
    up = lambda x: np.nextafter(f32(x), f32(np.inf)); dn = lambda x: np.nextafter(f32(x), f32(-np.inf))
    eps = f32(cr.FLT_EPSILON)
    vote_offsets = np.array([0, 0, 4, 5, 6, 8, 8], np.uint32)
    rng = np.random.default_rng(17)
    bq = rng.integers(-4, 5, (8, 4)) / 4.0
    bq[np.abs(bq).sum(1) == 0] = [1, 0, 0, 0]
    cb = dict(words=lattice_rows(6), vote_offsets=vote_offsets, vote_xyz=(rng.integers(-32, 33, (8, 3)) / 32.0).astype(f32),
              vote_class=np.array([0, 1, 2, 5, 0, 0, 2, 0], np.uint32), vote_instance=np.array([3, 1, 4, 1, 5, 9, 2, 6], np.uint32),
              class_sigma=np.array([0.5, np.nan, 0.25], f32), n_classes=3,
              word_weight=np.array([1, 2, 0.5, 1, 1.5, 1], f32),
              vote_weight=np.array([0.5, 0.75, 1.0, 0.25, eps, dn(eps), 1.0, 0.5], f32),
              vote_class_weight=np.array([0.5, 0.25, 1.0, 0.125, 1.0, 1.0, 0.75, 1.0], f32),
              vote_bbox_quat=bq.astype(f32), vote_bbox_size=(rng.integers(1, 9, (8, 3)) / 8.0).astype(f32))
    lists = [[],
             [(1, 1.0), (1, up(1.0)), (1, dn(1.0))],
             [(1, 0.5), (1, up(0.5)), (1, dn(0.5)), (0, 0.125)],
             [], [], [],
             [(1, 2.0), (1, up(2.0)), (1, dn(2.0)), (-1, 0.25), (6, 0.25)],
             [(2, 0.125), (3, 0.125), (4, -1.0), (5, 0.25)],
             [(1, 0.0), (4, dn(0.5))],
             []]
    lists += [[(4, 0.125)] for _ in range(24)] + [[]]                         # every signed permutation casts the two votes of word 4
    lrf_all, _ = frame_list()
    pick = [0, 5, 9, 13, 23, 24, 31, 40, 57, 71] + list(range(24)) + [30]      # features 10..33: the 24 permutations, each with a live vote
    nq = len(lists)
    kp = (rng.integers(-64, 65, (nq, 3)) / 64.0).astype(f32)
    act_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    idx = np.array([w for l in lists for w, _ in l], np.int32)
    dist = np.array([d for l in lists for _, d in l], f32)
    k = max(len(l) for l in lists)
    didx = np.full((nq, k), -1, np.int32); ddist = np.zeros((nq, k), f32)
    for f, l in enumerate(lists):
        for j, (w, d) in enumerate(l):
            didx[f, j] = w; ddist[f, j] = d
    return dict(cb=cb, lrf=lrf_all[pick], kp=kp, act_off=act_off, idx=idx, dist=dist, feat_of_act=np.repeat(np.arange(nq), np.diff(act_off)),
                dense_idx=didx, dense_dist=ddist, n_words=6,
                pins="|d| > 2 sigma and weight < FLT_EPSILON exactly on, one float above and one float below the boundary; a class id >= "
                     "n_classes (sigma 1), a NaN sigma (kept, NaN matching weight), idx -1 and n_words, words without votes and with "
                     "max_votes, empty CSR lists at both ends and in a run, all 16 flag values; the sign of rot_quaternion at every signed "
                     "permutation (trace exactly 0, ties of the diagonal) through the bbox quaternion")


@functools.lru_cache(maxsize=None)
def votes_scene():
    return votes_edges()


@functools.lru_cache(maxsize=None)
def votes_reference(flags):
    s = votes_scene()
    return cr.cast_votes_ref(s["cb"], flags, s["lrf"], s["kp"], s["feat_of_act"], s["idx"], s["dist"])


def dense_slots(s):
    """slot of CSR activation a, vote v in the dense [nq, k] layout of cast_votes"""
    maxv = int(np.diff(s["cb"]["vote_offsets"].astype(np.int64)).max())
    k = s["dense_idx"].shape[1]
    a = np.arange(len(s["idx"]))
    f = s["feat_of_act"]; j = a - s["act_off"][f]
    return ((f * k + j)[:, None] * maxv + np.arange(maxv)[None, :]).reshape(-1)
