"""Deterministic vote scenes for the maxima tests (test_maxima_cpu.py proves what each one reaches, test_gpu_maxima.py runs them on
the device). No GPU import. A scene is (slot_offsets uint32 [n_obj + 1], votes) with votes = dict(pos [n, 3], weight, cls, inst,
bbox_size [n, 3] and, where needed, bbox_quat [n, 4]) by vote slot; cls -1 marks a slot without a vote.

The exact scenes use dyadic numbers only (weights in 64ths, Hough bins 0.125 / 0.25 / 0.5 on dyadic corners, offsets from the bin
centres in quarter bins, the uniform mean-shift kernel), so that every sum is exact in the oracle's float / double and in the
kernel's fixed point alike and a tie is a tie on both sides."""
import numpy as np

import maxima_model as mm

f32 = np.float32


def pack(pos, w, cls, inst, bs=None, quat=None):
    n = len(w)
    v = dict(pos=np.asarray(pos, f32).reshape(n, 3), weight=np.asarray(w, f32), cls=np.asarray(cls, np.int32), inst=np.asarray(inst, np.int32),
             bbox_size=np.asarray(bs, f32).reshape(n, 3) if bs is not None else (1 + (np.arange(n * 3) % 4) / 4).astype(f32).reshape(n, 3))
    if quat is not None:
        v["bbox_quat"] = np.asarray(quat, f32).reshape(n, 4)
    return v


def concat(scenes):
    """several (off, votes) one after the other as further objects of one call"""
    off = [0]
    for o, _ in scenes:
        off += (np.asarray(o, np.int64)[1:] + off[-1]).tolist()
    keys = scenes[0][1].keys()
    return np.asarray(off, np.uint32), {k: np.concatenate([v[k] for _, v in scenes]) for k in keys}


def filler(n_slots, like):
    """one object of n_slots slots that hold no vote (class -1): it only raises the call's cap / sends it down the workspace path"""
    v = {k: np.zeros((n_slots,) + a.shape[1:], a.dtype) for k, a in like.items()}
    v["cls"][:] = -1; v["weight"][:] = 1
    if "bbox_quat" in v:
        v["bbox_quat"][:, 0] = 1
    return np.asarray([0, n_slots], np.uint32), v


def objects(out, idx):
    """the outputs of the objects idx of a result (numpy or torch), as numpy"""
    return {k: (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a))[idx] for k, a in out.items() if k != "bins"}


# ------------------------------------------------------------------------------------------------ random scenes (moved from test_gpu_parity)
def vote_scene(rng, n_obj, n_classes, with_empty=True, big=()):
    pos, w, cls, inst, bs, off = [], [], [], [], [], [0]
    for o in range(n_obj):
        if with_empty and o == 1:
            off.append(off[-1]); continue
        n_blobs = rng.integers(1, 4) + (3 if o in big else 0)
        for b in range(n_blobs):
            c = rng.integers(0, n_classes)
            m = rng.integers(5, 120) * (12 if o in big else 1)
            centre = rng.uniform(-2, 2, 3)
            pos.append(centre + 0.15 * rng.normal(size=(m, 3))); w.append(rng.uniform(0.2, 1.0, m))
            cls.append(np.full(m, c)); inst.append(rng.integers(0, 4, m)); bs.append(rng.uniform(0.5, 1.5, (m, 3)))
        m = rng.integers(0, 40)                                   # clutter + slots without a vote
        pos.append(rng.uniform(-3, 3, (m, 3))); w.append(rng.uniform(0.2, 1.0, m)); cls.append(rng.integers(-1, n_classes, m))
        inst.append(rng.integers(0, 4, m)); bs.append(rng.uniform(0.5, 1.5, (m, 3)))
        off.append(off[-1] + sum(len(x) for x in pos) - off[-1])
    v = dict(pos=np.concatenate(pos).astype(np.float32), weight=np.concatenate(w).astype(np.float32), cls=np.concatenate(cls).astype(np.int32),
             inst=np.concatenate(inst).astype(np.int32), bbox_size=np.concatenate(bs).astype(np.float32))
    # shuffle inside every object so that classes interleave like real vote slots
    for o in range(n_obj):
        s, e = off[o], off[o + 1]
        p = s + rng.permutation(e - s)
        for key in v:
            v[key][s:e] = v[key][p]
    return np.asarray(off, np.uint32), v


def with_quats(rng, v):
    """bbox quaternions per vote slot: a few base rotations per blob-ish neighbourhood + jitter, unit length"""
    n = len(v["weight"])
    base = rng.normal(size=(6, 4)); base /= np.linalg.norm(base, axis=1, keepdims=True)
    q = base[rng.integers(0, 6, n)] + 0.05 * rng.normal(size=(n, 4))
    q *= np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]           # q and -q are the same rotation: the scatter matrix does not care
    v = dict(v); v["bbox_quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return v


def colliding_classes_scene():
    """12 objects, 5 classes: every object's votes once more under the next class, slightly shifted, so that maxima of different
    classes collide (the scene of the MaxFilterType Simple test)"""
    rng = np.random.default_rng(77)
    return collide(*vote_scene(rng, 12, 5), 5)


def collide(off, v, n_classes):
    """every object's votes once more under the next class, shifted by 0.05 and at 0.7 of the weight"""
    v2 = {k: np.concatenate([a, a]) for k, a in v.items()}
    n = len(v["weight"])
    v2["cls"][n:] = np.where(v["cls"] >= 0, (v["cls"] + 1) % n_classes, -1); v2["pos"][n:] += 0.05; v2["weight"][n:] *= 0.7
    order = np.concatenate([np.r_[off[o]:off[o + 1], n + off[o]:n + off[o + 1]] for o in range(len(off) - 1)])   # interleave the copies per object
    return (2 * off.astype(np.int64)).astype(np.uint32), {k: a[order] for k, a in v2.items()}


def stacked_classes_scene():
    """12 objects, 5 classes: blobs of DIFFERENT classes on top of each other and same-class blobs just outside the intra-class
    suppression, with quaternions (the scene of the MaxFilterType Merge test)"""
    rng = np.random.default_rng(83)
    pos, w, cls, inst, bs, off = [], [], [], [], [], [0]
    for o in range(12):
        for b in range(rng.integers(2, 4)):
            centre = rng.uniform(-1.5, 1.5, 3)
            for c in rng.choice(5, size=rng.integers(1, 4), replace=False):      # several classes vote for (almost) the same place
                m = rng.integers(8, 60)
                pos.append(centre + rng.uniform(-0.2, 0.2, 3) + 0.08 * rng.normal(size=(m, 3))); w.append(rng.uniform(0.2, 1.0, m))
                cls.append(np.full(m, c)); inst.append(rng.integers(0, 3, m)); bs.append(rng.uniform(0.5, 1.5, (m, 3)))
        off.append(sum(len(x) for x in pos))
    v = dict(pos=np.concatenate(pos).astype(np.float32), weight=np.concatenate(w).astype(np.float32), cls=np.concatenate(cls).astype(np.int32),
             inst=np.concatenate(inst).astype(np.int32), bbox_size=np.concatenate(bs).astype(np.float32))
    return np.asarray(off, np.uint32), with_quats(rng, v)


# ------------------------------------------------------------------------------------------------ Hough3D: the dyadic lattice
LAT_MIN, LAT_MAX, LAT_BIN = (-1.0, -2.0, -3.0), (5.5, 4.125, 4.0), 0.25      # 26 x 25 x 28 bins; the y extent is 24.5 bins
LAT_CNT = (26, 25, 28)
LAT_SEAMS = (22, 19)          # first bin of the second tile for tile edge 24 (LDS, cap <= 1024; workspace) and 21 (LDS, cap 2048)
LAT_MAXIMA = 96


def _lattice_features(seams):
    """[(class, bin (x, y, z), offset in quarter bins, weight in 64ths)] and the planted relations between bins.
    Every family of features keeps a Chebyshev distance >= 2 (>= 3 around off-centre votes) from every other, so that no bin of one
    is a 26-neighbour of a bin of another."""
    F, R = [], dict(plateau=[], step=[], first=[], last=[], kept=[], dropped=[])
    c0 = (0, 0, 0)

    def put(b, w64, off=c0, cls=0):
        F.append((cls, tuple(b), off, w64))

    def axis_bins(d, s, k, j):
        lo, hi = [0, 0, 0], [0, 0, 0]
        lo[d], hi[d] = s - 1, s
        for e, val in zip([a for a in range(3) if a != d], (2 + 3 * k, 2 + 3 * j)):
            lo[e] = hi[e] = val
        return tuple(lo), tuple(hi)
    for d in range(3):                                      # across every seam: a plateau, a step up and a step down
        for j, s in enumerate(seams):
            a, b = axis_bins(d, s, 0, j); put(a, 64); put(b, 32); put(b, 32); R["plateau"].append((a, b))
            a, b = axis_bins(d, s, 1, j); put(a, 64); put(b, 80); R["step"].append((a, b))          # b > a: only b is a maximum
            a, b = axis_bins(d, s, 2, j); put(a, 80); put(b, 64); R["step"].append((b, a))
    put((5, 5, 5), 64); put((6, 5, 5), 48); put((6, 5, 5), 16); R["plateau"].append(((5, 5, 5), (6, 5, 5)))   # a plateau inside a tile
    for b in ((0, 3, 3), (3, 0, 9), (9, 3, 0)):             # maxima in bin 0 of an axis
        put(b, 64); R["first"].append(b)
    return F, R, put


def lattice():
    """scene 1: one object, class 0 holds the lattice, class 1 two votes. -> (off, votes, relations)"""
    F, R, put = _lattice_features(LAT_SEAMS)
    # bin 0 of x one row above the last-x-bin maximum (25, 14, 14): with the two leading bin counts exchanged EVERYWHERE an index only
    # aliases (nx - 1, y, z) with (0, y + 1, z), so this is the pair that tells a consistently swapped index from the right one
    put((0, 15, 14), 64); R["first"].append((0, 15, 14))
    for b in ((25, 14, 14), (14, 24, 14), (14, 14, 27)):    # maxima in the last bin of an axis; y's is the partial bin, whose centre IS max_coord
        put(b, 64); R["last"].append(b)
    put((12, 12, 12), 64); put((12, 12, 12), 64)            # max(H) = 2
    put((16, 12, 12), 96); put((16, 12, 12), 32)            # exactly max(H): kept at rel = 1 and 1.5
    put((12, 16, 16), 64); put((12, 16, 16), 63)            # one quantum below max(H): dropped there
    put((16, 16, 8), 63)                                    # one quantum below 0.5 max(H): dropped at rel = 0.5 (every 64/64 bin sits exactly on it)
    R["kept"] += [((16, 12, 12), 1.0), ((5, 5, 5), 0.5)]; R["dropped"] += [((12, 16, 16), 1.0), ((16, 16, 8), 0.5)]
    put((8, 14, 4), 64, (1, -1, 0)); put((8, 14, 4), 48, (-1, 1, 1))       # off-centre votes: the trilinear split
    put((3, 3, 3), 64, cls=1); put((3, 3, 3), 32, (1, 1, -1), cls=1)
    pos = [[LAT_MIN[d] + (b[d] + 0.5 + o[d] / 4) * LAT_BIN for d in range(3)] for _, b, o, _ in F]
    w = [w64 / 64 for _, _, _, w64 in F]
    cls = [c for c, _, _, _ in F]
    # a vote exactly on the boundary of bins 7 | 8 along x (interpolation halves it: a plateau of two bins at 1), one exactly at
    # min_coord (inside; its low neighbours are outside the space) and one exactly at max_coord (outside along x and z)
    pos += [[LAT_MIN[0] + 8 * LAT_BIN, LAT_MIN[1] + 8.5 * LAT_BIN, LAT_MIN[2] + 12.5 * LAT_BIN], list(LAT_MIN), list(LAT_MAX)]
    w += [2.0, 1.0, 1.0]; cls += [0, 0, 0]
    R["boundary"] = ((7, 8, 12), (8, 8, 12)); R["corner"] = (0, 0, 0)
    n = len(w)
    order = np.random.default_rng(5).permutation(n)         # slot order is not feature order
    v = pack(np.asarray(pos)[order], np.asarray(w)[order], np.asarray(cls)[order], (np.arange(n) * 7 % 5)[order])
    return np.asarray([0, n], np.uint32), v, R


def lattice_bin_index(b, cnt=LAT_CNT):
    return b[0] + cnt[0] * (b[1] + cnt[1] * b[2])


CB_BINS = (0.125, 0.25, 0.5)


def class_bin_lattice():
    """scene 3: three classes with bins 0.125 / 0.25 / 0.5 in the space of the lattice: a plateau pair, a step, a bin-0 maximum and an
    off-centre vote each, on each class's own bin grid"""
    pos, w, cls = [], [], []
    for c, bs in enumerate(CB_BINS):
        for b, o, w64 in (((2, 2, 2), (0, 0, 0), 64), ((3, 2, 2), (0, 0, 0), 32), ((3, 2, 2), (0, 0, 0), 32),      # plateau
                          ((2, 5, 2), (0, 0, 0), 64), ((2, 6, 2), (0, 0, 0), 80),                                  # step
                          ((0, 4, 5), (0, 0, 0), 64), ((5, 1, 5), (1, -1, 1), 96), ((5, 1, 5), (0, 0, 0), 16)):
            pos.append([LAT_MIN[d] + (b[d] + 0.5 + o[d] / 4) * bs for d in range(3)]); w.append(w64 / 64); cls.append(c)
    n = len(w)
    order = np.random.default_rng(6).permutation(n)
    return np.asarray([0, n], np.uint32), pack(np.asarray(pos)[order], np.asarray(w)[order], np.asarray(cls)[order], (np.arange(n) % 3)[order])


def isolated_bins(n):
    """scene 5: n unit votes of one class on the centres of distinct, non-adjacent bins of the default space (bin 0.25)"""
    i = np.arange(n)
    b = np.stack([2 * (i % 19) + 1, 2 * (i // 19) + 1, np.full(n, 20)], 1)
    pos = -5.0 + (b + 0.5) * 0.25
    return np.asarray([0, n], np.uint32), pack(pos, np.ones(n), np.zeros(n), i % 3)


# ------------------------------------------------------------------------------------------------ mean shift
ISO_H = 1.0


def isolated_votes(n_per_class, n_classes, weight=0.5):
    """scene 6: slot s is vote s // n_classes of class s % n_classes, at x = 16 h * (s // n_classes), y = z = 0: 16 bandwidths apart
    within a class (classes do not interact), x ascending with the slot. Under the uniform kernel every vote is a maximum of its own."""
    s = np.arange(n_per_class * n_classes)
    pos = np.stack([16.0 * ISO_H * (s // n_classes), np.zeros(len(s)), np.zeros(len(s))], 1)
    return np.asarray([0, len(s)], np.uint32), pack(pos, np.full(len(s), weight), s % n_classes, s * 7 % 5)


def three_blobs():
    """scene 7: three Gaussian blobs of one class (sigma 0.2) whose modes the mean shift (h = 0.5) only separates after a few steps"""
    rng = np.random.default_rng(2024)
    centres = np.asarray([[0.0, 0.0, 0.0], [0.75, 0.1, 0.0], [0.3, 0.8, 0.2]])
    pos = np.concatenate([c + 0.2 * rng.normal(size=(40, 3)) for c in centres])
    n = len(pos)
    return np.asarray([0, n], np.uint32), pack(pos, rng.uniform(0.2, 1.0, n), np.zeros(n), rng.integers(0, 3, n))


CHAIN_H = 1.0
CHAIN = np.asarray([[0.3125, 0.0, 0.0], [0.3125, 0.703125, 0.703125], [1.09375, 0.703125, 0.703125], [1.25, 0.703125, 0.703125]])


def chain():
    """scene 7, closed form: four unit votes under the uniform kernel, h = 1. The only seed that sees a vote is the cell centre at
    the origin (it sees vote 0 alone); from the mean of votes 0..k-1 exactly vote k comes into range, so after k steps the centre is
    the mean of the first k votes, and it rests at the mean of all four. test_maxima_cpu.py proves the ranges."""
    return np.asarray([0, 4], np.uint32), pack(CHAIN, np.ones(4), np.zeros(4), np.arange(4))


SEED_H = float(f32(0.35355338))           # (h * 2) / sqrtf(2) is exactly 0.5 in float32


def seed_boundary_rows():
    """scene 8: rows of votes with x = (k + 0.5) * 0.5, k = -3..2 (x / cell exactly half-integral, both signs), y and z on cell centres"""
    pos, w = [], []
    for r, (y, z) in enumerate(((0.0, 0.0), (1.5, -1.0), (-2.0, 0.5))):
        for k in range(-3, 3):
            pos.append([(k + 0.5) * 0.5, y, z]); w.append((1 + (k + r) % 3) / 4)
    n = len(w)
    return np.asarray([0, n], np.uint32), pack(pos, w, np.zeros(n), np.arange(n) % 4)


def seed_boundary_corner(n_coords):
    """one vote with n_coords coordinates on a cell boundary: 2 -> its seed sits sqrt(1/8) away, a hair more than h; 3 -> farther"""
    p = [0.25 if d < n_coords else 0.0 for d in range(3)]
    return np.asarray([0, 1], np.uint32), pack([p], [1.0], [0], [0])


TALLY_CASES = ("full64", "full256", "collide", "negative", "equal", "zero")


def tally(case):
    """scene 9: one tight blob of one class (one maximum holding every vote), ids and dyadic weights per case"""
    n = dict(full64=64, full256=256).get(case, 40)
    i = np.arange(n)
    cap = mm.pow2_cap(n)
    if case.startswith("full"):                              # n == cap distinct ids; the heaviest weight is shared: the lowest id wins
        ids, w = 3 * i[::-1] + 1, (1 + i % 7) / 64
    elif case == "collide":                                  # 12 ids with one first probe slot near the table's end
        r = next(r for r in range(1, 1 << 16) if mm.first_probe(r, cap) >= cap - 6)
        ids, w = (i % 12) * cap + r, (1 + i % 5) / 64
    elif case == "negative":                                 # -7 and 7 tie at the top: 7 is the lower unsigned number
        ids, w = np.asarray([-7, 7, -2, 3])[i % 4], np.where(i % 4 < 2, 0.5, 0.25)
    elif case == "equal":                                    # 4 (0.5 + 0.25 + 0.25 ...) and 9 (1.0 ...) reach the same sum by different routes
        ids = np.asarray([9, 4, 4, 4, 2])[i % 5]; w = np.asarray([1.0, 0.5, 0.25, 0.25, 0.75])[i % 5]
    else:                                                    # "zero": every vote of instance 5 has weight 0
        ids = np.asarray([5, 1, 6])[i % 3]; w = np.asarray([0.0, 0.5, 0.25])[i % 3]
    pos = np.stack([(i % 4) / 64, (i // 4 % 4) / 64, (i // 16) / 256], 1)
    return np.asarray([0, n], np.uint32), pack(pos, w, np.zeros(n), ids)


TALLY_HOUGH = dict(bin_size=2.0, min_coord=(-1, -1, -1), max_coord=(1, 1, 1), use_interpolation=False)      # one bin


def zero_weight_blob():
    """a maximum whose members all have weight 0: the reference divides by the zero weight sum (undefined; kept out of the parity scenes)"""
    off, v = tally("zero")
    v["weight"][:] = 0
    return off, v


# ------------------------------------------------------------------------------------------------ both paths, many pairs
OPT_CLASSES = 4


def options_scene():
    """scene 10: (off, votes) of 7 random objects with quaternions and the same call with one object of 2049 slots appended"""
    rng = np.random.default_rng(101)
    off, v = collide(*vote_scene(rng, 7, OPT_CLASSES), OPT_CLASSES)       # classes collide: the filters have work
    v = with_quats(rng, v)
    m = mm.K["LDS_SLOTS"] + 1
    centres = rng.uniform(-2, 2, (8, 3))
    blob = rng.integers(0, 8, m)
    ex = with_quats(rng, pack(centres[blob] + 0.15 * rng.normal(size=(m, 3)), rng.uniform(0.2, 1.0, m), blob % OPT_CLASSES, rng.integers(0, 4, m),
                              rng.uniform(0.5, 1.5, (m, 3))))
    cen = rng.uniform(-0.5, 0.5, (8, 3)).astype(f32); rad = rng.uniform(1.0, 2.0, 8).astype(f32)
    return (off, v), concat([(off, v), (np.asarray([0, m], np.uint32), ex)]), cen, rad


MANY_CLASSES, MANY_OBJECTS, MANY_BIG = 128, 9, 8


def many_pairs():
    """scene 11: 9 objects x 128 classes = 1152 (object, class) pairs; object 8 has 18 votes in every class (2304 slots: the
    workspace path), the others 200 slots in 60 blobs of random classes"""
    rng = np.random.default_rng(11)
    scenes = []
    for o in range(MANY_OBJECTS):
        if o == MANY_BIG:
            c = np.repeat(np.arange(MANY_CLASSES), 18)
            centres = rng.uniform(-2.5, 2.5, (MANY_CLASSES, 3))
            pos = centres[c] + 0.06 * rng.normal(size=(len(c), 3))
            p = rng.permutation(len(c)); c, pos = c[p], pos[p]
        else:
            blob = rng.integers(0, 60, 200)                   # 60 small blobs of random classes
            c = rng.integers(0, MANY_CLASSES, 60)[blob]
            pos = rng.uniform(-2.5, 2.5, (60, 3))[blob] + 0.05 * rng.normal(size=(200, 3))
        n = len(c)
        scenes.append((np.asarray([0, n], np.uint32), pack(pos, rng.uniform(0.2, 1.0, n), c, rng.integers(0, 4, n), rng.uniform(0.5, 1.5, (n, 3)))))
    return concat(scenes)


EDGE_CLASSES, EDGE_SIZES = 205, [2100, 150, 10, 150, 300]


def chunk_edge_pairs():
    """5 objects x 205 classes = 1025 (object, class) pairs: one more than a pass of k_work_offsets, so the pair (4, 204) alone -- flat
    index 1024 -- takes its region from the carry of everything before it. Object 0 has 2100 slots (the workspace path); every class
    of an object is one tight blob around the class's centre; object 4 has 40 votes each in classes 203 and 204, the pairs on
    either side of the edge"""
    rng = np.random.default_rng(21)
    centres = rng.uniform(-2.5, 2.5, (EDGE_CLASSES, 3))
    scenes = []
    for o, n in enumerate(EDGE_SIZES):
        c = rng.integers(0, EDGE_CLASSES, n)
        if o == 4:
            c[:40], c[40:80] = EDGE_CLASSES - 1, EDGE_CLASSES - 2
        pos = centres[c] + 0.05 * rng.normal(size=(n, 3))
        scenes.append((np.asarray([0, n], np.uint32), pack(pos, rng.uniform(0.2, 1.0, n), c, rng.integers(0, 4, n), rng.uniform(0.5, 1.5, (n, 3)))))
    return concat(scenes)


# the option sets of scene 10; every one runs on the LDS path (scene alone) and on the workspace path (2049-slot object appended)
OPT_CLASS_BW = [0.3, 0.5, 0.8, 0.4]
MS_BASE = dict(n_classes=OPT_CLASSES, bandwidth=0.5, max_maxima=16, min_votes_threshold=2)
MS_OPTIONS = dict(average=dict(suppression=0), suppress=dict(suppression=1), none=dict(suppression=2), uniform=dict(kernel=1),
                  class_bandwidth=dict(class_bandwidth=OPT_CLASS_BW), rotation=dict(average_rotation=True), simple=dict(max_filter=1),
                  merge=dict(max_filter=2, average_rotation=True), merge_class_bandwidth=dict(max_filter=2, class_bandwidth=OPT_CLASS_BW),
                  som1=dict(single_object_max_type=1, bandwidth=0.8, min_votes_threshold=1),
                  som2=dict(single_object_max_type=2, bandwidth=0.8, min_votes_threshold=1),
                  som3=dict(single_object_max_type=3, bandwidth=0.8, min_votes_threshold=1))
HOUGH_BASE = dict(n_classes=OPT_CLASSES, bin_size=0.5, rel_threshold=0.3, max_maxima=16, min_votes_threshold=2)
HOUGH_OPTIONS = dict(interpolated=dict(use_interpolation=True), plain=dict(use_interpolation=False), rotation=dict(average_rotation=True),
                     simple=dict(max_filter=1), merge=dict(max_filter=2, average_rotation=True), class_bin=dict(class_bin=[0.25, 0.5, 0.5, 1.0]))


# ------------------------------------------------------------------------------------------------ calls and closed forms shared by the CPU and the GPU tests
LAT_KW = dict(n_classes=2, bin_size=LAT_BIN, min_coord=LAT_MIN, max_coord=LAT_MAX, max_maxima=LAT_MAXIMA)
LATTICE_RUNS = dict(alone=0, cap2048=1100, workspace=2049)          # slots of the filler object sent along


def lattice_run(name):
    off, v, R = lattice()
    if LATTICE_RUNS[name]:
        off, v = concat([(off, v), filler(LATTICE_RUNS[name], v)])
    return off, v, R


def class_bin_scenes():
    rng = np.random.default_rng(9)
    off, v = vote_scene(rng, 6, 3)
    return dict(lattice=class_bin_lattice(), random=(off, v))


CB_KW = dict(n_classes=3, bin_size=0.5, class_bin=list(CB_BINS), min_coord=LAT_MIN, max_coord=LAT_MAX, rel_threshold=0.5, max_maxima=32)
ISO_KW = dict(bandwidth=ISO_H, kernel=1)


def isolated_closed_form(n_per_class, n_classes, limit=None):
    """class ascending, then slot order; every vote its own maximum at its own place"""
    off, v = isolated_votes(n_per_class, n_classes)
    order = np.argsort(v["cls"], kind="stable")[:limit]
    return dict(n=len(order), pos=v["pos"][order], cls=v["cls"][order], inst=v["inst"][order], bbox_size=v["bbox_size"][order],
                weight=1.0 / len(order))


def assert_isolated(out, want):
    n = want["n"]
    assert out["n"][0] == n
    assert np.array_equal(out["cls"][0, :n], want["cls"]) and np.array_equal(out["inst"][0, :n], want["inst"])
    assert np.array_equal(out["pos"][0, :n], want["pos"]) and np.array_equal(out["bbox_size"][0, :n], want["bbox_size"])
    assert (out["n_votes"][0, :n] == 1).all()
    np.testing.assert_allclose(out["weight"][0, :n], want["weight"], atol=1e-7)
    np.testing.assert_allclose(out["inst_weight"][0, :n], want["weight"], atol=1e-7)


CHAIN_KW = dict(n_classes=1, bandwidth=CHAIN_H, threshold=0.0, kernel=1, suppression=1, max_maxima=4)
TALLY_MS = dict(n_classes=1, bandwidth=0.5, kernel=1, max_maxima=4)
