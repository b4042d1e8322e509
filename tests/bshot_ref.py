"""B-SHOT restated in numpy from features/features_bshot.cpp:109-157 (getBinaryVector), statement by statement, plus a brute-force
Hamming search. Shares no code with the library.

Sums are float32 in the written order; every comparison is float64: the reference compares a float lhs with `sum * 0.9`, where 0.9 is
a double literal, so both sides are promoted."""
import numpy as np

f32 = np.float32
f64 = np.float64
DIM = 352


def binary_vector(vec):
    """getBinaryVector for one group of four floats -> [4] ints"""
    v = [f32(x) for x in vec]
    result = [0, 0, 0, 0]                                          # initialization: case A
    with np.errstate(invalid="ignore", over="ignore"):
        s = f32(f32(f32(v[0] + v[1]) + v[2]) + v[3])
        if s != 0:
            t = f64(s) * f64(0.9)
            # case B
            case_b = False
            if f64(v[0]) > t: result[0] = 1
            if f64(v[1]) > t: result[1] = 1
            if f64(v[2]) > t: result[2] = 1
            if f64(v[3]) > t: result[3] = 1
            if sum(result) == 1: case_b = True
            # case C
            case_c = False
            if not case_b:
                if f64(f32(v[0] + v[1])) > t: result = [1, 1, 0, 0]
                if f64(f32(v[0] + v[2])) > t: result = [1, 0, 1, 0]
                if f64(f32(v[0] + v[3])) > t: result = [1, 0, 0, 1]
                if f64(f32(v[1] + v[2])) > t: result = [0, 1, 1, 0]
                if f64(f32(v[1] + v[3])) > t: result = [0, 1, 0, 1]
                if f64(f32(v[2] + v[3])) > t: result = [0, 0, 1, 1]
                if sum(result) == 2: case_c = True
            # case D
            case_d = False
            if not case_b and not case_c:
                if f64(f32(f32(v[0] + v[1]) + v[2])) > t: result = [1, 1, 1, 0]
                if f64(f32(f32(v[0] + v[1]) + v[3])) > t: result = [1, 1, 0, 1]
                if f64(f32(f32(v[0] + v[2]) + v[3])) > t: result = [1, 0, 1, 1]
                if f64(f32(f32(v[1] + v[2]) + v[3])) > t: result = [0, 1, 1, 1]
                if sum(result) == 3: case_d = True
            # case E
            if not case_b and not case_c and not case_d:
                result = [1, 1, 1, 1]
    return result


def binarize(rows):
    """the same for whole rows [n, 4 m] -> float32 zeros and ones, vectorised over the groups in the same statement order"""
    rows = np.asarray(rows, f32)
    g = rows.reshape(-1, 4)
    v = [g[:, i] for i in range(4)]
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((v[0] + v[1]).astype(f32) + v[2]).astype(f32) + v[3]
        s = s.astype(f32)
        t = s.astype(f64) * f64(0.9)
        gt = lambda lhs: lhs.astype(f32).astype(f64) > t
        res = np.zeros((len(g), 4), np.int64)
        live = s != 0
        for i in range(4):
            res[:, i] = gt(v[i])
        case_b = res.sum(1) == 1
        for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            hit = ~case_b & gt(v[i] + v[j])
            pat = np.zeros(4, np.int64); pat[[i, j]] = 1
            res[hit] = pat
        case_c = ~case_b & (res.sum(1) == 2)
        for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
            hit = ~case_b & ~case_c & gt((v[i] + v[j]).astype(f32) + v[k])
            pat = np.zeros(4, np.int64); pat[[i, j, k]] = 1
            res[hit] = pat
        case_d = ~case_b & ~case_c & (res.sum(1) == 3)
        res[~case_b & ~case_c & ~case_d] = 1
        res[~live] = 0
    return res.astype(f32).reshape(rows.shape)


def margins(rows64):
    """per group of float64 rows [n, 4 m]: (sum, the smallest |lhs - 0.9 sum| over the 14 subset tests), both [n, m]"""
    g = np.asarray(rows64, f64).reshape(-1, 4)
    s = g.sum(1)
    subsets = [(i,) for i in range(4)] + [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    m = np.full(len(g), np.inf)
    for sub in subsets:
        m = np.minimum(m, np.abs(g[:, list(sub)].sum(1) - 0.9 * s))
    shape = (rows64.shape[0], rows64.shape[1] // 4)
    return s.reshape(shape), m.reshape(shape)


def hamming_knn(words, q, k):
    """brute force: the k nearest rows of words for every row of q by (Hamming distance, row) -> idx [nq, k] int32 (-1 beyond the
    codebook), dist [nq, k] float32 (NaN there)"""
    w = np.asarray(words) != 0
    x = np.asarray(q) != 0
    nw = len(w)
    wf = w.astype(f32)                                             # float32 products of zeros and ones: exact integers (<= dim < 2^24)
    wn = w.sum(1).astype(np.int64)
    kk = min(k, nw)
    idx = np.full((len(x), k), -1, np.int32)
    dist = np.full((len(x), k), np.nan, f32)
    for a in range(0, len(x), 4096):                               # in chunks: the key matrix of a chunk stays small
        xc = x[a:a + 4096]
        d = xc.sum(1).astype(np.int64)[:, None] + wn[None, :] - 2 * (xc.astype(f32) @ wf.T).astype(np.int64)
        key = d * nw + np.arange(nw)[None, :]
        if kk < nw:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key = np.sort(key, axis=1)[:, :kk]
        idx[a:a + 4096, :kk] = key % nw
        dist[a:a + 4096, :kk] = (key // nw).astype(f32)
    return idx, dist
