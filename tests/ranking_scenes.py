"""Inputs of the feature ranking tests: small class-major descriptor sets (non-negative, histogram-like rows, unit L2 norm like SHOT)
and hand-made score vectors for the selection."""
import numpy as np


def _rows(rng, sizes, dim):
    """every class scatters around its own sparse prototype, so own-class and other-class neighbours differ"""
    out = []
    for s in sizes:
        proto = rng.random(dim) ** 3 * (rng.random(dim) < 0.5)
        x = rng.random((s, dim)) ** 3 * (rng.random((s, dim)) < 0.6)
        x = 0.5 * proto[None, :] + 0.5 * x
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
        out.append(x.astype(np.float32))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate(out)), off


def mixed():
    """one class smaller than K + 1, one empty"""
    desc, off = _rows(np.random.default_rng(101), (150, 5, 0, 97), 33)
    return dict(name="mixed", desc=desc, off=off, k_search=10)


def wide():
    """8 exact duplicates of a row inside class 0 and one row of class 1 repeated 4 times in class 2: zero distances, ties that go to
    the lowest row, a self match that is not first. (A Strangeness score of +inf needs KSearch zero distances in another class: that
    case is in nan(), where KSearch is 3.)"""
    desc, off = _rows(np.random.default_rng(202), (200, 130, 70), 352)
    for t in range(8):
        desc[20 + 2 * t] = desc[3]                   # class 0: rows 3, 20, 22, ... are one row
    for t in range(4):
        desc[off[2] + 5 + t] = desc[off[1] + 7]      # class 2 rows = one row of class 1, four times
    return dict(name="wide", desc=desc, off=off, k_search=10)


def large_k():
    desc, off = _rows(np.random.default_rng(303), (300, 260), 64)
    return dict(name="large-k", desc=desc, off=off, k_search=20)


def nan():
    """one row with 4 copies in class 0 and 3 in class 1, KSearch 3: its own-class sum and its smallest other-class sum are both 0, a
    Strangeness score of 0/0. A single further copy in class 2 has a positive own-class sum over that 0: +inf."""
    desc, off = _rows(np.random.default_rng(404), (40, 30, 25), 16)
    for i in (2, 11, 17, 33):
        desc[i] = desc[2]
    for i in (1, 8, 20):
        desc[off[1] + i] = desc[2]
    desc[off[2] + 4] = desc[2]
    return dict(name="nan", desc=desc, off=off, k_search=3)


def hub():
    """rows that are the neighbour of many: 11 copies of one row with 1250 satellites in class 0, the same with 200 satellites in
    class 1. A satellite is the row plus a small dense perturbation in a random direction, its size between 0.05 and 0.1 per element:
    in 352 dimensions two random directions are nearly orthogonal, so a satellite is farther from every other satellite (about
    d_r + d_r') than from the copies (d_r). The copies' reverse lists hold more than a thousand and a few hundred terms of different
    sizes: the long-list paths of the deterministic accumulation, where the order of the float sum shows."""
    rng = np.random.default_rng(505)
    dim, out = 352, []
    for sats in (1250, 200):
        h = rng.random(dim) + 0.5
        e = rng.uniform(-1, 1, (sats, dim)) * rng.uniform(0.05, 0.1, (sats, 1))
        out.append(np.concatenate([np.tile(h, (11, 1)), h[None, :] + e]).astype(np.float32))
    off = np.asarray([0, len(out[0]), len(out[0]) + len(out[1])], np.uint32)
    return dict(name="hub", desc=np.ascontiguousarray(np.concatenate(out)), off=off, k_search=10)


SCENES = (mixed, wide, large_k, nan, hub)


def bayes_threshold(dist):
    """a threshold between two neighbour distances of the scene: the midpoint of the two middle distinct values"""
    d = np.unique(dist[np.isfinite(dist)].astype(np.float32))
    m = len(d) // 2
    return float((np.float64(d[m - 1]) + np.float64(d[m])) / 2)


# (factor, extract_offset) pairs of the selection tests
WINDOWS = ((0.75, 0.0), (0.75, 0.125), (0.75, 0.25), (0.5, 0.7), (1.0, 0.0), (0.3, 0.0), (0.0, 0.0))


def score_vectors():
    """hand-made score vectors: (name, score, class offsets)"""
    inf, nan_ = np.inf, np.nan
    cases = [
        ("integer-ties", [3, 1, 2, 1, 3, 3, 0, 1, 2, 2, 1, 0], [0, 12]),
        ("seven", [0.5, 0.1, 0.9, 0.3, 0.7, 0.2, 0.6], [0, 7]),
        ("signed-zero", [0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -0.0, 0.0], [0, 8]),
        ("inf", [inf, 1.0, -inf, inf, 0.0, 2.0, -inf, inf], [0, 8]),
        ("nan", [nan_, 1.0, inf, nan_, -1.0, 0.5, nan_, inf, 0.25], [0, 9]),
        ("classes", [2, 2, 1, nan_, 0, 5, 5, 5, -0.0, 0.0, inf, 1, 1, 7], [0, 5, 5, 6, 14]),
    ]
    return [(n, np.asarray(s, np.float32), np.asarray(o, np.uint32)) for n, s, o in cases]
