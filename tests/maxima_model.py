"""Host model of the launch decisions of csrc/maxima.hip (maxima_setup, big_object_workspace, k_work_offsets, class_votes_layout,
hough3d_maxima_impl, hough3d_body, instance_tally): which path a call takes, how large the per-class tables are, where the Hough
accumulator tiles meet and where an instance id first lands in its hash table. No GPU import: test_maxima_cpu.py uses it to PROVE
that the scenes of maxima_scenes.py reach the paths they were built for.

The capacities are read from the source, so that a retune makes the path proofs fail instead of silently hollowing them."""
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point-cloud-donkey_amd", "csrc")


def _const(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)", text, re.M)
    assert m, f"{name}: no longer a #define of maxima.hip"
    return int(m.group(1))


def constants():
    with open(os.path.join(_CSRC, "maxima.hip")) as f:
        text = f.read()
    return {k: _const(text, "MX_" + k) for k in ("LDS_SLOTS", "MAXM", "MAXM_C", "MAXC")}


K = constants()
OFFSET_CHUNK = 1024          # (object, class) pairs per pass of k_work_offsets (its block size)


def pow2_cap(n):
    """pow2_cap(): the smallest power of two >= max(n, 64)"""
    c = 64
    while c < n:
        c <<= 1
    return c


def launch(slot_off):
    """maxima_setup: (cap, big) of a call; cap sizes the LDS tables of every workgroup, big sends the WHOLE call down the workspace path"""
    sizes = np.diff(np.asarray(slot_off, np.int64))
    cap = pow2_cap(int(sizes.max()))
    return cap, cap > K["LDS_SLOTS"]


def class_counts(slot_off, cls, n_classes):
    """k_class_counts: votes per (object, class), row-major"""
    off = np.asarray(slot_off, np.int64)
    out = np.zeros((len(off) - 1, n_classes), np.int64)
    for o in range(len(off) - 1):
        c = np.asarray(cls[off[o]:off[o + 1]])
        c = c[(c >= 0) & (c < n_classes)]
        out[o] = np.bincount(c, minlength=n_classes)
    return out


def class_caps(counts):
    """class_votes_layout<GM = true>: table size of every (object, class) on the workspace path"""
    return np.vectorize(pow2_cap)(counts)


def work_offsets(counts):
    """k_work_offsets: region start of every (object, class) in slots (absent classes take nothing) and, per pair, the pass of
    the chunk loop that computed it (pass >= 1: the start rests on the carry out of an earlier chunk)"""
    flat = np.asarray(counts).reshape(-1)
    size = np.where(flat > 0, np.vectorize(pow2_cap)(flat), 0)
    return (np.cumsum(size) - size).reshape(np.shape(counts)), (np.arange(len(flat)) // OFFSET_CHUNK).reshape(np.shape(counts))


def hough_tile_edge(cap, big):
    """the edge loop of hough3d_maxima_impl: 37 bytes of LDS per vote slot (none on the workspace path), the rest of 150 KB is the tile"""
    vote_bytes = 0 if big else cap * (4 * 4 + 2 * 4 + 8 + 4 + 1)
    vote_bytes = (vote_bytes + 15) // 16 * 16
    edge = 24
    while edge > 8 and vote_bytes + edge ** 3 * 8 > 150 * 1024:
        edge -= 1
    return edge


def hough_tiles(lo, hi, edge):
    """hough3d_body: a tile's interior is (edge - 2) bins per axis, starting at the low corner of the reachable-bin box [lo, hi].
    -> (tiles per axis, per axis the list of seams s: bins s - 1 and s lie in different tiles)"""
    ei = edge - 2
    nt = [(hi[d] - lo[d]) // ei + 1 for d in range(3)]
    return nt, [[lo[d] + k * ei for k in range(1, nt[d])] for d in range(3)]


def reachable_box(bins, cnt):
    """hough3d_body: bounding box of the in-space votes' bins (int [n, 3]), one bin wider for the interpolation neighbours"""
    bins = np.asarray(bins, np.int64).reshape(-1, 3)
    cnt = np.asarray(cnt, np.int64)
    return np.maximum(bins.min(0) - 1, 0).tolist(), np.minimum(bins.max(0) + 1, cnt - 1).tolist()


def first_probe(inst_id, cap):
    """instance_tally: first slot of an instance id in the table of cap entries (Knuth's multiplicative hash, linear probing after it)"""
    return ((int(inst_id) & 0xFFFFFFFF) * 2654435761 & 0xFFFFFFFF) & (cap - 1)


def probe_table(ids, cap):
    """the table after inserting ids in the given order -> (slot of every distinct id, longest probe chain, wrapped past the end?)"""
    table, slot_of, longest, wrapped = {}, {}, 0, False
    for i in ids:
        i = int(i)
        if i in slot_of:
            continue
        s, steps = first_probe(i, cap), 0
        while s in table:
            s = (s + 1) & (cap - 1); steps += 1
            wrapped |= s == 0
            assert steps < cap, "table full"
        table[s] = i; slot_of[i] = s; longest = max(longest, steps)
    return slot_of, longest, wrapped
