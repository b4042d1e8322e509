"""float64 numpy restatement of pcl::recognition::HoughSpace3D as SURVEY.md Appendix A.7 describes it, and of what VotingHough3D
does with a maximum (voting_hough_3d.cpp:70-93: the weighted centre of the bin's voters; Voting::findMaxima, voting.cpp:131-236 and
436-462: weight, instance, box size, order, normalisation). Written from the survey and those line references, not from the oracle
or the kernel: test_maxima_cpu.py holds the oracle to it on inputs whose sums are exact in every number format involved, and the
mutation check of that file's docstring shows that it tells a swapped axis, a wrong comparison and a moved threshold apart.

Everything is plain Python over float64; scenes have a few hundred votes."""
import math

import numpy as np


def bin_counts(min_coord, max_coord, bin_size):
    """bins per axis: ceil((max - min) / bin) -- an extent that is no multiple of the bin gets a partial last bin"""
    return [int(math.ceil((float(max_coord[d]) - float(min_coord[d])) / float(bin_size))) for d in range(3)]


def vote_bin(p, min_coord, bin_size, cnt):
    """central bin of a point, or None outside the space (a coordinate exactly at min is inside, exactly at min + cnt * bin outside)"""
    c = [int(math.floor((float(p[d]) - float(min_coord[d])) / bin_size)) for d in range(3)]
    return c if all(0 <= c[d] < cnt[d] for d in range(3)) else None


def accumulate(pos, w, min_coord, max_coord, bin_size, interpolate):
    """-> (cnt, H): H maps the bin index x + nx (y + ny z) to [value, voters in vote order]"""
    bin_size = float(bin_size)
    cnt = bin_counts(min_coord, max_coord, bin_size)
    H = {}
    for i in range(len(w)):
        c = vote_bin(pos[i], min_coord, bin_size, cnt)
        if c is None:
            continue
        if not interpolate:                                           # vote: the whole weight to the central bin
            e = H.setdefault(c[0] + cnt[0] * (c[1] + cnt[1] * c[2]), [0.0, []])
            e[0] += float(w[i]); e[1].append(i)
            continue
        # voteInt: per axis the central bin gets 1 - |x - centre| / bin, the nearer neighbour the rest
        share = []
        for d in range(3):
            x = float(pos[i][d]) - float(min_coord[d])
            diff = x - (c[d] + 0.5) * bin_size
            wc = 1.0 - abs(diff) / bin_size
            share.append([(c[d], wc), (c[d] + (-1 if diff < 0 else 1), 1.0 - wc)])
        for bx, fx in share[0]:
            for by, fy in share[1]:
                for bz, fz in share[2]:
                    f = fx * fy * fz
                    if not f > 0.0 or not (0 <= bx < cnt[0] and 0 <= by < cnt[1] and 0 <= bz < cnt[2]):
                        continue                                      # nothing to give, or the neighbour lies outside the space
                    e = H.setdefault(bx + cnt[0] * (by + cnt[1] * bz), [0.0, []])
                    e[0] += float(w[i]) * f; e[1].append(i)
    return cnt, H


def find_maxima(cnt, H, rel):
    """findMaxima(-rel): threshold = rel * max(H) (PCL takes max(H) itself for rel > 1); a bin >= threshold without a strictly
    greater 26-neighbour is a maximum; ascending bin index"""
    if not H:
        return []
    hmax = max(e[0] for e in H.values())
    thr = rel * hmax if rel <= 1.0 else hmax
    out = []
    for idx in sorted(H):
        v = H[idx][0]
        if v < thr or not v > 0.0:                                    # an empty bin has no voters: Voting::findMaxima drops it
            continue
        x, y, z = idx % cnt[0], (idx // cnt[0]) % cnt[1], idx // (cnt[0] * cnt[1])
        greater = False
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    nx, ny, nz = x + dx, y + dy, z + dz
                    if (dx or dy or dz) and 0 <= nx < cnt[0] and 0 <= ny < cnt[1] and 0 <= nz < cnt[2]:
                        e = H.get(nx + cnt[0] * (ny + cnt[1] * nz))
                        greater |= e is not None and e[0] > v
        if not greater:
            out.append(idx)
    return out


def best_instance(inst, w):
    """the instance id with the largest summed weight; the lowest id as an unsigned number among equals; none (-1, 0) when no sum is > 0"""
    sums = {}
    for i, x in zip(inst, w):
        sums[int(i) & 0xFFFFFFFF] = sums.get(int(i) & 0xFFFFFFFF, 0.0) + float(x)
    best, bid = 0.0, None
    for u in sorted(sums):
        if sums[u] > best:
            best, bid = sums[u], u
    if bid is None:
        return -1, 0.0
    return (bid - (1 << 32) if bid >= 1 << 31 else bid), best


def hough3d_maxima(slot_offsets, votes, n_classes, bin_size, min_coord=(-5, -5, -5), max_coord=(5, 5, 5), use_interpolation=True,
                   rel_threshold=0.8, min_votes_threshold=1, max_maxima=16, class_bin=None):
    """the outputs of the oracle's hough3d_maxima (no MinThreshold, BestK, filter or rotation), float64"""
    off = np.asarray(slot_offsets, np.int64)
    n_obj = len(off) - 1
    out = dict(n=np.zeros(n_obj, np.int32), pos=np.zeros((n_obj, max_maxima, 3)), weight=np.zeros((n_obj, max_maxima)),
               cls=np.full((n_obj, max_maxima), -1, np.int32), inst=np.full((n_obj, max_maxima), -1, np.int32),
               inst_weight=np.zeros((n_obj, max_maxima)), bbox_size=np.zeros((n_obj, max_maxima, 3)),
               n_votes=np.zeros((n_obj, max_maxima), np.int32), class_score=np.zeros((n_obj, n_classes)), bins=[])
    bs_all = votes.get("bbox_size")
    for o in range(n_obj):
        found = []
        for c in range(n_classes):
            sel = off[o] + np.flatnonzero(votes["cls"][off[o]:off[o + 1]] == c)
            if not len(sel):
                continue
            pos, w = votes["pos"][sel].astype(np.float64), votes["weight"][sel].astype(np.float64)
            cnt, H = accumulate(pos, w, min_coord, max_coord, class_bin[c] if class_bin is not None else bin_size, use_interpolation)
            for idx in find_maxima(cnt, H, float(rel_threshold)):
                vt = H[idx][1]
                if len(vt) < min_votes_threshold:
                    continue
                sw = w[vt].sum()
                inst, iw = best_instance(votes["inst"][sel[vt]], w[vt])
                bs = (bs_all[sel[vt]].astype(np.float64) * w[vt, None]).sum(0) / sw if bs_all is not None else np.zeros(3)
                found.append(dict(pos=(pos[vt] * w[vt, None]).sum(0) / sw, weight=sw, cls=c, inst=inst, inst_weight=iw, bbox_size=bs,
                                  n_votes=len(vt), bin=idx, value=H[idx][0]))
        found.sort(key=lambda m: -m["weight"])                        # stable: equal weights keep (class, bin index) order
        sw, siw = sum(m["weight"] for m in found), sum(m["inst_weight"] for m in found)
        out["bins"].append([(m["cls"], m["bin"], m["value"]) for m in found])
        for m in found:
            m["weight"] = m["weight"] / sw if sw else 0.0
            m["inst_weight"] = m["inst_weight"] / siw if siw else 0.0
            out["class_score"][o, m["cls"]] = max(out["class_score"][o, m["cls"]], m["weight"])
        out["n"][o] = min(len(found), max_maxima)
        for i, m in enumerate(found[:max_maxima]):
            for key in ("pos", "weight", "cls", "inst", "inst_weight", "bbox_size", "n_votes"):
                out[key][o, i] = m[key]
    return out
