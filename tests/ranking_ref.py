"""numpy float32 transcription of the reference's feature ranking (feature_ranking/*.cpp), the checker of ismhip_rank_scores and
ismhip_rank_select.

The four iComputeScores bodies are written as the reference writes them: one query after the other, float accumulation in that order.
`knn(metric, words, queries, k)` is the exact chi-square search (oracle_py.knn: ascending (distance, row), -1 / NaN past the end of a
small dataset), which stands for flann::Index<ChiSquareDistance>::knnSearch with SearchParams(-1).

The selection is rankFeaturesWithScores + extractSubsetFromRankedList (feature_ranking.cpp:121-203) with this project's DEFINED order
where the reference's unstable std::sort leaves it open: ascending by (score, index within the class), -0 equal to +0, NaN after +inf.
"""
import numpy as np

CHI2 = 1
f32 = np.float32
TYPES = ("KNNActivation", "Incremental", "Strangeness", "NaiveBayes")


def _all_knn(knn, desc, k):
    idx, dist = knn(CHI2, desc, desc, k)
    return idx, dist.astype(np.float32)


def _increment(inc):
    inc = 1 if inc == 0 else inc                     # ranking_knn_activation.cpp:88
    return inc if 1 <= inc <= 3 else 1               # :91-95


def knn_activation(knn, desc, off, k_search, increment_type=0):
    """ranking_knn_activation.cpp:53-110 with UseFeaturePosition false (score_dist_rate = 1)"""
    inc = _increment(increment_type)
    idx, dist = _all_knn(knn, desc, k_search + 1)
    score = np.zeros(len(desc), np.float32)
    with np.errstate(all="ignore"):
        for q in range(len(desc)):
            m = int((idx[q] >= 0).sum())
            for j in range(m - 1):                   # :74: all but the LAST result
                t, d = idx[q, j], dist[q, j]
                if inc == 1:
                    score[t] = f32(score[t] + f32(1))
                elif inc == 2:
                    score[t] = f32(score[t] + f32(f32(1) / f32(d + f32(1))))
                else:
                    score[t] = f32(score[t] + f32(np.exp(d)))
    return score


def knn_activation_exp_f64(knn, desc, k_search):
    """increment type 3 in float64: (sum of exp(d), sum of |terms|, number of terms) per feature"""
    idx, dist = _all_knn(knn, desc, k_search + 1)
    n = len(desc)
    s = np.zeros(n, np.float64); a = np.zeros(n, np.float64); t = np.zeros(n, np.int64)
    for q in range(n):
        m = int((idx[q] >= 0).sum())
        for j in range(m - 1):
            e = np.exp(np.float64(dist[q, j]))
            s[idx[q, j]] += e; a[idx[q, j]] += abs(e); t[idx[q, j]] += 1
    return s, a, t


def incremental(knn, desc, off, k_search):
    """ranking_incremental.cpp:51-84"""
    idx, dist = _all_knn(knn, desc, k_search + 1)
    score = np.zeros(len(desc), np.float32)
    for q in range(len(desc)):
        m = int((idx[q] >= 0).sum())
        for j in range(m - 1):
            score[idx[q, j]] = f32(score[idx[q, j]] + f32(dist[q, j] - dist[q, j + 1]))
    return score


def strangeness(knn, desc, off, k_search):
    """ranking_strangeness.cpp:58-93; an empty class contributes the sum of an empty list"""
    n, C = len(desc), len(off) - 1
    sums = np.zeros((n, C), np.float32)
    for c in range(C):
        rows = desc[off[c]:off[c + 1]]
        if len(rows) == 0:
            continue
        idx, dist = knn(CHI2, rows, desc, k_search)
        for q in range(n):
            s = f32(0)
            for j in range(k_search):
                if idx[q, j] >= 0:
                    s = f32(s + f32(dist[q, j]))     # :76-80
            sums[q, c] = s
    score = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for c in range(C):
            for q in range(off[c], off[c + 1]):
                all_sums = sums[q].copy()
                own = all_sums[c]
                all_sums[c] = -1                      # :85
                all_sums.sort()
                score[q] = f32(own / all_sums[1])     # :87
    return score


def naive_bayes(knn, desc, off, k_search, dist_threshold):
    """ranking_naive_bayes.cpp:52-79 with findSimilarFeaturesFlann (feature_ranking.cpp:346-363)"""
    n, C = len(desc), len(off) - 1
    thr = f32(dist_threshold)
    score = np.zeros(n, np.float32)

    def similar(rows, queries):
        if len(rows) == 0 or len(queries) == 0:
            return np.zeros(len(queries), np.int64)
        idx, dist = knn(CHI2, rows, queries, k_search)
        return ((idx >= 0) & (dist.astype(np.float32) < thr)).sum(1)

    with np.errstate(all="ignore"):
        for c in range(C):
            cur = desc[off[c]:off[c + 1]]
            other = np.concatenate([desc[:off[c]], desc[off[c + 1]:]])      # createCloudWithClassIds(..., inverse): global row order
            neg, pos = similar(other, cur), similar(cur, cur)
            num_current, num_other = f32(len(cur)), f32(len(other))
            for i in range(len(cur)):
                num_pos, num_neg = f32(pos[i]), f32(neg[i])
                pos_prob = f32(num_pos / num_current)
                score[off[c] + i] = f32(pos_prob / f32(f32(num_pos + num_neg) / f32(num_current + num_other)))
    return score


def scores(knn, rank_type, desc, off, k_search, dist_threshold=0.1, increment_type=0):
    desc = np.ascontiguousarray(desc, np.float32)
    off = [int(o) for o in off]
    if rank_type == "KNNActivation":
        return knn_activation(knn, desc, off, k_search, increment_type)
    if rank_type == "Incremental":
        return incremental(knn, desc, off, k_search)
    if rank_type == "Strangeness":
        return strangeness(knn, desc, off, k_search)
    if rank_type == "NaiveBayes":
        return naive_bayes(knn, desc, off, k_search, dist_threshold)
    raise ValueError(rank_type)


def ranked_order(score):
    """indices of one class in ascending (score, index) order: -0 == +0 (a float comparison), NaN after +inf"""
    s = np.asarray(score, np.float32)
    nan = np.isnan(s)
    val = np.where(nan, np.float32(0), s).astype(np.float64) + 0.0      # -0.0 + 0.0 = +0.0
    return np.lexsort((np.arange(len(s)), val, nan))


def select(score, off, factor, extract_offset):
    """-> (keep [n] uint8, n_keep [n_classes] uint32)"""
    score = np.asarray(score, np.float32)
    factor, extract_offset = f32(factor), f32(extract_offset)
    keep = np.zeros(len(score), np.uint8)
    n_keep = np.zeros(len(off) - 1, np.uint32)
    for c in range(len(off) - 1):
        b, e = int(off[c]), int(off[c + 1])
        s = e - b
        min_index = f32(f32(s) * extract_offset)                        # feature_ranking.cpp:179-185
        max_index = f32(f32(s) * f32(factor + extract_offset))
        if min_index < 0:
            min_index = f32(0)
        if max_index > f32(s):
            max_index = f32(s)
        order = ranked_order(score[b:e])
        for j in range(s):
            if f32(j) >= min_index and f32(j) < max_index:              # :191
                keep[b + order[j]] = 1
                n_keep[c] += 1
    return keep, n_keep


def extract_offset_from_list(extract_list, factor, extract_offset=0.0):
    """the deprecated ExtractFromList (feature_ranking.cpp:135-148): float = double expression, as the reference assigns it"""
    factor = f32(factor)
    if extract_list == "front":
        return f32(0)
    if extract_list in ("center", "middle"):
        return f32(0.5 * (1 - np.float64(factor)))
    if extract_list == "back":
        return f32(1.0 - np.float64(factor))
    return f32(extract_offset)
