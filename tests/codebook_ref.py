"""Float64 references of the codebook stage, numpy only: Codebook::activate after the activation step (codebook.cpp:64-368 with
codeword_distribution.cpp:37-71 addCodeword and :169-243 computeWeights) and CodewordDistribution::castVotes (:73-167).

The inputs are the float32 arrays the library gets, taken as exact values; every real-valued result is evaluated in float64 in the
reference's formulas (the quaternion of an LRF is NOT normalised, as in utils.cpp:342-394). Integer outputs are exact. What depends
on a float32 comparison is reported with its margin, so that a test can tell a decided case from an undecided one:
  * every median comes with min_move, the smallest change it would take if either middle rank moved by one place,
  * every LRF comes with `near_tie`, the distance of its trace from the branch it did not take,
  * every cast vote comes with |d| - 2 sigma and weight - FLT_EPSILON.
The class weights are int-to-float conversions, divisions and products only, so they are also restated in numpy float32 in the
reference's operation order: that copy is what a float32 implementation must give bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64
FLT_EPSILON = float(np.finfo(f32).eps)
W_CLASS, W_VOTE, W_MATCHING, W_CODEWORD = 1, 2, 4, 8
SAMPLE_ABOVE = 4096                    # words with more votes are evaluated at a fixed sample of their votes
SAMPLE_STEP = 128


# ------------------------------------------------------------------------------------------------------------ quaternions
def rot_quaternion(l9, trace_ge=False, diag_ge=False):
    """Utils::getRotQuaternion + matrix2Quat (rows of the matrix = the LRF axes) in float64 -> ((w, x, y, z), near_tie).
    near_tie = |trace|, the only rounded quantity a branch depends on: the diagonal comparisons are between input values, which
    float32 and float64 order alike, and a trace of exactly 0 is exact in float32 too. 0 < near_tie < a few float32 roundings of
    the diagonal means that a float32 evaluation may take the other branch (it then describes the same rotation).
    trace_ge / diag_ge evaluate a WRONG variant (`trace >= 0`, `>=` on the diagonal) so that a test can show which frames tell the
    strict comparisons from the lax ones: the rotation is the same, the SIGN of the quaternion is not."""
    m = np.asarray(l9, f64).reshape(3, 3)
    q = [0.0, 0.0, 0.0, 1.0]                                   # x, y, z, w
    trace = m[0, 0] + m[1, 1] + m[2, 2]
    near = abs(trace)
    if trace > 0.0 or (trace_ge and trace == 0.0):
        root = np.sqrt(trace + 1.0)
        q[3] = 0.5 * root
        root = 0.5 / root
        q[0] = (m[2, 1] - m[1, 2]) * root
        q[1] = (m[0, 2] - m[2, 0]) * root
        q[2] = (m[1, 0] - m[0, 1]) * root
    else:
        i = 0
        if m[1, 1] > m[0, 0] or (diag_ge and m[1, 1] == m[0, 0]):
            i = 1
        if m[2, 2] > m[i, i] or (diag_ge and m[2, 2] == m[i, i]):
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        root = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * root
        root = 0.5 / root
        q[3] = (m[k, j] - m[j, k]) * root
        q[j] = (m[j, i] + m[i, j]) * root
        q[k] = (m[k, i] + m[i, k]) * root
    return np.array([q[3], q[0], q[1], q[2]], f64), float(near)


def qmul(a, b):
    """boost::math::quaternion operator* on [..., 4] arrays (w, x, y, z)"""
    aw, ax, ay, az = np.moveaxis(np.asarray(a, f64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, f64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def qconj(q):
    return np.asarray(q, f64) * np.array([1.0, -1.0, -1.0, -1.0])


def frames(lrf):
    """per LRF: quaternion [n, 4], near_tie [n], and the two linear maps of the (unnormalised) quaternion as matrices:
    into[f] @ v = q v conj(q) (rotateInto), back[f] @ v = conj(q) v q (rotateBack)"""
    lrf = np.asarray(lrf, f32).reshape(-1, 9)
    n = len(lrf)
    q = np.empty((n, 4)); near = np.empty(n)
    uniq = {}
    for f in range(n):
        key = lrf[f].tobytes()
        if key not in uniq:
            uniq[key] = rot_quaternion(lrf[f])
        q[f], near[f] = uniq[key]
    basis = np.concatenate([np.zeros((3, 1)), np.eye(3)], 1)                       # pure quaternions of the unit vectors
    qb, cb = q[:, None, :], qconj(q)[:, None, :]
    into = np.swapaxes(qmul(qmul(qb, basis[None]), cb)[..., 1:], 1, 2)             # columns = images of the unit vectors
    back = np.swapaxes(qmul(qmul(cb, basis[None]), qb)[..., 1:], 1, 2)
    return q, near, into, back


# -------------------------------------------------------------------------------------------------------------- training
def sigma_samples(cls, model, act_off, n_classes):
    """the sigma^2 sample of every class (codebook.cpp:94-193): (features, first activation, number of activations) or None for a
    class without features. Words: whole lists of the class's first features, the count checked BEFORE each list; features: whole
    models, the count checked before each model."""
    out = []
    cls = np.asarray(cls); model = np.asarray(model)
    for c in range(n_classes):
        fs = np.nonzero(cls == c)[0]
        if len(fs) == 0:
            out.append(None)
            continue
        assert np.array_equal(fs, np.arange(fs[0], fs[0] + len(fs))), "features must be class-major"
        me = int(np.sqrt(float(len(fs))))
        words = 0; t = 0
        while t < len(fs) and words < me:
            words += int(act_off[fs[t] + 1] - act_off[fs[t]]); t += 1
        sf = []; t = 0
        while t < len(fs) and len(sf) < me:
            e = t
            while e < len(fs) and model[fs[e]] == model[fs[t]]:
                e += 1
            sf.extend(fs[t:e]); t = e
        out.append((np.asarray(sf, np.int64), int(act_off[fs[0]]), words))
    return out


def distance64(metric, a, b):
    """the FLANN functors (utils/distance.h) in float64 on float32 rows; chi-square skips x + y <= 0"""
    a = np.asarray(a, f64); b = np.asarray(b, f64)
    if metric == 1:
        s = a + b
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(s > 0, (a - b) ** 2 / np.where(s > 0, s, 1.0), 0.0)
        return t.sum(-1)
    return ((a - b) ** 2).sum(-1)


def variance_of(d):
    """the reference's sample variance of a list in its own arithmetic (IEEE: an empty list gives 0 / (0 - 1) = -0.0, one entry
    0 / 0 = NaN)"""
    num = len(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = f64(np.sum(d)) / f64(num)
        var = f64(np.sum((d - mean) ** 2)) if num else f64(0.0)
        return var / f64(num - 1)


def median_and_move(w):
    """median of a list as computeWeights takes it (:228-240) and the smallest change it would take if either middle rank moved by
    one place (inf for a single entry)"""
    s = np.sort(w, axis=-1)
    m = s.shape[-1]
    h = m // 2
    if m == 1:
        return s[..., 0], np.full(s.shape[:-1], np.inf)
    if m % 2:
        return s[..., h], np.minimum(s[..., h] - s[..., h - 1], s[..., h + 1] - s[..., h])
    med = (s[..., h - 1] + s[..., h]) / 2
    move = (s[..., h] - s[..., h - 1]) / 2
    if m > 2:
        move = np.minimum(move, np.minimum(s[..., h - 1] - s[..., h - 2], s[..., h + 1] - s[..., h]) / 2)
    return med, move


def sample_of(m):
    """votes of a word at which the reference evaluates the weights: all, or above SAMPLE_ABOVE the first, the middle, the last and
    every SAMPLE_STEP-th"""
    if m <= SAMPLE_ABOVE:
        return np.arange(m)
    return np.unique(np.concatenate([np.arange(0, m, SAMPLE_STEP), [0, m // 2, m - 1]]))


def class_weights(word_class_runs, n_classes, dtype):
    """steps 3-9 of Codebook::activate (codebook.cpp:226-368) in `dtype` arithmetic. word_class_runs: per kept word the list of
    (class, votes) in ascending class order. -> (term1 [C], term2 [words], term3 [C]); m_term3 is keyed by class only, so the LAST
    word holding the class wins (:325-339)."""
    one = dtype(1.0)
    num_features = np.zeros(n_classes, np.int64); words_per_class = np.zeros(n_classes, np.int64)
    for runs in word_class_runs:
        for c, k in runs:
            num_features[c] += k; words_per_class[c] += 1
    term1 = np.zeros(n_classes, dtype); term3 = np.zeros(n_classes, dtype)
    term2 = np.empty(len(word_class_runs), dtype)
    for c in range(n_classes):
        if words_per_class[c]:
            term1[c] = one / dtype(words_per_class[c])
    for e, runs in enumerate(word_class_runs):
        term2[e] = one / dtype(sum(k for _, k in runs))
        total = None
        for c, k in runs:
            t = dtype(k) / dtype(num_features[c])
            total = t if total is None else dtype(total + t)
        for c, k in runs:
            term3[c] = dtype(dtype(dtype(k) / dtype(num_features[c])) / total)
    return term1, term2, term3


def train_from_lists(metric, desc, lrf, kp, cls, model, centre, act_off, act_idx, n_classes, codewords=None, clean_up=False):
    """Codebook::activate after the activation step. act_off [n+1], act_idx [n_act]: the codeword rows every feature activates, in
    order. -> dict: word_src, vote_offsets, vote_feature (exact); vote_xyz, vote_weight, min_move, class_sigma, vote_class_weight
    (float64); vote_class_weight32 (numpy float32, the reference's operation order); evaluated [votes] (False: the vote of a word above
    SAMPLE_ABOVE votes that is not in the sample: vote_weight NaN there); near_tie [n] of the LRFs."""
    desc = np.asarray(desc, f32); kp = np.asarray(kp, f32); centre = np.asarray(centre, f32)
    cls = np.asarray(cls, np.int64); act_off = np.asarray(act_off, np.int64); act_idx = np.asarray(act_idx, np.int64)
    n = len(desc)
    words = desc if codewords is None else np.asarray(codewords, f32)
    ncw = len(words)
    assert act_off[0] == 0 and act_off[-1] == len(act_idx) and len(act_off) == n + 1
    assert len(act_idx) == 0 or (act_idx.min() >= 0 and act_idx.max() < ncw)
    feat_of = np.repeat(np.arange(n), np.diff(act_off))
    # distributions: the votes of a word in activation order; K = 1 clean-up keeps the words with exactly one vote (:201-224)
    order = np.argsort(act_idx, kind="stable")
    cnt = np.bincount(act_idx, minlength=ncw)
    keep = (cnt == 1) if clean_up else (cnt > 0)
    word_src = np.nonzero(keep)[0]
    sel = order[keep[act_idx[order]]]
    vote_feature = feat_of[sel]
    vote_offsets = np.concatenate([[0], np.cumsum(cnt[word_src])])
    q, near, into, back = frames(lrf)
    diff = centre.astype(f64) - kp.astype(f64)
    vote_xyz = np.einsum("vab,vb->va", into[vote_feature], diff[vote_feature])
    # computeWeights: median over the activating features j of exp(-|kp_j + rotateBack(vote_i, LRF_j) - centre_i|^2 / 0.25)
    nv = len(vote_feature)
    vote_weight = np.full(nv, np.nan); min_move = np.full(nv, np.nan); evaluated = np.zeros(nv, bool)
    for e in range(len(word_src)):
        v0, v1 = vote_offsets[e], vote_offsets[e + 1]
        m = v1 - v0
        fj = vote_feature[v0:v1]
        rows = sample_of(m)
        step = max(1, (1 << 21) // m)
        for r0 in range(0, len(rows), step):
            vi = v0 + rows[r0:r0 + step]
            c = kp[fj].astype(f64)[None] + np.einsum("jab,ib->ija", back[fj], vote_xyz[vi])
            d2 = ((c - centre[vote_feature[vi]].astype(f64)[:, None, :]) ** 2).sum(-1)
            vote_weight[vi], min_move[vi] = median_and_move(np.exp(-d2 / 0.25))
            evaluated[vi] = True
    # class sigma^2
    class_sigma = np.full(n_classes, np.nan)
    for c, s in enumerate(sigma_samples(cls, model, act_off, n_classes)):
        if s is None:
            continue
        sf, a0, nw = s
        sw = act_idx[a0:a0 + nw]
        d = distance64(metric, desc[sf][:, None, :], words[sw][None, :, :]).reshape(-1) if len(sf) * nw else np.zeros(0)
        class_sigma[c] = variance_of(d)
    # statistical class weights
    vcls = cls[vote_feature]
    runs = []
    for e in range(len(word_src)):
        vc = vcls[vote_offsets[e]:vote_offsets[e + 1]]
        assert np.all(np.diff(vc) >= 0)
        u, k = np.unique(vc, return_counts=True)
        runs.append(list(zip(u.tolist(), k.tolist())))
    vote_word = np.repeat(np.arange(len(word_src)), np.diff(vote_offsets))
    out = dict(word_src=word_src.astype(np.uint32), vote_offsets=vote_offsets.astype(np.uint32), vote_feature=vote_feature.astype(np.uint32),
               vote_xyz=vote_xyz, vote_weight=vote_weight, min_move=min_move, evaluated=evaluated, class_sigma=class_sigma, near_tie=near,
               quat=q)
    for key, dt in (("vote_class_weight", f64), ("vote_class_weight32", f32)):
        t1, t2, t3 = class_weights(runs, n_classes, dt)
        out[key] = ((t1[vcls] * t2[vote_word]) * t3[vcls]).astype(dt) if nv else np.zeros(0, dt)
        out["term3" if dt is f64 else "term3_32"] = t3
    return out


# ----------------------------------------------------------------------------------------------------------- vote casting
def cast_votes_ref(cb, flags, lrf, kp, feat_of_act, idx, dist):
    """CodewordDistribution::castVotes for a flat list of activations (activation a of feature feat_of_act[a] names codeword idx[a]
    at functor value dist[a]); slot = a * max_votes + (vote - first vote of the word). cb: dict with vote_offsets, vote_xyz, vote_class,
    vote_instance, class_sigma and optionally word_weight, vote_weight, vote_class_weight, vote_bbox_quat, vote_bbox_size.
    -> dict: live, cls, inst, codeword (exact), weight (float32: the product in flag order, the matching term in float64 rounded once),
    pos, bbox_quat (float64), bbox_size, margin_sigma = |d| - 2 sigma and margin_eps = weight - FLT_EPSILON per slot (NaN where the
    slot's word has no such vote), matching_margin = the relative distance of the float64 matching term from the nearest value at
    which its float32 rounding changes (NaN where it is not evaluated), near_tie per activation."""
    vo = np.asarray(cb["vote_offsets"], np.int64)
    n_words = len(vo) - 1
    maxv = int(np.diff(vo).max()) if n_words else 0
    sig = np.asarray(cb["class_sigma"], f32)
    idx = np.asarray(idx, np.int64); dist = np.asarray(dist, f32); feat_of_act = np.asarray(feat_of_act, np.int64)
    kp = np.asarray(kp, f32)
    q, near, into, back = frames(lrf)
    ns = len(idx) * maxv
    out = dict(live=np.zeros(ns, bool), cls=np.full(ns, -1, np.int32), inst=np.full(ns, -1, np.int32), codeword=np.full(ns, -1, np.int32),
               weight=np.zeros(ns, f32), pos=np.zeros((ns, 3)), bbox_quat=np.tile([1.0, 0.0, 0.0, 0.0], (ns, 1)), bbox_size=np.zeros((ns, 3), f32),
               margin_sigma=np.full(ns, np.nan), margin_eps=np.full(ns, np.nan), matching_margin=np.full(ns, np.nan), near_tie=near[feat_of_act] if len(idx) else np.zeros(0))
    opt = lambda k: None if cb.get(k) is None else np.asarray(cb[k], f32)
    ww, vw, vcw, vbq, vbs = opt("word_weight"), opt("vote_weight"), opt("vote_class_weight"), opt("vote_bbox_quat"), opt("vote_bbox_size")
    vxyz = np.asarray(cb["vote_xyz"], f32).astype(f64)
    one = f32(1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for a in range(len(idx)):
            c = idx[a]
            if c < 0 or c >= n_words:
                continue
            f = feat_of_act[a]; d = dist[a]
            for v in range(vo[c], vo[c + 1]):
                s = a * maxv + (v - vo[c])
                k = int(cb["vote_class"][v])
                sg = sig[k] if k < len(sig) else one                                         # :108-117
                w = one
                if flags & W_CLASS:
                    w = f32(w * (vcw[v] if vcw is not None else one))
                if flags & W_VOTE:
                    w = f32(w * (vw[v] if vw is not None else one))
                if flags & W_MATCHING:
                    sg64, d64 = f64(sg), f64(d)
                    m64 = (1.0 / np.sqrt(2.0 * np.pi * sg64)) * np.exp(-(d64 * d64) / (2.0 * sg64))
                    m32 = f32(m64)
                    if np.isfinite(m64) and m64 != 0:
                        edges = [(f64(m32) + f64(np.nextafter(m32, f32(t)))) / 2 for t in (-np.inf, np.inf)]
                        out["matching_margin"][s] = min(abs(m64 - e) for e in edges) / abs(m64)
                    w = f32(w * m32)
                if flags & W_CODEWORD:
                    w = f32(w * (ww[c] if ww is not None else one))
                out["margin_sigma"][s] = f64(abs(d)) - 2.0 * f64(sg)
                out["margin_eps"][s] = f64(w) - FLT_EPSILON
                if abs(d) > f32(2) * sg:                                                     # :131 (NaN sigma: not dropped)
                    continue
                if w < f32(FLT_EPSILON):                                                     # :137 (NaN weight: not dropped)
                    continue
                out["live"][s] = True
                out["pos"][s] = kp[f].astype(f64) + back[f] @ vxyz[v]
                out["weight"][s] = w; out["cls"][s] = k; out["inst"][s] = int(cb["vote_instance"][v]); out["codeword"][s] = c
                b = vbq[v].astype(f64) if vbq is not None else np.array([1.0, 0.0, 0.0, 0.0])
                out["bbox_quat"][s] = qmul(b, q[f])                                          # :162
                if vbs is not None:
                    out["bbox_size"][s] = vbs[v]
    return out
