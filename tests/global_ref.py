"""Restatement of the reference's global-descriptor verification in numpy, written from its text:

  * FeaturesSHORTSHOTGlobal::compute_descriptor / configureSphericalGrid (features/features_short_shot_global.cpp:94-249): float32 for
    v = p - c and the three frame dot products (unfused, in short_shot_ref.py's order), float64 for everything after, +1 per point, no
    interpolation; Features::getCloudRadius (features.cpp:128-151) and pcl::compute3DCentroid for the keypoint and the radius;
  * GlobalClassifier::classifyWithKNN, mergeGlobalAndLocalHypotheses (functions 1 .. 7), useHighRankedGlobalHypothesis
    (classifier/global_classifier.cpp:242-347, 457-601) and the merge sequence of Voting::findMaxima (voting/voting.cpp:272-323) with
    normalizeWeights (:441-462), in float32 where the reference holds floats.

The device and the host's libm may differ by a few ulp of double (~1e-13 in raw bin units), so the counts are returned as an INTERVAL: a
point is UNDECIDED when one of its three raw bin coordinates lies within EPS of an integer at which its bin changes, or when its 1e-15
test or a selection test is not clear by a relative EPS; undecided points count in `upper` only, in every bin they could reach.
EPS = 1e-9 is the margin test_short_shot_cpu.py holds the local descriptor's scenes to (switch_margin >= 1e-9 raw units)."""
import numpy as np

f32, f64 = np.float32, np.float64
RAD2DEG = 57.29578                       # pcl::rad2deg(double), PCL 1.10 common/impl/angles.hpp
EPS = 1e-9
# configureSphericalGrid (:171-226): 64 is (4, 2, 8) here, (2, 4, 8) in the local descriptor
AUTO_BINS = {8: (1, 1, 8), 16: (2, 2, 4), 24: (2, 2, 6), 32: (2, 2, 8), 64: (4, 2, 8), 96: (3, 4, 8), 128: (4, 4, 8), 192: (6, 4, 8), 256: (8, 4, 8)}


def configure_spherical_grid(dims=32, bin_type="auto", bins=(1, 1, 8)):
    """configureSphericalGrid (:168-249) -> (dims, (r, e, a))"""
    if bin_type == "auto":
        return (dims, AUTO_BINS[dims]) if dims in AUTO_BINS else (32, (2, 2, 8))
    if bin_type == "manual":
        return bins[0] * bins[1] * bins[2], tuple(bins)
    return 32, (2, 2, 8)


def _sqdist(p, c):
    """the unfused float32 (dx*dx + dy*dy) + dz*dz of every ball sweep"""
    v = (np.asarray(p, f32) - np.asarray(c, f32)[None, :]).astype(f32)
    return ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(f32) + v[:, 2] * v[:, 2]).astype(f32), v


def r2_of(radius):
    """PCL: static_cast<float>(radius * radius) with a double radius"""
    return f32(f64(f32(radius)) * f64(f32(radius)))


def select(points, center=None, radius=-1.0):
    """the region's points: the finite ones, and with radius >= 0 those with d2 < (float)((double)radius * radius) to the centre"""
    p = np.asarray(points, f32).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    if radius is None or radius < 0:
        return p
    d2, _ = _sqdist(p, center)
    return p[d2 < r2_of(radius)]


def centroid_radius(sel):
    """pcl::compute3DCentroid (double sums, cast to float) and getCloudRadius (float norm, max) of the selected points"""
    if len(sel) == 0:
        return np.full(3, np.nan, f32), f32(0)
    c = (sel.astype(f64).sum(0) / f64(len(sel))).astype(f32)
    d2, _ = _sqdist(sel, c)
    return c, f32(np.sqrt(d2).max())


def row_of_counts(counts):
    """count / sqrt(sum count^2) in double, cast to float32 (:151-161); all zero gives 0 / 0: NaN"""
    c = np.asarray(counts, f64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (c / np.sqrt((c * c).sum(-1, keepdims=True))).astype(f32)


def _raw(v, frame, R, bins, min_radius, log_radius):
    """the three float64 raw bin coordinates of the float32 offsets v"""
    rb, eb, ab = bins
    frame = np.asarray(frame, f32).reshape(3, 3)
    dot = lambda ax: ((v[:, 0] * ax[0] + v[:, 1] * ax[1]).astype(f32) + v[:, 2] * ax[2]).astype(f32).astype(f64)
    xl, yl, zl = dot(frame[0]), dot(frame[1]), dot(frame[2])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt((xl * xl + yl * yl) + zl * zl)
        theta = np.arccos(zl / r) * RAD2DEG
        phi = np.arctan2(yl, xl) * RAD2DEG
        if log_radius:
            raw_r = ((rb - 1) * (np.log(r) - np.log(f64(min_radius)))) / np.log(f64(R) / f64(min_radius)) + 1
        else:
            raw_r = (rb * r) / f64(R)
        return raw_r, (eb * theta) / 180, (ab * (phi + 180)) / 360


def _bin(raw, n, clamp_low):
    """int() (towards zero; NaN and out-of-range as x86-64's INT_MIN) and the reference's clamps"""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(raw) & (np.abs(raw) < 2147483648.0)
        b = np.where(ok, np.trunc(np.where(ok, raw, 0.0)), -2147483648.0).astype(np.int64)
    if clamp_low:
        b = np.maximum(b, 0)
    return np.minimum(b, n - 1)


def short_shot_global_counts(sel, centroid, R, frame, bins=(2, 2, 8), min_radius=0.1, log_radius=False, eps=EPS, sel_d2=None, sel_r2=None):
    """The integer histogram of one region from the selected points sel [n, 3], the keypoint `centroid`, the radius R and the frame [9]
    (the caller passes the device's own: they are outputs of the same call, held to the oracle separately).
    -> (counts, lower, upper, n_undecided): counts takes every decision at face value. sel_d2 / sel_r2: the points' squared distance to
    a selection centre and the selection's r2, when the caller wants points within eps of the selection boundary treated as undecided
    (sel must then hold the points on both sides of it)."""
    rb, eb, ab = bins
    D = rb * eb * ab
    sel = np.asarray(sel, f32).reshape(-1, 3)
    zero = np.zeros(D, np.int64)
    if len(sel) == 0 or not np.isfinite(np.asarray(frame, f32)).all():
        return zero, zero.copy(), zero.copy(), 0
    d2, v = _sqdist(sel, centroid)
    r2 = r2_of(R)
    inside = d2 < r2
    use = inside & (d2.astype(f64) > 1e-15)
    if sel_d2 is not None:
        use &= sel_d2 < sel_r2
    raws = _raw(v, frame, R, bins, min_radius, log_radius)
    b = [_bin(raws[0], rb, True), _bin(raws[1], eb, False), _bin(raws[2], ab, False)]
    valid = use & (b[1] >= 0) & (b[2] >= 0)
    idx = b[0] + b[1] * rb + b[2] * rb * eb
    counts = np.bincount(idx[valid], minlength=D).astype(np.int64)
    # undecided points
    und = np.abs(d2.astype(f64) - f64(r2)) <= eps * f64(r2)
    und |= np.abs(d2.astype(f64) - 1e-15) <= eps * 1e-15
    if sel_d2 is not None:
        und |= np.abs(sel_d2.astype(f64) - f64(sel_r2)) <= eps * f64(sel_r2)
    near = []
    for raw, n in zip(raws, (rb, eb, ab)):
        with np.errstate(invalid="ignore"):
            k = np.rint(raw)
            near.append(np.isfinite(raw) & (np.abs(raw - k) <= eps) & (k >= 1) & (k <= n - 1))
    und |= (near[0] | near[1] | near[2]) & inside
    if sel_d2 is not None:                       # a point clearly outside the selection is decided: it counts nowhere
        und &= sel_d2.astype(f64) < f64(sel_r2) * (1 + eps)
    lower = np.bincount(idx[valid & ~und], minlength=D).astype(np.int64)
    upper = lower.copy()
    for i in np.nonzero(und)[0]:
        reach = set()
        for sr in (-eps, eps):
            for st in (-eps, eps):
                for sp in (-eps, eps):
                    br = _bin(np.array([raws[0][i] + sr]), rb, True)[0]
                    bt = _bin(np.array([raws[1][i] + st]), eb, False)[0]
                    bp = _bin(np.array([raws[2][i] + sp]), ab, False)[0]
                    if bt >= 0 and bp >= 0:
                        reach.add(int(br + bt * rb + bp * rb * eb))
        for j in reach:
            upper[j] += 1
    return counts, lower, upper, int(und.sum())


def short_shot_global(points, frame=None, center=None, radius=-1.0, bins=(2, 2, 8), min_radius=0.1, log_radius=False):
    """one region end to end on the host: -> dict(n_sel, centroid, radius, counts, row); frame: [9] (the caller's)"""
    sel = select(points, center, radius)
    c, R = centroid_radius(sel)
    counts, lower, upper, und = short_shot_global_counts(sel, c, R, frame, bins, min_radius, log_radius)
    return dict(n_sel=len(sel), centroid=c, radius=R, counts=counts, lower=lower, upper=upper, undecided=und, row=row_of_counts(counts))


# ---- the host sequence ------------------------------------------------------------------------------------------------------------

def knn_score(dist):
    """float score = std::exp(-sqrt(dist_squared)) on a float: sqrtf, then expf (the host's libm: compare to 1e-6 relative)"""
    return f32(np.exp(f32(-np.sqrt(f32(dist)))))


def classify_with_knn(neighbour_class, neighbour_instance, neighbour_dist, max_class, single_object_mode):
    """classifyWithKNN (:242-347) on the neighbours of ONE query, in the search's order -> (classId, classWeight, instanceId, instanceWeight).
    std::map order: ties in the occurrence counts go to the lowest id."""
    acc = {}
    for c, i, d in zip(neighbour_class, neighbour_instance, neighbour_dist):
        s = knn_score(d)
        a = acc.setdefault(int(c), dict(n=0, s=f32(0), inst={}))
        a["n"] += 1
        a["s"] = f32(a["s"] + s)
        e = a["inst"].setdefault(int(i), [0, f32(0)])
        e[0] += 1
        e[1] = f32(e[1] + s)
    cls, cw, inst, iw = int(max_class), f32(0), 0, f32(0)

    def best_instance(a):
        best, bid = 0, 0
        for k in sorted(a["inst"]):
            if a["inst"][k][0] > best:
                best, bid = a["inst"][k][0], k
        e = a["inst"][bid]
        return bid, f32(e[1] / f32(e[0]))

    if single_object_mode:
        best = 0
        for c in sorted(acc):
            if acc[c]["n"] > best:
                best, cls = acc[c]["n"], c
        a = acc[cls]
        cw = f32(a["s"] / f32(a["n"]))
        inst, iw = best_instance(a)
    elif cls in acc:
        a = acc[cls]
        cw = f32(a["s"] / f32(a["n"]))
        inst, iw = best_instance(a)
    return cls, cw, inst, iw


def zero_hypothesis(max_class, max_instance):
    """classify() below GlobalFeatureMinPoints (:229-239)"""
    return int(max_class), f32(0), int(max_instance), f32(0)


class Maximum:
    """the fields of VotingMaximum that the merge sequence reads and writes"""

    def __init__(self, cls, weight, inst, inst_weight, pos=(0, 0, 0), g=(0, 0, 0, 0), roi_centroid=(0, 0, 0)):
        self.cls, self.weight, self.inst, self.inst_weight = int(cls), f32(weight), int(inst), f32(inst_weight)
        self.pos = np.asarray(pos, f32)
        self.g_cls, self.g_weight, self.g_inst, self.g_inst_weight = int(g[0]), f32(g[1]), int(g[2]), f32(g[3])
        self.roi = np.asarray(roi_centroid, f32)          # this maximum's own region centroid (zeros in single-object mode)

    def key(self):
        return (self.cls, float(self.weight), self.inst, float(self.inst_weight), self.g_cls, float(self.g_weight), self.g_inst, float(self.g_inst_weight))


def normalize_weights(maxima):
    """normalizeWeights (:441-462): four float sums in list order, each weight divided by its sum (0 when the sum is 0)"""
    s = [f32(0)] * 4
    for m in maxima:
        s = [f32(s[0] + m.weight), f32(s[1] + m.inst_weight), f32(s[2] + m.g_weight), f32(s[3] + m.g_inst_weight)]
    for m in maxima:
        m.weight = f32(m.weight / s[0]) if s[0] != 0 else f32(0)
        m.inst_weight = f32(m.inst_weight / s[1]) if s[1] != 0 else f32(0)
        m.g_weight = f32(m.g_weight / s[2]) if s[2] != 0 else f32(0)
        m.g_inst_weight = f32(m.g_inst_weight / s[3]) if s[3] != 0 else f32(0)


def _use_high_ranked(maxima, rate_limit):
    top, gcls = maxima[0].weight, maxima[0].g_cls
    lim = f32(top * f32(rate_limit))
    for m in maxima:
        if m.weight >= lim and m.cls == gcls:
            maxima[0].cls, maxima[0].inst = maxima[0].g_cls, maxima[0].g_inst
            break
        elif m.weight < lim:
            break


def _norm3(v):
    v = np.asarray(v, f32)
    return f32(np.sqrt(f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))


def merge_hypotheses(fn, maxima, radius, min_svm_score=0.70, rate_limit=0.60, weight_factor=1.5):
    """mergeGlobalAndLocalHypotheses (:457-577) on a non-empty list sorted by weight"""
    wf = f32(weight_factor)
    if fn == 1:
        if maxima[0].g_weight > f32(min_svm_score):
            maxima[0].cls, maxima[0].inst = maxima[0].g_cls, maxima[0].g_inst
    elif fn == 2:
        if maxima[0].g_weight > f32(min_svm_score):
            _use_high_ranked(maxima, rate_limit)
    elif fn == 3:
        _use_high_ranked(maxima, rate_limit)
    elif fn in (4, 5, 7):
        for m in maxima:
            near = _norm3(m.roi) == 0 or _norm3(m.pos - m.roi) < f32(f32(radius) / f32(2))
            if fn == 4:
                if m.cls == m.g_cls and near:
                    m.weight = f32(0) if m.g_weight == 0 else f32(m.weight * wf)
                if m.inst == m.g_inst and near:
                    m.inst_weight = f32(0) if m.g_inst_weight == 0 else f32(m.inst_weight * wf)
            elif fn == 5:
                if near:
                    if m.cls == m.g_cls:
                        m.weight = f32(m.weight * f32(f32(1) + m.g_weight))
                    if m.inst == m.g_inst:
                        m.inst_weight = f32(m.inst_weight * f32(f32(1) + m.g_inst_weight))
            else:
                if m.cls == m.g_cls and near:
                    m.weight = f32(f32(m.weight + m.g_weight) - f32(m.weight * m.g_weight))
                    if m.inst == m.g_inst:
                        m.inst_weight = f32(f32(m.inst_weight + m.g_inst_weight) - f32(m.inst_weight * m.g_inst_weight))
    elif fn == 6:
        for m in maxima:
            if m.cls == m.g_cls:
                m.weight = f32(m.weight * m.g_weight)
            if m.inst == m.g_inst:
                m.inst_weight = f32(m.inst_weight * m.g_inst_weight)


def merge_sequence(maxima, fn, radius, min_threshold=0.0, best_k=-1, min_svm_score=0.70, rate_limit=0.60, weight_factor=1.5, pre_normalized=True):
    """voting.cpp:272-323 on maxima sorted by weight (descending, stable). pre_normalized: the weights already carry the first
    normalisation's common scale (the device's), so function 5 sees scaled instead of raw weights; the hypothesis
    weights are normalised here in either case except for function 5, as the reference does."""
    maxima = sorted(maxima, key=lambda m: -float(m.weight))
    if not maxima:
        return maxima
    if fn != 5:
        normalize_weights(maxima)
    merge_hypotheses(fn, maxima, radius, min_svm_score, rate_limit, weight_factor)
    maxima = sorted(maxima, key=lambda m: -float(m.weight))
    first_zero = next((i for i, m in enumerate(maxima) if m.weight == 0), len(maxima))     # find_if + erase(it, end)
    maxima = maxima[:first_zero]
    normalize_weights(maxima)
    thr = f32(min_threshold)
    if thr < 0:
        thr = f32(-thr * (maxima[0].weight if maxima else f32(0)))
    maxima = [m for m in maxima if m.weight >= thr]
    if best_k > 0 and len(maxima) >= best_k:
        maxima = maxima[:best_k]
    return maxima
