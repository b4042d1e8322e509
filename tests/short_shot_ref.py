"""Restatement of the generalised Short SHOT (features/features_short_shot.cpp:77-283 of the reference) in numpy, in the operation
order and with the number types of the reference's source: float32 for the local coordinates, float64 for the spherical coordinates
and the raw bin values, which are then cast to float32 as the reference's `float raw_*` variables are. Brute-force neighbours.

Three points are this library's definition rather than the reference's text: the summation order of the float dot product
(the reference's Eigen Vector4f::dot does not state one), Radius and the minimum radius taken as float32, and pcl::rad2deg(double)'s
truncated constant 57.29578, restated from PCL 1.10.

Besides the descriptors and the neighbour counts every function returns two margins per keypoint:
  frac_margin   the smallest distance of any float32 raw value's fraction from 0.5 (inf without a contributing neighbour);
  switch_margin the smallest distance, in raw units, of any raw value BEFORE its cast to float32 from a value at which the cast would
                change a hard decision (the int() of the raw value or its `decimals <= 0.5f`). This is what decides whether two
                libm implementations (host, device: a few ulp of double apart, ~1e-13 here) can disagree on a bin. A value placed
                EXACTLY on a switch (raw_r == 1.5) is robust by this measure: it sits half a float32 ulp from the next decision."""
import numpy as np

f32, f64 = np.float32, np.float64
RAD2DEG = 57.29578                       # pcl::rad2deg(double), PCL 1.10 common/impl/angles.hpp
AUTO_BINS = {8: (1, 1, 8), 16: (2, 2, 4), 24: (2, 2, 6), 32: (2, 2, 8), 64: (2, 4, 8), 96: (3, 4, 8), 128: (4, 4, 8), 192: (6, 4, 8), 256: (8, 4, 8)}


def configure_spherical_grid(dims=32, bin_type="auto", bins=(2, 2, 8)):
    """configureSphericalGrid (:285-366) -> (dims, (r, e, a))"""
    if bin_type == "auto":
        return (dims, AUTO_BINS[dims]) if dims in AUTO_BINS else (32, (2, 2, 8))
    if bin_type == "manual":
        return bins[0] * bins[1] * bins[2], tuple(bins)
    return 32, (2, 2, 8)


def min_radius_of(radius, use_min_radius=False, min_radius_relative=0.0, log_radius=False):
    """compute_descriptor :88-103, as the float32 the library's entry point takes"""
    if use_min_radius:
        return f32(f64(f32(radius)) * f64(min_radius_relative))
    return f32(f64(f32(radius)) * f64(f32(0.1))) if log_radius else f32(0.0)


def _interp(raw):
    """linear_interpolation (:246-260) on a float32 array -> (share float32, step int, decimals float32)"""
    dec = (raw - np.trunc(raw).astype(np.int32).astype(f32)).astype(f32)
    lo = dec <= f32(0.5)
    share = np.where(lo, (dec.astype(f64) + 0.5).astype(f32), ((f32(1) - dec).astype(f32).astype(f64) + 0.5).astype(f32)).astype(f32)
    return share, np.where(lo, -1, 1).astype(np.int32), dec


def _switch_distance(v):
    """distance of the float64 values v from the nearest value at which float32(v) changes int() or `fraction <= 0.5`: adjacent
    float32 values decide differently only across an integer n (pred(n) | n) and across n + 0.5 (n + 0.5 | succ(n + 0.5)), and the
    cast switches between two adjacent float32 values at their midpoint. int() truncates towards zero, so nothing changes across 0
    (the raw values here are > -1: a hair below 0 only for phi = -180 degrees)"""
    v = np.asarray(v, f64)
    out = np.full(v.shape, np.inf)
    base = np.floor(v)
    for k in (-1.0, 0.0, 1.0):
        n = (base + k).astype(f32)
        t_int = (np.nextafter(n, f32(-np.inf)).astype(f64) + n.astype(f64)) / 2
        h = (n.astype(f64) + 0.5).astype(f32)
        t_half = (h.astype(f64) + np.nextafter(h, f32(np.inf)).astype(f64)) / 2
        d_int = np.where(n > 0, np.abs(v - t_int), np.inf)
        out = np.minimum(out, np.minimum(d_int, np.abs(v - t_half)))
    return out


def short_shot_keypoint(points, kp, frame, radius, bins, min_radius=0.0, log_radius=False):
    """one keypoint on the NaN-free points [n, 3] float32 -> (row float32 [D], neighbour count, frac_margin, switch_margin)"""
    rb, eb, ab = bins
    D = rb * eb * ab
    kp, frame = np.asarray(kp, f32), np.asarray(frame, f32).reshape(3, 3)
    if not (np.isfinite(kp).all() and np.isfinite(frame).all()):
        return np.full(D, np.nan, f32), 0, np.inf, np.inf
    R = f64(f32(radius))
    rmin = f64(f32(min_radius))
    v = (points - kp[None, :]).astype(f32)
    d2 = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(f32) + v[:, 2] * v[:, 2]).astype(f32)
    inside = d2 < f32(R * R)
    count = int(inside.sum())
    v = v[inside & (d2 > f32(1e-15))]
    dot = lambda ax: ((v[:, 0] * ax[0] + v[:, 1] * ax[1]).astype(f32) + v[:, 2] * ax[2]).astype(f32).astype(f64)
    xl, yl, zl = dot(frame[0]), dot(frame[1]), dot(frame[2])
    r = np.sqrt((xl * xl + yl * yl) + zl * zl)
    keep = ~(r < rmin)
    xl, yl, zl, r = xl[keep], yl[keep], zl[keep], r[keep]
    hist = np.zeros(D, f64)
    if len(r) == 0:
        with np.errstate(invalid="ignore"):
            return (hist / 0.0).astype(f32), count, np.inf, np.inf
    theta = np.arccos(zl / r) * RAD2DEG
    phi = np.arctan2(yl, xl) * RAD2DEG
    if log_radius:
        ln_rmin = 0.0 if rmin == 0 else np.log(rmin)
        ln_rmax_rmin = 0.0 if rmin == 0 else np.log(R / rmin)
        raw_r64 = ((rb - 1) * (np.log(r) - ln_rmin)) / ln_rmax_rmin + 1
    else:
        raw_r64 = (rb * r) / R
    raw64 = [raw_r64, (eb * theta) / 180, (ab * (phi + 180)) / 360]
    raw = [a.astype(f32) for a in raw64]
    b_r = np.clip(np.trunc(raw[0]).astype(np.int32), 0, rb - 1)
    b_t = np.minimum(np.trunc(raw[1]).astype(np.int32), eb - 1)
    b_p = np.minimum(np.trunc(raw[2]).astype(np.int32), ab - 1)
    (f_r, s_r, d_r), (f_t, s_t, d_t), (f_p, s_p, d_p) = _interp(raw[0]), _interp(raw[1]), _interp(raw[2])
    r2b = np.clip(b_r + s_r, 0, rb - 1)
    t2b = np.clip(b_t + s_t, 0, eb - 1)
    p2b = b_p + s_p
    p2b = np.where(p2b < 0, ab - 1, np.where(p2b >= ab, 0, p2b))
    one = f32(1)
    idx = lambda br, bt, bp: br + bt * rb + bp * rb * eb
    np.add.at(hist, idx(b_r, b_t, b_p), ((f_r + f_t).astype(f32) + f_p).astype(f32).astype(f64))
    ok = (p2b != b_p) if ab > 1 else np.zeros(len(r), bool)
    np.add.at(hist, idx(b_r, b_t, p2b)[ok], ((f_r + f_t).astype(f32) + (one - f_p).astype(f32)).astype(f32).astype(f64)[ok])
    ok = (t2b != b_t) if eb > 1 else np.zeros(len(r), bool)
    np.add.at(hist, idx(b_r, t2b, b_p)[ok], ((f_r + (one - f_t).astype(f32)).astype(f32) + f_p).astype(f32).astype(f64)[ok])
    ok = (r2b != b_r) if rb > 1 else np.zeros(len(r), bool)
    np.add.at(hist, idx(r2b, b_t, b_p)[ok], (((one - f_r).astype(f32) + f_t).astype(f32) + f_p).astype(f32).astype(f64)[ok])
    norm = np.sqrt(np.cumsum(hist * hist)[-1])            # sequential double sum, as the reference's loop
    frac = min(float(np.abs(d.astype(f64) - 0.5).min()) for d in (d_r, d_t, d_p))
    switch = min(float(_switch_distance(a).min()) for a in raw64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (hist / norm).astype(f32), count, frac, switch


def short_shot_ref(pt_off, points, kp_off, keypoints, frames, radius, bins, min_radius=0.0, log_radius=False):
    """ragged batch (offsets as frontend_scenes.soa makes them; frames [nkp, 9]) ->
    (desc float32 [nkp, D], counts int64 [nkp], frac_margin [nkp], switch_margin [nkp])"""
    points, keypoints, frames = np.asarray(points, f32), np.asarray(keypoints, f32), np.asarray(frames, f32)
    n = int(kp_off[-1])
    D = bins[0] * bins[1] * bins[2]
    desc, cnt = np.zeros((n, D), f32), np.zeros(n, np.int64)
    frac, switch = np.full(n, np.inf), np.full(n, np.inf)
    for o in range(len(pt_off) - 1):
        p = points[pt_off[o]:pt_off[o + 1]]
        p = p[np.isfinite(p).all(1)]
        for k in range(kp_off[o], kp_off[o + 1]):
            desc[k], cnt[k], frac[k], switch[k] = short_shot_keypoint(p, keypoints[k], frames[k], radius, bins, min_radius, log_radius)
    return desc, cnt, frac, switch
