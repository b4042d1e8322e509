"""Restatement of the Short SHOT with colour histogram (features/features_short_cshot.cpp:103-507, 592-646 of the reference) in numpy, in
the operation order and with the number types of the reference's source, on the pieces of short_shot_ref.py (linear_interpolation, the
switch distance, the rad2deg constant, configureSphericalGrid, the minimum radius): float32 local coordinates, float64 spherical
coordinates and raw bin values cast to float32, float32 increments accumulated in float64, one L2 norm over the fused row.

The three deviations of short_shot_ref.py carry over (dot-product order, float32 Radius / minimum radius, 57.29578). A fourth: the colour
distance is taken in float32 as PCL's cshot.hpp takes it (the reference says its block is copied from there; its unqualified fabs pins
neither width). Raw CIELab per colour comes from the caller's `rgb2lab(colour) -> (L, a, b)` (the tests pass the oracle's, which the CSHOT
edge-colour test holds bit-equal to the device's LUT path); it is called once per distinct colour.

The secondary colour bin receives (1 - f_c) + (1 - f_r) + f_theta + f_phi as the reference writes it (:424), not ... + f_r.

switch_margin: the smallest distance, in raw units, of any geometric raw value of EITHER grid before its cast to float32 from a value at
which the cast would change a hard decision (short_shot_ref._switch_distance). raw_c involves no libm and no margin: its float32
operations are the same on every IEEE machine."""
import numpy as np

import short_shot_ref as ssr

f32, f64 = np.float32, np.float64
COLOR_BINS = {d: ssr.AUTO_BINS[d] for d in (8, 16, 24, 32, 64, 96, 128)}


def configure_spherical_color_grid(dims=32):
    """configureSphericalColorGrid (:592-646) -> (dims, (rc, ec, ac)); there is no manual colour grid"""
    return (dims, COLOR_BINS[dims]) if dims in COLOR_BINS else (32, (2, 2, 8))


def total_dims(bins, color_bins, hist_size):
    return bins[0] * bins[1] * bins[2] + color_bins[0] * color_bins[1] * color_bins[2] * hist_size


def lab_table(rgb2lab, colors):
    """normalised CIELab (:151-155, :189-193) of every colour in `colors` -> float32 [n, 3]; rgb2lab runs once per distinct colour"""
    colors = np.asarray(colors, np.uint32).reshape(-1)
    uniq, inv = np.unique(colors, return_inverse=True)
    raw = np.array([rgb2lab(int(c)) for c in uniq], f32).reshape(-1, 3)
    norm = np.stack([raw[:, 0] / f32(100), raw[:, 1] / f32(120), raw[:, 2] / f32(120)], 1).astype(f32)
    return norm[inv]


def color_distance(lab_ref, lab):
    """(:194-198) on normalised CIELab, float32 [3] against float32 [n, 3] -> float32 [n] in [0, 1]"""
    dl = np.abs((lab_ref[0] - lab[:, 0]).astype(f32))
    da = np.abs((lab_ref[1] - lab[:, 1]).astype(f32))
    db = np.abs((lab_ref[2] - lab[:, 2]).astype(f32))
    cd = ((dl + ((da + db).astype(f32) / f32(2)).astype(f32)).astype(f32) / f32(3)).astype(f32)
    return np.minimum(np.maximum(cd, f32(0)), f32(1)).astype(f32)


def raw_values(bins, r, theta, phi, R, rmin, log_radius):
    """the three float64 raw bin values of one grid (:232-246 / :320-334) before their cast to float32"""
    rb, eb, ab = bins
    if log_radius:
        ln_rmin = 0.0 if rmin == 0 else np.log(rmin)
        ln_rmax_rmin = 0.0 if rmin == 0 else np.log(R / rmin)
        raw_r = ((rb - 1) * (np.log(r) - ln_rmin)) / ln_rmax_rmin + 1
    else:
        raw_r = (rb * r) / R
    return [raw_r, (eb * theta) / 180, (ab * (phi + 180)) / 360]


def axis(raw, n, clamp_low=False, cyclic=False):
    """one axis: primary bin, share, secondary bin after correct_bin, and whether the secondary bin exists"""
    b = np.trunc(raw).astype(np.int32)
    b = np.minimum(np.maximum(b, 0) if clamp_low else b, n - 1)
    f, s, _ = ssr._interp(raw)
    b2 = b + s
    b2 = np.where(b2 < 0, n - 1, np.where(b2 >= n, 0, b2)) if cyclic else np.clip(b2, 0, n - 1)
    ok = (b2 != b) if n > 1 else np.zeros(len(raw), bool)
    return b, f, b2, ok


def _sum(*terms):
    """float32 sum, left to right"""
    acc = terms[0]
    for t in terms[1:]:
        acc = (acc + t).astype(f32)
    return acc


def shape_deposits(hist, bins, raw):
    """compute_shape_descriptor (:225-310) on float32 raw values -> adds into hist (float64)"""
    rb, eb, ab = bins
    (b_r, f_r, r2, ok_r), (b_t, f_t, t2, ok_t), (b_p, f_p, p2, ok_p) = axis(raw[0], rb, clamp_low=True), axis(raw[1], eb), axis(raw[2], ab, cyclic=True)
    one = f32(1)
    idx = lambda br, bt, bp: br + bt * rb + bp * rb * eb
    np.add.at(hist, idx(b_r, b_t, b_p), _sum(f_r, f_t, f_p).astype(f64))
    np.add.at(hist, idx(b_r, b_t, p2)[ok_p], _sum(f_r, f_t, (one - f_p).astype(f32)).astype(f64)[ok_p])
    np.add.at(hist, idx(b_r, t2, b_p)[ok_t], _sum(f_r, (one - f_t).astype(f32), f_p).astype(f64)[ok_t])
    np.add.at(hist, idx(r2, b_t, b_p)[ok_r], _sum((one - f_r).astype(f32), f_t, f_p).astype(f64)[ok_r])


def color_deposits(hist, color_bins, hist_size, raw, raw_c):
    """compute_color_descriptor (:312-429) on float32 raw values -> adds into hist (float64, the colour part only)"""
    rb, eb, ab = color_bins
    H = hist_size
    (b_r, f_r, r2, ok_r), (b_t, f_t, t2, ok_t), (b_p, f_p, p2, ok_p) = axis(raw[0], rb, clamp_low=True), axis(raw[1], eb), axis(raw[2], ab, cyclic=True)
    b_c, f_c, c2, ok_c = axis(raw_c, H)
    one = f32(1)
    idx = lambda bc, br, bt, bp: bc + br * H + bt * H * rb + bp * H * rb * eb
    np.add.at(hist, idx(b_c, b_r, b_t, b_p), _sum(f_c, f_r, f_t, f_p).astype(f64))
    np.add.at(hist, idx(b_c, b_r, b_t, p2)[ok_p], _sum(f_c, f_r, f_t, (one - f_p).astype(f32)).astype(f64)[ok_p])
    np.add.at(hist, idx(b_c, b_r, t2, b_p)[ok_t], _sum(f_c, f_r, (one - f_t).astype(f32), f_p).astype(f64)[ok_t])
    np.add.at(hist, idx(b_c, r2, b_t, b_p)[ok_r], _sum(f_c, (one - f_r).astype(f32), f_t, f_p).astype(f64)[ok_r])
    np.add.at(hist, idx(c2, b_r, b_t, b_p)[ok_c], _sum((one - f_c).astype(f32), (one - f_r).astype(f32), f_t, f_p).astype(f64)[ok_c])   # :424 as written


def short_cshot_keypoint(points, lab, kp, kp_lab, frame, radius, bins, color_bins, hist_size, min_radius=0.0, log_radius=False):
    """one keypoint on the NaN-free points [n, 3] float32 with their normalised CIELab [n, 3] -> (row float32 [D], neighbour count,
    switch_margin)"""
    Ds, D = bins[0] * bins[1] * bins[2], total_dims(bins, color_bins, hist_size)
    kp, frame = np.asarray(kp, f32), np.asarray(frame, f32).reshape(3, 3)
    if not (np.isfinite(kp).all() and np.isfinite(frame).all()):
        return np.full(D, np.nan, f32), 0, np.inf
    R, rmin = f64(f32(radius)), f64(f32(min_radius))
    v = (points - kp[None, :]).astype(f32)
    d2 = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(f32) + v[:, 2] * v[:, 2]).astype(f32)
    inside = d2 < f32(R * R)
    count = int(inside.sum())
    sel = inside & (d2 > f32(1e-15))
    v, lab = v[sel], lab[sel]
    dot = lambda ax: ((v[:, 0] * ax[0] + v[:, 1] * ax[1]).astype(f32) + v[:, 2] * ax[2]).astype(f32).astype(f64)
    xl, yl, zl = dot(frame[0]), dot(frame[1]), dot(frame[2])
    r = np.sqrt((xl * xl + yl * yl) + zl * zl)
    keep = ~(r < rmin)
    xl, yl, zl, r, lab = xl[keep], yl[keep], zl[keep], r[keep], lab[keep]
    hist = np.zeros(D, f64)
    if len(r) == 0:
        with np.errstate(invalid="ignore"):
            return (hist / 0.0).astype(f32), count, np.inf
    theta = np.arccos(zl / r) * ssr.RAD2DEG
    phi = np.arctan2(yl, xl) * ssr.RAD2DEG
    raw_s = raw_values(bins, r, theta, phi, R, rmin, log_radius)
    raw_g = raw_values(color_bins, r, theta, phi, R, rmin, log_radius)
    shape_deposits(hist[:Ds], bins, [a.astype(f32) for a in raw_s])
    raw_c = (color_distance(np.asarray(kp_lab, f32), lab).astype(f64) * hist_size).astype(f32)
    color_deposits(hist[Ds:], color_bins, hist_size, [a.astype(f32) for a in raw_g], raw_c)
    norm = np.sqrt(np.cumsum(hist * hist)[-1])            # sequential double sum over the fused row, as the reference's loop
    switch = min(float(ssr._switch_distance(a).min()) for a in raw_s + raw_g)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (hist / norm).astype(f32), count, switch


def short_cshot_ref(rgb2lab, pt_off, points, rgba, kp_off, keypoints, kp_rgba, frames, radius, bins, color_bins=(2, 2, 8), hist_size=15,
                    min_radius=0.0, log_radius=False):
    """ragged batch (offsets as frontend_scenes.soa makes them; frames [nkp, 9]; colours 0x00RRGGBB) ->
    (desc float32 [nkp, D], counts int64 [nkp], switch_margin [nkp])"""
    points, keypoints, frames = np.asarray(points, f32), np.asarray(keypoints, f32), np.asarray(frames, f32)
    n = int(kp_off[-1])
    both = lab_table(rgb2lab, np.concatenate([np.asarray(rgba, np.uint32).reshape(-1), np.asarray(kp_rgba, np.uint32).reshape(-1)]))
    lab, kp_lab = both[:len(points)], both[len(points):]
    desc, cnt, switch = np.zeros((n, total_dims(bins, color_bins, hist_size)), f32), np.zeros(n, np.int64), np.full(n, np.inf)
    for o in range(len(pt_off) - 1):
        p, l = points[pt_off[o]:pt_off[o + 1]], lab[pt_off[o]:pt_off[o + 1]]
        ok = np.isfinite(p).all(1)
        p, l = p[ok], l[ok]
        for k in range(kp_off[o], kp_off[o + 1]):
            desc[k], cnt[k], switch[k] = short_cshot_keypoint(p, l, keypoints[k], kp_lab[k], frames[k], radius, bins, color_bins, hist_size,
                                                              min_radius, log_radius)
    return desc, cnt, switch
