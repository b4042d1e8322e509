"""The CVFH region descriptor (ismhip_global_cvfh, include/ismhip.h) restated in float64, numpy only, from the header's text: clustering
normals, the link graph, its connected components, the kept clusters with their means, and interval counts per bin of a row given the
row's centroid and normal (vfh_ref.py's approach, MARGIN = 1e-4 raw bin units, with the distance block 45 * f4 / dmax).

A link whose distance or angle lies within a margin of its threshold is UNDECIDED. The margins, from the device's expressions:
  distance  d2 = (dx*dx + dy*dy) + dz*dz in float32, unfused, against float32(tol * tol): three differences (2^-24 relative each, squared:
            2 * 2^-24), three products and two sums (2^-24 each), the threshold's own rounding 2^-24: below 8 * 2^-24 relative. DIST_REL.
  angle     the cosine is a float64 sum of three float64 products of float32 components: 3 * 2^-53; cos(threshold) from another libm: one
            ulp, 1.2e-16. With the cloud's own normals both sides see the same float32 inputs: COS_GIVEN = 1e-12 is generous.
            With re-estimated normals the device's float32 normal is the cast of a float64 eigenvector: each component moves by at most
            2^-25 against the exact one, the direction by sqrt(3) * 2^-25, a cosine of two such normals by 2 * sqrt(3) * 2^-25 = 1.04e-7;
            the eigenvector itself (moments rounded to 2^-48 of their bound, a Jacobi solver at 1e-15) moves by ~1e-14 / gap, gap the
            relative distance (l1 - l0) / l2 of the two smallest eigenvalues: below 1e-8 for gap >= GAP_MIN = 1e-6. COS_EST = 1e-6 covers
            both nearly ten times. A re-estimated normal with a smaller gap, or whose sign test |(vp - q) . n| is below SIGN_REL * |vp - q|,
            is UNSTABLE: every link it could take part in by distance is undecided."""
import numpy as np

import vfh_ref as vr

f32, f64 = np.float32, np.float64
NONE = 0xffffffff
ANGLE = 10.0 / 180.0 * np.pi
DIST_REL = 8 * 2.0 ** -24
COS_GIVEN, COS_EST = 1e-12, 1e-6
GAP_MIN, SIGN_REL = 1e-6, 1e-6
NORM = f32(47278.0)
MARGIN = vr.MARGIN


def d2_f32(P, q):
    """the library's squared distance: float32, unfused, (dx*dx + dy*dy) + dz*dz"""
    d = (np.asarray(P, f32) - np.asarray(q, f32)).astype(f32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]).astype(f32)


def r2_f32(r):
    return f32(f64(f32(r)) * f64(f32(r)))


def select(P, center, radius):
    """indices of the finite points of an object a region selects (radius None or negative: all of them)"""
    P = np.asarray(P, f32).reshape(-1, 3)
    fin = np.isfinite(P).all(1)
    if radius is None or radius < 0:
        return np.nonzero(fin)[0]
    with np.errstate(invalid="ignore"):
        return np.nonzero(fin & (d2_f32(P, center) < r2_f32(radius)))[0]


def clustering_normals(P, N, sel, normal_radius, min_points, viewpoint=(0, 0, 0)):
    """-> (normals [len(sel), 3] float64 (NaN rows), unstable [len(sel)] bool, estimated: bool)"""
    P, N = np.asarray(P, f32).reshape(-1, 3), np.asarray(N, f32).reshape(-1, 3)
    if not (normal_radius > 0) or len(sel) < min_points:
        return N[sel].astype(f64), np.zeros(len(sel), bool), False
    S = P[sel]
    out = np.full((len(sel), 3), np.nan)
    unstable = np.zeros(len(sel), bool)
    r2 = r2_f32(normal_radius)
    vp = np.asarray(viewpoint, f32)
    for i, q in enumerate(S):
        d2 = d2_f32(S, q)
        nb = d2 < r2
        if np.any(np.abs(d2.astype(f64) - f64(r2)) <= DIST_REL * f64(r2)):
            unstable[i] = True
        if nb.sum() < 3:
            continue
        v = S[nb].astype(f64) - q.astype(f64)
        m = v.mean(0)
        C = v.T @ v / len(v) - np.outer(m, m)
        w, V = np.linalg.eigh(C)
        n = V[:, 0]
        if not (w[1] - w[0]) >= GAP_MIN * max(w[2], 1e-300):
            unstable[i] = True
        to_vp = (vp - q).astype(f64)
        s = float(to_vp @ n)
        if abs(s) <= SIGN_REL * np.linalg.norm(to_vp):
            unstable[i] = True
        out[i] = -n if s < 0 else n
    return out, unstable, True


def link_graph(P, sel, normals, unstable, estimated, tolerance, angle=ANGLE):
    """-> (decided [k, k] bool, undecided [k, k] bool) over the selected points, symmetric, no diagonal"""
    S = np.asarray(P, f32).reshape(-1, 3)[sel]
    k = len(S)
    t2 = r2_f32(tolerance)
    d2 = np.stack([d2_f32(S, q) for q in S]) if k else np.zeros((0, 0), f32)
    near = d2 < t2
    near_und = np.abs(d2.astype(f64) - f64(t2)) <= DIST_REL * f64(t2)
    fin = np.isfinite(normals).all(1)
    with np.errstate(invalid="ignore"):
        c = np.clip(normals @ normals.T, -1.0, 1.0)
    thr = np.cos(angle)
    ok = fin[:, None] & fin[None, :]
    ang = ok & (c > thr)
    ang_und = ok & (np.abs(c - thr) <= (COS_EST if estimated else COS_GIVEN))
    shaky = unstable[:, None] | unstable[None, :]
    off = ~np.eye(k, dtype=bool)
    maybe_near = near | near_und
    und = off & maybe_near & ((near_und & (ang | ang_und)) | ang_und | (shaky & ok if estimated else False))
    if estimated:                                               # an unstable normal may be NaN on one side and finite on the other
        und |= off & maybe_near & shaky
    dec = off & near & ang & ~und
    return dec, und


def components(adj):
    """connected components of a boolean adjacency -> label [k]: the smallest member index of each point's component"""
    k = len(adj)
    label = np.arange(k)
    seen = np.zeros(k, bool)
    for s in range(k):
        if seen[s]:
            continue
        stack, seen[s] = [s], True
        while stack:
            u = stack.pop()
            label[u] = s
            for v in np.nonzero(adj[u] & ~seen)[0]:
                seen[v] = True
                stack.append(v)
    return label


def region(P, N, center, radius, tolerance, normal_radius, min_points, viewpoint=(0, 0, 0), angle=ANGLE):
    """One region of one object -> dict: sel (original indices), labels [npts] (original index of the component's smallest member, NONE
    where not selected) by the decided links, labels_loose (decided + undecided), n_undecided (links), clusters: list of dict(root, size,
    members (original indices), centroid, normal (float64)), fallback: bool, normals (clustering, [len(sel), 3])"""
    P, N = np.asarray(P, f32).reshape(-1, 3), np.asarray(N, f32).reshape(-1, 3)
    sel = select(P, center, radius)
    nrm, unstable, est = clustering_normals(P, N, sel, normal_radius, min_points, viewpoint)
    dec, und = link_graph(P, sel, nrm, unstable, est, tolerance, angle)
    out = dict(sel=sel, normals=nrm, n_undecided=int(und.sum()) // 2, estimated=est)
    for key, adj in (("labels", dec), ("labels_loose", dec | und)):
        lab = np.full(len(P), NONE, np.int64)
        if len(sel):
            lab[sel] = sel[components(adj)]
        out[key] = lab
    lab = out["labels"]
    clusters = []
    for root in np.unique(lab[sel]) if len(sel) else []:
        members = np.nonzero(lab == root)[0]
        if len(members) >= min_points:
            clusters.append(dict(root=int(root), size=len(members), members=members))
    out["fallback"] = len(sel) > 0 and not clusters
    if out["fallback"]:
        clusters = [dict(root=NONE, size=len(sel), members=sel)]
    pos_of = {int(o): i for i, o in enumerate(sel)}
    for c in clusters:
        c["centroid"] = P[c["members"]].astype(f64).mean(0)
        n = nrm[[pos_of[int(o)] for o in c["members"]]]
        n = n[np.isfinite(n).all(1)]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = n.mean(0) if len(n) else np.full(3, np.nan)
            c["mean_normal_length"] = float(np.linalg.norm(mean))
            c["normal"] = mean / np.linalg.norm(mean)
    out["clusters"] = clusters
    return out


def dmax_f32(P, c):
    """the largest float32 |p - c| (the deposit's f4) over the points"""
    d = (np.asarray(P, f32) - np.asarray(c, f32)).astype(f32)
    return f32(np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32) + d[:, 2] * d[:, 2]).astype(f32)).max())


def row_counts(P, N, c, nc, viewpoint=(0, 0, 0), margin=MARGIN):
    """One row: P / N the region's selected points and CLOUD normals, c / nc the row's (device) centroid and normal -> vfh_ref.vfh_counts'
    dict with the distance block binned as 45 * f4 / dmax"""
    P, N = vr.finite_normals(P, N)
    m = len(P)
    counts, lower, upper = (np.zeros(vr.DIM, np.int64) for _ in range(3))
    out = dict(counts=counts, lower=lower, upper=upper, m=m, undecided=0, total_lower=np.zeros(5, np.int64), total_upper=np.zeros(5, np.int64))
    if m < 2:
        return out
    pr = vr.pairs64(P, N, c, nc, margin)
    dmax = f64(dmax_f32(P, c))
    dn = np.linalg.norm(P.astype(f64) - np.asarray(c, f32).astype(f64)[None, :], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t4 = vr.SHAPE_BINS * dn / dmax
    t4 = np.where(np.isfinite(t4), t4, 0.0)
    pr["t"][:, 3] = t4
    pr["masks"][:, 3] = vr._edge_mask(t4, np.full(m, margin))
    live = ~pr["reject"]
    single = (pr["masks"] & (pr["masks"] - 1)) == 0
    und_pt = np.zeros(m, bool)
    for blk in range(4):
        mk = pr["masks"][:, blk]
        face = np.clip(np.floor(pr["t"][:, blk]), 0, vr.SHAPE_BINS - 1).astype(np.int64)
        counts[blk * 45:(blk + 1) * 45] = np.bincount(face[live], minlength=45)
        decided = live & single[:, blk] & ~pr["maybe"]
        und_pt |= live & ~decided
        for b in range(45):
            has = live & ((mk >> b) & 1).astype(bool)
            lower[blk * 45 + b] = int((has & decided).sum())
            upper[blk * 45 + b] = int(has.sum())
        out["total_lower"][blk] = int(decided.sum())
        out["total_upper"][blk] = int(live.sum())
    d = vr.view_direction(c, viewpoint)
    t, vb, vund = vr.viewpoint64(N, d, margin)
    counts[180:] = np.bincount(vb, minlength=128)
    lower[180:] = np.bincount(vb[~vund], minlength=128)
    upper[180:] = lower[180:]
    for i in np.nonzero(vund)[0]:
        r = int(np.rint(t[i]))
        upper[180 + r] += 1
        upper[180 + r - 1] += 1
    out["total_lower"][4] = out["total_upper"][4] = m
    out["undecided"] = int((und_pt | vund).sum())
    return out


def row_of_counts(counts):
    """float32(count) / 47278.0f"""
    return (np.asarray(counts).astype(f32) / NORM).astype(f32)
