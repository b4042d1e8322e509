"""One wide ragged batch for every Features type, cloud pass and keypoint detector (tests/test_batch_cpu.py, tests/test_gpu_feature_batch.py,
tests/test_gpu_keypoint_batch.py), built once per process, and the answers of the modules' own restatements on it, object by object.

Eleven objects: one full group of eight of the XCD-local block map (csrc/common.h: xcd_object_block) and a group of three, which leaves
five padding slots. The keypoint runs are 13, 2, 3, 1, 4, 0, 1, 6, 2, 7, 5: the longest (13, no multiple of the four waves of a block) is
unique, so every other object has blocks without a keypoint. The surfaces are the bumpy ellipsoids of iss3d_scenes.py, each at its own
scale, texture amplitude and intensity amplitude, so that the per-object maxima (k_cull_nmax, k_cull_kmax, k_sift_imax, k_rift_gmax) differ
by more than a power of two between objects: a kernel that reads another object's maximum puts its fixed point on another grid.

    0 longest      600 points, scale 1.0, 13 keypoints (9 cloud points, 4 next to the cloud)
    1 empty        0 points, 2 keypoints
    2 small3       300 points, scale 0.6, 3 keypoints
    3 all_nan      3 points whose coordinates are all NaN, 1 keypoint
    4 holes        257 points, scale 0.7: five NaN normals, one NaN point, one +inf point, interleaved; 4 keypoints
    5 no_kp        400 points, scale 0.8, normals of length 3 (the only non-unit ones: no descriptor reads them), no keypoint
    6 one_point    1 point with a keypoint on it
    7 off_cloud    900 points, scale 1.3, 6 keypoints: one far off the cloud (an empty ball), one not finite
    8 four_points  4 points of one colour within 0.1 (fewer than the 5 a frame needs), 2 keypoints: their rows lose only to the frame
    9 p65          65 points, scale 0.35, 7 keypoints
   10 small5       300 points, scale 0.5, 5 keypoints

Radii are those of the modules' own small scenes at this density (700 points of the unit ellipsoid: 0.15 for ISS3D's salient radius and
RIFT, 0.045 for SIFT3D's base scale, the culling tests' leaf of 0.2); the descriptor balls hold 10 to 55 points."""
import functools
import os

import numpy as np

import bshot_ref
import cgf_ref
import cgf_scenes
import cospair_ref
import esf_ref
import fpfh_ref
import lab_ref
import rift_ref
import rsd_ref
import short_cshot_ref
import short_shot_ref
import shot_ref
import shot_ref_scenes
import shotna_ref
import spin_image_ref
from iss3d_scenes import bumpy_ellipsoid

F = np.float32
TYPES = ("SHOT", "BSHOT", "CSHOT", "SHORT_SHOT", "SHORT_CSHOT", "FPFH", "CoSPAIR", "SpinImage", "RSD", "RIFT", "CGF", "ESF_LOCAL")
NAMES = ("longest", "empty", "small3", "all_nan", "holes", "no_kp", "one_point", "off_cloud", "four_points", "p65", "small5")
N_OBJ = len(NAMES)

RADIUS = 0.15                 # Features.Radius of every type but CGF and ESF_LOCAL
LRF_RADIUS = 0.2              # Features.ReferenceFrameRadius
CGF_RADIUS = 0.8              # R = 0.8, the frame at 0.6, the keypoint normal at 0.08
ESF_RADIUS = 0.3
ESF_SAMPLES = 1000            # as esf_scenes.py: no multiple of the kernel's 256-attempt blocks
SHORT_BINS = (2, 2, 8)        # ShortShotDims 32, "auto"
SHORT_COLOR_BINS = (2, 2, 8)  # ShortColorShotDims 32
SHORT_HIST = 15
SWITCH_MARGIN = 1e-9          # test_short_shot_cpu.py, test_short_cshot_cpu.py: no raw value closer than this to a switch of its cast
SPIN_WIDTH = 8
HOLES_NEAR = 1                # the keypoint of `holes` that sits beside its NaN normals (the second of its run)
# name -> (points, scale, texture amplitude of 127, intensity amplitude, seed)
SURFACES = {"longest": (600, 1.0, 100, 1.0, 101), "small3": (300, 0.6, 25, 9.0, 102), "holes": (257, 0.7, 60, 0.2, 104),
            "no_kp": (400, 0.8, 12, 40.0, 105), "off_cloud": (900, 1.3, 110, 3.0, 107), "p65": (65, 0.35, 40, 0.03, 109),
            "small5": (300, 0.5, 80, 150.0, 110)}
AXES = np.array([0.5, 0.35, 0.25])


def _surface(name):
    """-> (xyz, unit normals (the smooth ellipsoid's, as culling_scenes.normals_of without its noise), rgba int32, intensity)"""
    n, scale, amp, iamp, seed = SURFACES[name]
    u = bumpy_ellipsoid(n, seed).astype(np.float64)
    nrm = u / AXES ** 2
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    c = np.rint(128.0 + amp * np.stack([np.sin(9.0 * u[:, 0]), np.cos(7.0 * u[:, 1]), np.sin(11.0 * u[:, 2])], 1)).astype(np.int64)
    assert c.min() >= 0 and c.max() <= 255
    rng = np.random.default_rng(seed + 100)
    inten = iamp * (0.5 + 0.3 * np.sin(9.0 * u[:, 0]) * np.cos(7.0 * u[:, 1]) + 0.2 * np.sin(11.0 * u[:, 2]) + rng.normal(scale=0.02, size=n))
    return (u * scale).astype(F), nrm.astype(F), ((c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]).astype(np.int32), inten.astype(F)


def _keypoints(rng, xyz, n_cloud, n_near, ok=None):
    """n_cloud cloud points and n_near points 0.004 next to a cloud point, shuffled -> (keypoints, index of the cloud point each came from)"""
    pool = np.arange(len(xyz)) if ok is None else np.nonzero(ok)[0]
    pick = rng.choice(pool, n_cloud + n_near, replace=False)
    kp = xyz[pick].copy()
    kp[n_cloud:] += F(0.004)
    order = rng.permutation(len(kp))
    return kp[order], pick[order]


def _decided_colours(xyz, rgba, kp, src):
    """The keypoints' colours (that of the cloud point each came from; mid grey without one) and the cloud's colours with the blue channel
    of a few points moved by one or two, until shot_ref.py decides the colour step of every point in every keypoint's ball (about one
    pair in 200 of the plain texture lies inside the CIELab bound of a step edge) and lab_ref.py decides every colour's table entry."""
    rgba = rgba.copy()
    r2 = F(float(F(RADIUS)) * float(F(RADIUS)))
    balls = []
    for q in kp:
        with np.errstate(invalid="ignore"):
            d = (xyz - q).astype(F)
            d2 = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)
            balls.append(np.nonzero(d2 < r2)[0])
    for _ in range(64):
        kp_rgba = rgba[src] if src is not None else np.full(len(kp), 0x808080, np.int32)
        open_ = set(np.nonzero(~lab_ref.convert(rgba.astype(np.uint32)).decided)[0].tolist()) if len(rgba) else set()
        for k, nb in enumerate(balls):
            if len(nb):
                _step, dec = shot_ref_scenes.colour_steps(np.uint32(kp_rgba[k]), rgba[nb].astype(np.uint32))
                open_ |= set(nb[~dec].tolist())
        if not open_:
            return rgba, kp_rgba
        for i in open_:
            rgba[i] = (rgba[i] & ~0xff) | ((int(rgba[i]) & 0xff) + 1) % 256
    raise AssertionError("colours stay undecided")


@functools.lru_cache(maxsize=None)
def batch():
    """dict(pt_off, xyz, normals, rgba int32, intensity, kp_off, kp, kp_rgba int32, labels): the arrays pipeline.DeviceBatch takes, read only"""
    rng = np.random.default_rng(4711)
    objs = []
    none = (np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, np.int32), np.zeros(0, F))
    for name in NAMES:
        if name in SURFACES:
            xyz, nrm, rgba, inten = _surface(name)
        if name == "longest":
            kp, src = _keypoints(rng, xyz, 9, 4)
        elif name == "empty":
            xyz, nrm, rgba, inten = none
            kp, src = F([[0.1, 0.0, 0.0], [0.0, 0.2, 0.1]]), None
        elif name == "small3":
            kp, src = _keypoints(rng, xyz, 2, 1)
        elif name == "all_nan":
            xyz, nrm, rgba, inten = np.full((3, 3), np.nan, F), np.tile(F([0, 0, 1]), (3, 1)), np.int32([0x102030, 0x405060, 0x708090]), F([1, 2, 3])
            kp, src = F([[0.0, 0.0, 0.0]]), None
        elif name == "holes":
            # the five NaN normals sit next to the point of largest x, which is keypoint HOLES_NEAR; the other three keypoints lie more
            # than two radii from every NaN normal, so that no pair of their FPFH neighbourhoods reads one (fpfh_ref.py calls such a pair
            # degenerate and its keypoint exempt)
            top = int(np.argmax(xyz[:, 0]))
            dist = np.linalg.norm(xyz.astype(np.float64) - xyz[top].astype(np.float64), axis=1)
            near = np.argsort(dist)[1:8]
            for j, i in enumerate(near[:5]):
                nrm[i, j % 3] = np.nan
            xyz[near[5], 1] = np.nan
            xyz[near[6], 2] = np.inf
            far = np.ones(len(xyz), bool)
            for i in near[:5]:
                far &= np.linalg.norm(xyz.astype(np.float64) - xyz[i].astype(np.float64), axis=1) > 2.0 * RADIUS + 0.02
            kp, src = _keypoints(rng, xyz, 2, 1, far)
            kp, src = np.concatenate([kp[:1], xyz[top][None, :], kp[1:]]), np.concatenate([src[:1], [top], src[1:]])
        elif name == "no_kp":
            nrm = (nrm * F(3.0)).astype(F)
            kp, src = np.zeros((0, 3), F), None
        elif name == "one_point":
            xyz, nrm, rgba, inten = F([[0.3, -0.2, 0.1]]), F([[0, 0, 1]]), np.int32([0x8040c0]), F([0.7])
            kp, src = xyz.copy(), np.array([0])
        elif name == "off_cloud":
            kp, src = _keypoints(rng, xyz, 3, 1)
            kp = np.concatenate([kp[:2], F([[30.0, 0.0, 0.0]]), kp[2:3], F([[np.nan, 0.0, 0.0]]), kp[3:]])
            src = np.concatenate([src[:2], [0], src[2:3], [1], src[3:]])
        elif name == "four_points":
            # one colour: every intensity gradient is exactly zero, and RIFT's rows here are its all-zero rows
            xyz = (F([0.2, 0.1, -0.3]) + F(0.1) * rng.uniform(-0.5, 0.5, size=(4, 3))).astype(F)
            nrm = np.tile(F([0, 0, 1]), (4, 1)); rgba = np.full(4, 0x204060, np.int32); inten = F([0.1, 0.4, 0.2, 0.3])
            kp, src = np.stack([xyz[2], xyz[0] + F(0.004)]).astype(F), np.array([2, 0])
        elif name == "p65":
            kp, src = _keypoints(rng, xyz, 5, 2)
        elif name == "small5":
            kp, src = _keypoints(rng, xyz, 4, 1)
        rgba, kp_rgba = _decided_colours(xyz, rgba, kp.astype(F), src)
        objs.append((xyz, nrm, rgba, inten, kp.astype(F), kp_rgba.astype(np.int32)))
    off = lambda i: np.concatenate([[0], np.cumsum([len(o[i]) for o in objs])]).astype(np.uint32)
    out = dict(pt_off=off(0), xyz=np.concatenate([o[0] for o in objs]).astype(F), normals=np.concatenate([o[1] for o in objs]).astype(F),
               rgba=np.concatenate([o[2] for o in objs]).astype(np.int32), intensity=np.concatenate([o[3] for o in objs]).astype(F),
               kp_off=off(4), kp=np.concatenate([o[4] for o in objs]).astype(F), kp_rgba=np.concatenate([o[5] for o in objs]).astype(np.int32),
               labels=np.arange(N_OBJ, dtype=np.int32))
    for a in out.values():
        a.setflags(write=False)
    return out


def single(o, b=None):
    """object o of the batch as a batch of its own (n_obj = 1)"""
    b = batch() if b is None else b
    ps, pe, ks, ke = int(b["pt_off"][o]), int(b["pt_off"][o + 1]), int(b["kp_off"][o]), int(b["kp_off"][o + 1])
    return dict(pt_off=np.array([0, pe - ps], np.uint32), xyz=b["xyz"][ps:pe], normals=b["normals"][ps:pe], rgba=b["rgba"][ps:pe],
                intensity=b["intensity"][ps:pe], kp_off=np.array([0, ke - ks], np.uint32), kp=b["kp"][ks:ke], kp_rgba=b["kp_rgba"][ks:ke],
                labels=b["labels"][o:o + 1])


def obj(name):
    return NAMES.index(name)


def kp_range(name):
    b = batch()
    return int(b["kp_off"][obj(name)]), int(b["kp_off"][obj(name) + 1])


def objects():
    """per object (points slice, keypoints slice)"""
    b = batch()
    return [(slice(int(b["pt_off"][o]), int(b["pt_off"][o + 1])), slice(int(b["kp_off"][o]), int(b["kp_off"][o + 1]))) for o in range(N_OBJ)]


@functools.lru_cache(maxsize=None)
def cgf_layers():
    """a small embedding made as cgf_scenes.random_layers makes one: 2244 -> 48 -> 32, sparse, so that the derived bound is tight"""
    return cgf_scenes.random_layers(np.random.default_rng(77), [cgf_ref.DIM, 48, 32], cgf_scenes.MLP_NNZ)


def capi_kwargs(T):
    """the arguments of the type's capi call besides the cloud, the keypoints and (SHOT family) the frames"""
    return {"SHOT": dict(radius=RADIUS), "BSHOT": dict(radius=RADIUS), "CSHOT": dict(radius=RADIUS),
            "SHORT_SHOT": dict(radius=RADIUS, bins=SHORT_BINS, min_radius=0.0, log_radius=False),
            "SHORT_CSHOT": dict(radius=RADIUS, bins=SHORT_BINS, color_bins=SHORT_COLOR_BINS, hist_size=SHORT_HIST, min_radius=0.0, log_radius=False),
            "FPFH": dict(radius=RADIUS), "CoSPAIR": dict(radius=RADIUS), "SpinImage": dict(radius=RADIUS, image_width=SPIN_WIDTH),
            "RSD": dict(radius=RADIUS, full_histogram=True), "RIFT": dict(radius=RADIUS), "CGF": dict(radius=CGF_RADIUS),
            "ESF_LOCAL": dict(radius=ESF_RADIUS, n_samples=ESF_SAMPLES)}[T]


def config_kwargs(T):
    """the IsmConfig fields that make pipeline.Recognizer.compute_features issue the same calls (CGF's model file and ESF_LOCAL's sample count
    are set by the caller: the one is a file, the other the library's constant)"""
    radius = {"CGF": CGF_RADIUS, "ESF_LOCAL": ESF_RADIUS}.get(T, RADIUS)
    return dict(feature=T, radius=radius, lrf_radius=LRF_RADIUS, lrf_type="SHOT", short_shot_dims=32, short_color_shot_dims=32,
                short_color_shot_hist_size=SHORT_HIST, use_full_rsd_histogram=True)


def pipeline_cell(T):
    """the grid cell pipeline.Recognizer.compute_features derives for config_kwargs(T), the ISMHIP_CELL_SCALE switch read as it reads it"""
    radius = {"CGF": CGF_RADIUS, "ESF_LOCAL": ESF_RADIUS}.get(T, RADIUS)
    return min(radius, LRF_RADIUS if T != "FPFH" else radius) * float(os.environ.get("ISMHIP_CELL_SCALE", "0.4"))


# ------------------------------------------------------------------------------------------------------------------ the restatements
@functools.lru_cache(maxsize=None)
def frames(radius=LRF_RADIUS):
    """shotna_ref.frames with normal_votes=False (the SHOT frame) -> dict(frame [K, 9] float32, decided [K], valid, ...)"""
    b = batch()
    return shotna_ref.frames(b["pt_off"], b["xyz"], b["normals"], b["kp_off"], b["kp"], radius, normal_votes=False)


def _per_object(fn):
    """fn(points slice, keypoints slice, object index) -> dict of arrays over the object's keypoints; concatenated over the batch"""
    parts = [fn(ps, ks, o) for o, (ps, ks) in enumerate(objects())]
    keys = parts[0].keys()
    return {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in keys}


def _rows_answer(rows, cnt, undecided, **more):
    rows = np.asarray(rows)
    out = dict(rows=rows, cnt=np.asarray(cnt, np.int64), undecided=np.asarray(undecided, bool))
    out.update(more)
    return out


def _shot(lrf, color):
    b = batch()
    rows = []
    for ps, ks in (o for o in objects()):
        for k in range(ks.start, ks.stop):
            rows.append(shot_ref.cshot1344(b["xyz"][ps], b["normals"][ps], b["rgba"][ps], b["kp"][k], b["kp_rgba"][k], lrf[k], RADIUS))
    cnt = np.array([r.count for r in rows], np.int64)
    if color:
        return _rows_answer(np.array([r.desc for r in rows], F).reshape(-1, 1344), cnt, [not r.decided for r in rows],
                            bound=np.array([r.bound for r in rows]).reshape(-1, 1344), shape=np.array([r.shape for r in rows], F).reshape(-1, 352),
                            shape_bound=np.array([r.shape_bound for r in rows]).reshape(-1, 352))
    return _rows_answer(np.array([r.shape for r in rows], F).reshape(-1, 352), cnt, np.zeros(len(rows), bool),
                        bound=np.array([r.shape_bound for r in rows]).reshape(-1, 352))


def answer(T, lrf=None, rgb2lab=None, device=None):
    """The restatement of type T on the batch, object by object -> dict(rows [K, D], cnt [K], undecided [K] bool, ...).
    lrf: the frames [K, 9] the SHOT family is described on (default: frames()); rgb2lab: the oracle's CIELab (SHORT_CSHOT, CoSPAIR);
    device: what the restatements of CGF, RIFT and ESF_LOCAL take from the device, as their own tests hand it over --
    CGF dict(lrf, normals), RIFT dict(grad), ESF_LOCAL dict(scale); default: the restatement's own."""
    b = batch()
    lrf = frames()["frame"] if lrf is None else np.asarray(lrf, F).reshape(-1, 9)
    K = len(b["kp"])
    if T == "SHOT":
        return _shot(lrf, False)
    if T == "CSHOT":
        return _shot(lrf, True)
    if T == "BSHOT":
        a = _shot(lrf, False)
        live = ~np.isnan(a["rows"][:, 0])
        s, margin = bshot_ref.margins(a["rows"][live].astype(np.float64))
        decided = np.ones((K, 88), bool)
        decided[live] = (s == 0) | (margin >= 4e-4)             # the margin of test_gpu_bshot.py: four elements x the 1e-4 descriptor tolerance
        return _rows_answer(bshot_ref.binarize(a["rows"]), a["cnt"], np.zeros(K, bool), groups_decided=decided, shot=a["rows"])
    if T == "SHORT_SHOT":
        rows, cnt, frac, switch = short_shot_ref.short_shot_ref(b["pt_off"], b["xyz"], b["kp_off"], b["kp"], lrf, RADIUS, SHORT_BINS)
        return _rows_answer(rows, cnt, (switch < SWITCH_MARGIN) | ((frac != 0.0) & (frac < SWITCH_MARGIN)), switch=switch, frac=frac)
    if T == "SHORT_CSHOT":
        rows, cnt, switch = short_cshot_ref.short_cshot_ref(rgb2lab, b["pt_off"], b["xyz"], b["rgba"].astype(np.uint32), b["kp_off"], b["kp"],
                                                            b["kp_rgba"].astype(np.uint32), lrf, RADIUS, SHORT_BINS, SHORT_COLOR_BINS, SHORT_HIST)
        return _rows_answer(rows, cnt, switch < SWITCH_MARGIN, switch=switch)
    if T == "FPFH":
        r = fpfh_ref.fpfh33(b["pt_off"], b["xyz"], b["normals"], b["kp_off"], b["kp"], RADIUS)
        return _rows_answer(r.lo.astype(F), r.count, r.exempt, ref=r)
    if T == "CoSPAIR":
        r = cospair_ref.cospair(rgb2lab, b["pt_off"], b["xyz"], b["normals"], b["rgba"].astype(np.uint32), b["kp_off"], b["kp"], RADIUS)
        return _rows_answer(r.want_lo, r.n.sum(1), np.zeros(K, bool), ref=r)
    if T == "SpinImage":
        axes, idx = spin_image_ref.batch_normals(b["pt_off"], b["xyz"], b["normals"], b["kp_off"], b["kp"])
        a = spin_image_ref.spin_images(b["pt_off"], b["xyz"], b["kp_off"], b["kp"], axes, RADIUS, SPIN_WIDTH)
        und = np.zeros(K, bool); und[:] = a["undecided"] > 0      # a total over the batch: zero, or every keypoint counts as undecided
        return _rows_answer(a["rows"], a["cnt"], und, axes=axes, idx=idx)
    if T == "RSD":
        a = rsd_ref.rsd(b["pt_off"], b["xyz"], b["normals"], b["kp_off"], b["kp"], RADIUS)
        return _rows_answer(a["row_lo"], a["cnt"], np.zeros(K, bool), ref=a)
    if T == "RIFT":
        def one(ps, ks, o):
            ga = rift_gradients(o)
            g = ga["grad"].astype(F) if device is None else np.asarray(device["grad"], F)[ps]
            want = rift_ref.rift(b["xyz"][ps], g, b["kp"][ks], RADIUS, undecided_points=ga["undecided"])
            return dict(rows=want["rows"], cnt=want["count"], undecided=want["undecided"], tol=want["tol"])
        return _per_object(one)
    if T == "CGF":
        R, _rmin, rl = cgf_ref.radii(CGF_RADIUS)
        if device is None:
            fr = frames(rl)["frame"]
            nrm = np.concatenate([cgf_ref.pca_normal(b["xyz"][ps], b["kp"][ks], 0.1 * R)[0] for ps, ks in objects()]).astype(F)
        else:
            fr, nrm = np.asarray(device["lrf"], F).reshape(-1, 9), np.asarray(device["normals"], F).reshape(-1, 3)

        def one(ps, ks, o):
            a = cgf_ref.raw(b["xyz"][ps], b["kp"][ks], fr[ks], nrm[ks], CGF_RADIUS)
            return dict(raw=a["rows"], sum=a["sum"], undecided=a["undecided"], ball=a["ball"])
        a = _per_object(one)
        y, e = cgf_ref.mlp(a["raw"], cgf_layers())
        return _rows_answer(y, a["sum"], a["undecided"], raw=a["raw"], bound=e, ball=a["ball"])
    if T == "ESF_LOCAL":
        a = esf_ref.esf_local(b["pt_off"], b["xyz"], b["kp_off"], b["kp"], ESF_RADIUS, ESF_SAMPLES, scale=None if device is None else device["scale"])
        rows = np.where(a["nan"][:, None], np.nan, a["lo"].astype(np.float64))
        return _rows_answer(rows, a["cnt"], a["whole"], ref=a)
    raise ValueError(T)


@functools.lru_cache(maxsize=None)
def rift_gradients(o):
    """rift_ref.gradients of object o at RADIUS"""
    b = batch()
    ps, _ks = objects()[o]
    return rift_ref.gradients(b["xyz"][ps], b["normals"][ps], b["rgba"][ps], RADIUS)


def special_rows(T, a):
    """(all-NaN rows, all-zero rows, finite rows with a non-zero) of an answer, as row masks"""
    r = np.asarray(a["rows"], np.float64)
    nan = np.isnan(r).all(1)
    zero = ~nan & ~np.isnan(r).any(1) & ~r.any(1)
    return nan, zero, ~nan & ~np.isnan(r).any(1) & r.any(1)


# ------------------------------------------------------------------------------------------------------------------ cloud passes and detectors
ISS_SALIENT, ISS_NONMAX, ISS_GAMMA, ISS_MIN_NEIGHBORS = 0.15, 0.1, 0.975, 5       # iss3d_scenes.SCENES[2]: 700 points
CULL_LEAF, CULL_MAX_DIST = 0.2, 0.05                                              # test_gpu_culling.py: LEAF, MAX_DIST
SIFT_MIN_SCALE, SIFT_OCTAVES, SIFT_SCALES = 0.045, 4, 3                           # sift3d_scenes.SCENES[2]: 700 points


def cloud_of(o):
    """(xyz, normals, rgba uint32, intensity) of object o"""
    b = batch()
    ps, _ks = objects()[o]
    return b["xyz"][ps], b["normals"][ps], b["rgba"][ps].astype(np.uint32), b["intensity"][ps]


@functools.lru_cache(maxsize=None)
def iss3d_answer(o):
    import iss3d_ref
    return iss3d_ref.iss3d(cloud_of(o)[0], ISS_SALIENT, ISS_NONMAX, ISS_GAMMA, ISS_GAMMA, ISS_MIN_NEIGHBORS)


@functools.lru_cache(maxsize=None)
def pc_answer(o):
    import culling_ref
    xyz, nrm, _c, _i = cloud_of(o)
    return culling_ref.principal_curvatures(xyz, nrm, CULL_LEAF)


@functools.lru_cache(maxsize=None)
def voxel_answer(o):
    """the voxel keypoints of object o at CULL_LEAF by voxel_ref.py -> (kp float32 [m, 3], rgba uint32 [m])"""
    import voxel_ref
    xyz, _n, rgba, _i = cloud_of(o)
    v = voxel_ref.voxel_ref(xyz, CULL_LEAF, rgba)
    return v["xyz"].astype(F).reshape(-1, 3), v["rgba"]


def culling_answer(o, rgb2lab, kp=None, kp_rgba=None):
    """culling_ref.py on object o and the keypoints kp (default: voxel_answer's) -> dict(curvature, kpq: culling_ref.scores, select: the
    default selection (kpq and colour distance, RequireCombinedList) on the restatement's own scores)"""
    import culling_ref
    xyz, _n, rgba, _i = cloud_of(o)
    if kp is None:
        kp, kp_rgba = voxel_answer(o)
    lab = culling_ref.lab_table(rgb2lab, rgba) if len(rgba) else np.zeros((0, 3), F)
    kp_lab = culling_ref.lab_table(rgb2lab, kp_rgba) if len(kp) else np.zeros((0, 3), F)
    curv = culling_ref.scores(xyz, kp, CULL_LEAF, "curvature", "colordistance", CULL_MAX_DIST, lab=lab, kp_lab=kp_lab)
    kpq = culling_ref.scores(xyz, kp, CULL_LEAF, "kpq", pc=pc_answer(o))
    return dict(curvature=curv, kpq=kpq, select=culling_ref.select(kpq["geo"], curv["color"]))


@functools.lru_cache(maxsize=None)
def sift_scales():
    import sift3d_ref
    return sift3d_ref.scales(SIFT_MIN_SCALE, SIFT_SCALES)


@functools.lru_cache(maxsize=None)
def sift3d_answer(o):
    """sift3d_ref.py on object o at the scales of the first octave -> dict(dog, bound, count, flags, undecided, nn)"""
    import sift3d_ref
    xyz, _n, _c, inten = cloud_of(o)
    D, B, cnt = sift3d_ref.dog(xyz, inten, sift_scales())
    flags, und, nn = sift3d_ref.extrema(xyz, D, B)
    return dict(dog=D, bound=B, count=cnt, flags=flags, undecided=und, nn=nn)


def object_maxima(rgb2lab=None):
    """what the four one-block-per-object reductions return, by the restatements: dict name -> float64 [N_OBJ]
    nmax (k_cull_nmax): the largest squared normal length over the finite normals of the finite points; kmax (k_cull_kmax): the largest
    finite |pc1 * pc2|; imax (k_sift_imax): the largest finite |I| of the finite points; gmax (k_rift_gmax): the largest finite |gradient|"""
    out = dict(nmax=np.zeros(N_OBJ), kmax=np.zeros(N_OBJ), imax=np.zeros(N_OBJ), gmax=np.zeros(N_OBJ))
    for o in range(N_OBJ):
        xyz, nrm, _c, inten = cloud_of(o)
        fin = np.isfinite(xyz).all(1) if len(xyz) else np.zeros(0, bool)
        ok = fin & np.isfinite(nrm).all(1)
        if ok.any():
            out["nmax"][o] = (nrm[ok].astype(np.float64) ** 2).sum(1).max()
        pc = pc_answer(o)
        K = np.abs((pc["pc1"] * pc["pc2"]).astype(F))
        if np.isfinite(K).any():
            out["kmax"][o] = K[np.isfinite(K)].max()
        use = fin & np.isfinite(inten)
        if use.any():
            out["imax"][o] = np.abs(inten[use]).max()
        g = np.linalg.norm(rift_gradients(o)["grad"].astype(F).astype(np.float64), axis=1)
        if np.isfinite(g).any():
            out["gmax"][o] = g[np.isfinite(g)].max()
    return out


CURV_RADIUS = 0.1             # ismhip_normal_curvature: SIFT3D's NormalRadius at this density


@functools.lru_cache(maxsize=None)
def curvature_answer(o):
    """culling_ref.scores "curvature" with every point of object o as its own keypoint: what ismhip_normal_curvature computes"""
    import culling_ref
    xyz = cloud_of(o)[0]
    return culling_ref.scores(xyz, xyz, CURV_RADIUS, "curvature")
