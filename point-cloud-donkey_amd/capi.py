"""ctypes binding of libismhip.so (include/ismhip.h) for the Python test / bench harness.

The product is the shared library; this module only marshals pointers. torch is used for device memory
(tensor.data_ptr()) and streams; no torch type crosses the C ABI. There is no CPU fallback: if the
library or a gfx950 device is missing, loading / ctx creation raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libismhip.so")

METRIC_L2SQ, METRIC_CHI2 = 0, 1
W_CLASS, W_VOTE, W_MATCHING, W_CODEWORD = 1, 2, 4, 8
KERNEL_GAUSSIAN, KERNEL_UNIFORM = 0, 1
SUPPRESS_AVERAGE, SUPPRESS_SUPPRESS, SUPPRESS_NONE = 0, 1, 2
MAXFILTER_NONE, MAXFILTER_SIMPLE, MAXFILTER_MERGE = 0, 1, 2
SOM_MEANSHIFT, SOM_BANDWIDTH, SOM_MODEL_RADIUS, SOM_COMPLETE_VOTING_SPACE = 0, 1, 2, 3
ERR_NODEVICE = -5

EXPORTS = [
    "ismhip_abi_version", "ismhip_ctx_create", "ismhip_ctx_create_on_stream", "ismhip_ctx_destroy", "ismhip_sync", "ismhip_last_error",
    "ismhip_timers_enable", "ismhip_timers_reset", "ismhip_timer_get",
    "ismhip_cloud_create", "ismhip_cloud_destroy", "ismhip_cloud_centroids", "ismhip_cloud_radii", "ismhip_estimate_normals", "ismhip_estimate_normals_pca",
    "ismhip_shot_lrf", "ismhip_shotna_lrf", "ismhip_shot352", "ismhip_cshot1344", "ismhip_fpfh33", "ismhip_center_dist",
    "ismhip_compact_features", "ismhip_compact_descriptor_rows", "ismhip_filter_normals", "ismhip_voxel_keypoints", "ismhip_gather_columns",
    "ismhip_codebook_create", "ismhip_codebook_set_word_class", "ismhip_codebook_destroy", "ismhip_codebook_max_votes_per_word", "ismhip_codebook_stage1_dims", "ismhip_codebook_stage2_dims", "ismhip_codebook_rotate_probe",
    "ismhip_knn", "ismhip_knn_ratio", "ismhip_knn_rule", "ismhip_cast_votes", "ismhip_find_maxima", "ismhip_hough3d_maxima", "ismhip_train_activate", "ismhip_kmeans",
    "ismhip_knn_threshold", "ismhip_cast_votes_csr", "ismhip_train_activate_lists", "ismhip_knn_large_k",
    "ismhip_filter_statistical", "ismhip_filter_radius", "ismhip_filter_passthrough_z", "ismhip_compact_points",
    "ismhip_codebook_set_word_keypoint", "ismhip_vote_keypoints", "ismhip_vote_keypoints_csr", "ismhip_ransac_filter", "ismhip_ransac_hypothesis",
    "ismhip_find_maxima_ransac", "ismhip_hough3d_maxima_ransac", "ismhip_short_shot", "ismhip_short_cshot", "ismhip_cospair",
    "ismhip_bshot_binarize", "ismhip_bshot352", "ismhip_codebook_make_binary", "ismhip_codebook_has_binary", "ismhip_knn_binary",
    "ismhip_rank_scores", "ismhip_rank_select", "ismhip_global_short_shot", "ismhip_global_shot352", "ismhip_global_vfh",
    "ismhip_iss3d_saliency", "ismhip_iss3d_keypoints", "ismhip_keypoint_normals", "ismhip_spin_image", "ismhip_rsd",
    "ismhip_principal_curvatures", "ismhip_culling_scores", "ismhip_culling_select", "ismhip_intensity_gradients", "ismhip_rift",
    "ismhip_keypoint_normals_pca", "ismhip_cgf_raw", "ismhip_mlp_create", "ismhip_mlp_destroy", "ismhip_mlp_in", "ismhip_mlp_out", "ismhip_mlp_forward",
    "ismhip_cgfw_open", "ismhip_cgfw_close", "ismhip_cgfw_layers", "ismhip_cgfw_layer", "ismhip_mlp_from_cgfw", "ismhip_rgb2lab",
    "ismhip_esf_local", "ismhip_global_gasd", "ismhip_gasd_hue_bins", "ismhip_region_mvbb", "ismhip_global_cvfh",
    "ismhip_normal_curvature", "ismhip_voxel_downsample_xyzi", "ismhip_sift3d_scale_space", "ismhip_sift3d_extrema", "ismhip_sift3d_keypoints",
    "ismhip_point_density", "ismhip_usc_tables", "ismhip_usc",
]
SIFT3D_MIN_POINTS = 25             # ISMHIP_SIFT3D_MIN_POINTS: an octave below it ends the object; also the extrema's number of neighbours
# KeypointsVoxelGridCulling: method and type strings as the reference compares them (lower-cased; CombineFilters is case-sensitive)
CULLING_GEOMETRY = {"none": 0, "curvature": 1, "kpq": 2}
CULLING_COLOR = {"none": 0, "colordistance": 1}
CULLING_TYPE = {"cutoff": 0, "threshold": 1}
CULLING_COMBINE = {"RequireOne": 0, "RequireBoth": 1, "RequireCombinedList": 2}
RANSAC_MAX_ITERATIONS = 10000      # corr_rejector.setMaximumIterations (voting.cpp:398)
RANSAC_SEED = 12345                # PCL seeds mt19937(12345) per cluster; the draws themselves are this library's


class MaximaParams(C.Structure):
    _fields_ = [("n_classes", C.c_int), ("class_bandwidth_h", C.c_void_p), ("bandwidth", C.c_float),
                ("threshold", C.c_float), ("max_iter", C.c_int), ("kernel", C.c_int), ("suppression", C.c_int),
                ("min_votes_threshold", C.c_int), ("min_threshold", C.c_float), ("best_k", C.c_int),
                ("max_maxima", C.c_int), ("max_filter", C.c_int),
                ("vote_bbox_quat", C.c_void_p), ("max_bbox_quat_out", C.c_void_p), ("single_object_max_type", C.c_int),
                ("object_centroid", C.c_void_p), ("object_radius", C.c_void_p)]


class HoughParams(C.Structure):
    _fields_ = [("n_classes", C.c_int), ("min_coord", C.c_float * 3), ("max_coord", C.c_float * 3), ("bin_size", C.c_float),
                ("class_bin_h", C.c_void_p), ("use_interpolation", C.c_int), ("rel_threshold", C.c_float),
                ("min_votes_threshold", C.c_int), ("min_threshold", C.c_float), ("best_k", C.c_int), ("max_maxima", C.c_int), ("max_filter", C.c_int),
                ("vote_bbox_quat", C.c_void_p), ("max_bbox_quat_out", C.c_void_p)]


class RansacParams(C.Structure):
    _fields_ = [("vote_keypoint", C.c_void_p), ("vote_keypoint_training", C.c_void_p), ("inlier_threshold", C.c_float),
                ("class_inlier_threshold_h", C.c_void_p), ("max_iterations", C.c_int), ("seed", C.c_ulonglong)]


class IsmHipError(RuntimeError):
    pass


_lib = None


def lib():
    """Loads libismhip.so (once). Raises if it has not been built — the hot path has no other back end."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IsmHipError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C point-cloud-donkey_amd/csrc)")
        # torch ships its own libamdhip64 (same SONAME as /opt/rocm's): import it FIRST so that the process holds exactly
        # one HIP runtime and libismhip.so binds to the one that owns torch's device memory and streams.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.ismhip_last_error.restype = C.c_char_p
        L.ismhip_last_error.argtypes = [C.c_void_p]
        for name in EXPORTS:
            fn = getattr(L, name)
            if name != "ismhip_last_error":
                fn.restype = C.c_int
        _lib = L
    return _lib


def _p(t):
    """device pointer of a torch tensor / host pointer of a numpy array / None"""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return C.c_void_p(t.ctypes.data)
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


class Ctx:
    def __init__(self, device=0, stream="torch"):
        """stream: "torch" = torch's current stream on the device (library work is then ordered with torch ops and
        tensor.cpu() waits for it), None = a private non-blocking stream, or a raw hipStream_t value."""
        self._h = C.c_void_p()
        L = lib()
        if stream is None:
            rc = L.ismhip_ctx_create(C.c_int(device), C.c_void_p(0), C.byref(self._h))
        else:
            if stream == "torch":
                import torch
                if not torch.cuda.is_available():
                    raise IsmHipError("no gfx950 device visible: the hot path has no CPU fallback (ISMHIP_ERR_NODEVICE)")
                if not (0 <= device < torch.cuda.device_count()):
                    raise IsmHipError(f"device {device} out of range (ISMHIP_ERR_INVALID)")
                stream = torch.cuda.current_stream(device).cuda_stream
            rc = L.ismhip_ctx_create_on_stream(C.c_int(device), C.c_void_p(stream), C.byref(self._h))
        if rc != 0:
            raise IsmHipError(f"ismhip_ctx_create failed ({rc}); a gfx950 device is required, there is no CPU fallback")
        self.device = device

    def check(self, rc, what):
        if rc != 0:
            raise IsmHipError(f"{what} failed ({rc}): {lib().ismhip_last_error(self._h).decode()}")

    def sync(self):
        self.check(lib().ismhip_sync(self._h), "ismhip_sync")

    def timers_enable(self, on=True):
        self.check(lib().ismhip_timers_enable(self._h, C.c_int(1 if on else 0)), "timers_enable")

    def timers_reset(self):
        self.check(lib().ismhip_timers_reset(self._h), "timers_reset")

    def timer(self, name):
        ms, n = C.c_double(), C.c_int64()
        self.check(lib().ismhip_timer_get(self._h, name.encode(), C.byref(ms), C.byref(n)), "timer_get")
        return ms.value, n.value

    def close(self):
        if self._h:
            lib().ismhip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Cloud:
    """ismhip_cloud: search surface of a batch of objects (device SoA tensors are borrowed, keep them alive)."""

    def __init__(self, ctx, pt_offsets, x, y, z, nx, ny, nz, cell_size, rgba=None):
        self.ctx = ctx
        self.pt_offsets = _u32(pt_offsets)
        self.n_obj = len(self.pt_offsets) - 1
        self._keep = (x, y, z, nx, ny, nz, rgba)
        self._h = C.c_void_p()
        rc = lib().ismhip_cloud_create(ctx._h, C.c_int(self.n_obj), _p(self.pt_offsets), _p(x), _p(y), _p(z), _p(nx), _p(ny),
                                       _p(nz), _p(rgba), C.c_float(cell_size), C.byref(self._h))
        ctx.check(rc, "ismhip_cloud_create")

    def close(self):
        if self._h:
            lib().ismhip_cloud_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Codebook:
    def __init__(self, ctx, words, vote_offsets, vote_xyz, vote_class, vote_instance, n_classes, class_sigma,
                 word_weight=None, vote_weight=None, vote_class_weight=None, vote_bbox_quat=None, vote_bbox_size=None):
        f32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        self.ctx = ctx
        words = f32(words)
        self.n_words, self.dim = words.shape
        self.n_classes = int(n_classes)
        self._h = C.c_void_p()
        rc = lib().ismhip_codebook_create(ctx._h, C.c_int(self.n_words), C.c_int(self.dim), _p(words), _p(f32(word_weight)),
                                          _p(_u32(vote_offsets)), _p(f32(vote_xyz)), _p(f32(vote_weight)),
                                          _p(f32(vote_class_weight)), _p(_u32(vote_class)), _p(_u32(vote_instance)),
                                          _p(f32(vote_bbox_quat)), _p(f32(vote_bbox_size)), C.c_int(self.n_classes),
                                          _p(f32(class_sigma)), C.byref(self._h))
        ctx.check(rc, "ismhip_codebook_create")
        self.max_votes = lib().ismhip_codebook_max_votes_per_word(self._h)
        e = C.c_float(1.0)
        self.stage1_dims = int(lib().ismhip_codebook_stage1_dims(self._h, C.byref(e)))     # 0: squared-L2 candidates on all dimensions
        self.stage1_energy = float(e.value)
        self.stage2_dims = int(lib().ismhip_codebook_stage2_dims(self._h, C.byref(e)))     # 0: stage 2 of the squared-L2 search on all dimensions
        self.stage2_energy = float(e.value)

    def rotate_probe(self, q, stage=1):
        """ismhip_codebook_rotate_probe: (image [nq, m] float16, |q|^2 [nq], sums of squares of the image rows [nq], R [m, dim_pad],
        scale, d_rel, d_abs) of the rotated image the search makes of the device rows q [nq, dim]; None when the codebook has none."""
        torch = _torch()
        consts = np.zeros(3, np.float32)
        m = lib().ismhip_codebook_rotate_probe(self.ctx._h, self._h, C.c_int(stage), C.c_int(0), None, None, None, None, None, _p(consts))
        if m < 0:
            self.ctx.check(m, "ismhip_codebook_rotate_probe")
        if m == 0:
            return None
        nq = int(q.shape[0])
        dim_pad = (self.dim + 31) // 32 * 32
        R = np.zeros((m, dim_pad), np.float32)
        img = torch.empty((nq, m), dtype=torch.float16, device=q.device)
        qn2 = torch.empty(nq, dtype=torch.float32, device=q.device)
        qn2h = torch.empty(nq, dtype=torch.float32, device=q.device)
        rc = lib().ismhip_codebook_rotate_probe(self.ctx._h, self._h, C.c_int(stage), C.c_int(nq), _p(q), _p(img), _p(qn2), _p(qn2h), _p(R), _p(consts))
        if rc < 0:
            self.ctx.check(rc, "ismhip_codebook_rotate_probe")
        return img.cpu().numpy(), qn2.cpu().numpy(), qn2h.cpu().numpy(), R, float(consts[0]), float(consts[1]), float(consts[2])

    def set_word_class(self, word_class):
        self.ctx.check(lib().ismhip_codebook_set_word_class(self.ctx._h, self._h, _p(_u32(word_class))), "ismhip_codebook_set_word_class")

    def set_word_keypoint(self, word_keypoint):
        """[n_words, 3] training keypoint of every codeword (Codeword::getFeaturePosition): the RANSAC vote filter's source points"""
        kp = np.ascontiguousarray(np.asarray(word_keypoint, dtype=np.float32))
        assert kp.shape == (self.n_words, 3)
        self.ctx.check(lib().ismhip_codebook_set_word_keypoint(self.ctx._h, self._h, _p(kp)), "ismhip_codebook_set_word_keypoint")

    def make_binary(self):
        """ismhip_codebook_make_binary: the int8 image of a codebook of zeros and ones, which knn_binary searches. Raises IsmHipError
        "(-1)" when an element is neither (the codebook stays as it was), "(-4)" when the search key does not fit."""
        self.ctx.check(lib().ismhip_codebook_make_binary(self.ctx._h, self._h), "ismhip_codebook_make_binary")

    @property
    def has_binary(self):
        return lib().ismhip_codebook_has_binary(self._h) == 1

    def close(self):
        if self._h:
            lib().ismhip_codebook_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _torch():
    import torch
    return torch


def shot_lrf(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius):
    torch = _torch()
    ko = _u32(kp_offsets)
    out = torch.empty((int(ko[-1]), 9), dtype=torch.float32, device=kpx.device)
    ctx.check(lib().ismhip_shot_lrf(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), _p(out)), "ismhip_shot_lrf")
    return out


def shotna_lrf(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius):
    """ismhip_shotna_lrf: the SHOT frame with the z sign voted by the normals the cloud holds at this moment (ReferenceFrameType "SHOTNA")"""
    torch = _torch()
    ko = _u32(kp_offsets)
    out = torch.empty((int(ko[-1]), 9), dtype=torch.float32, device=kpx.device)
    ctx.check(lib().ismhip_shotna_lrf(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), _p(out)), "ismhip_shotna_lrf")
    return out


LRF_TYPES = {"SHOT": shot_lrf, "SHOTNA": shotna_lrf}      # Features.ReferenceFrameType -> the call ("BOARD" and "FLARE" are not built)


def shot352(ctx, cloud, kp_offsets, kpx, kpy, kpz, lrf, radius, want_counts=False):
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, 352), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_shot352(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(lrf), C.c_float(radius), _p(out), _p(cnt)),
              "ismhip_shot352")
    return (out, cnt) if want_counts else out


def bshot_binarize(ctx, src, out=None):
    """ismhip_bshot_binarize of the rows src [n, 352] -> [n, 352] of 0.0 / 1.0; out may be src itself (in place)"""
    torch = _torch()
    assert src.dim() == 2 and src.shape[1] == 352 and src.dtype == torch.float32
    if out is None:
        out = torch.empty_like(src)
    ctx.check(lib().ismhip_bshot_binarize(ctx._h, C.c_int(src.shape[0]), _p(src), _p(out)), "ismhip_bshot_binarize")
    return out


def bshot352(ctx, cloud, kp_offsets, kpx, kpy, kpz, lrf, radius, want_counts=False):
    """ismhip_bshot352: the arguments and counts of shot352, the rows binarised"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, 352), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_bshot352(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(lrf), C.c_float(radius), _p(out), _p(cnt)),
              "ismhip_bshot352")
    return (out, cnt) if want_counts else out


def cshot1344(ctx, cloud, kp_offsets, kpx, kpy, kpz, kp_rgba, lrf, radius, want_counts=False):
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, 1344), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_cshot1344(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(kp_rgba), _p(lrf), C.c_float(radius),
                                     _p(out), _p(cnt)), "ismhip_cshot1344")
    return (out, cnt) if want_counts else out


def rgb2lab(ctx, rgba, normalised=False):
    """ismhip_rgb2lab (diagnostic): CIELab of the packed colours rgba (int32 device tensor [n]) -> float32 [n, 3] on the same device"""
    torch = _torch()
    assert rgba.dim() == 1 and rgba.dtype == torch.int32
    out = torch.empty((rgba.shape[0], 3), dtype=torch.float32, device=rgba.device)
    ctx.check(lib().ismhip_rgb2lab(ctx._h, C.c_int(rgba.shape[0]), _p(rgba), C.c_int(1 if normalised else 0), _p(out)), "ismhip_rgb2lab")
    return out


def short_shot(ctx, cloud, kp_offsets, kpx, kpy, kpz, lrf, radius, bins=(2, 2, 8), min_radius=0.0, log_radius=False, want_counts=False):
    """ismhip_short_shot on the (r, e, a) bins -> [nkp, r * e * a]; min_radius is the absolute one (short_shot_min_radius derives it)"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    r, e, a = (int(b) for b in bins)
    out = torch.empty((n, max(r * e * a, 0) if min(r, e, a) > 0 else 0), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_short_shot(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(lrf), C.c_float(radius), C.c_float(min_radius),
                                      C.c_int(1 if log_radius else 0), C.c_int(r), C.c_int(e), C.c_int(a), _p(out), _p(cnt)), "ismhip_short_shot")
    return (out, cnt) if want_counts else out


SHORT_SHOT_AUTO_BINS = {8: (1, 1, 8), 16: (2, 2, 4), 24: (2, 2, 6), 32: (2, 2, 8), 64: (2, 4, 8), 96: (3, 4, 8), 128: (4, 4, 8), 192: (6, 4, 8),
                        256: (8, 4, 8)}


def short_shot_grid(dims=32, bin_type="auto", bins=(2, 2, 8)):
    """FeaturesSHORTSHOT::configureSphericalGrid (features_short_shot.cpp:285-366) -> (dims, (r, e, a)): "auto" maps the nine sizes,
    "manual" takes the bins; an unknown size or bin type falls back to 32 / (2, 2, 8) as the reference does (with its LOG_ERROR)"""
    if bin_type == "manual":
        r, e, a = (int(b) for b in bins)
        return r * e * a, (r, e, a)
    if bin_type == "auto" and int(dims) in SHORT_SHOT_AUTO_BINS:
        return int(dims), SHORT_SHOT_AUTO_BINS[int(dims)]
    return 32, (2, 2, 8)


def short_shot_min_radius(radius, use_min_radius=False, min_radius_relative=0.0, log_radius=False):
    """the absolute minimum radius of compute_descriptor (:88-103) as the float the C ABI takes"""
    if use_min_radius:
        return float(np.float32(float(np.float32(radius)) * float(min_radius_relative)))
    return float(np.float32(float(np.float32(radius)) * float(np.float32(0.1)))) if log_radius else 0.0


def short_cshot(ctx, cloud, kp_offsets, kpx, kpy, kpz, kp_rgba, lrf, radius, bins=(2, 2, 8), color_bins=(2, 2, 8), hist_size=15, min_radius=0.0,
                log_radius=False, want_counts=False):
    """ismhip_short_cshot on the shape bins (r, e, a), the colour grid (rc, ec, ac) and hist_size colour bins per cell ->
    [nkp, r * e * a + rc * ec * ac * hist_size]; min_radius is the absolute one (short_shot_min_radius derives it)"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    r, e, a = (int(b) for b in bins)
    rc, ec, ac = (int(b) for b in color_bins)
    h = int(hist_size)
    out = torch.empty((n, r * e * a + rc * ec * ac * h if min(r, e, a, rc, ec, ac, h) > 0 else 0), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_short_cshot(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(kp_rgba), _p(lrf), C.c_float(radius),
                                       C.c_float(min_radius), C.c_int(1 if log_radius else 0), C.c_int(r), C.c_int(e), C.c_int(a), C.c_int(rc),
                                       C.c_int(ec), C.c_int(ac), C.c_int(h), _p(out), _p(cnt)), "ismhip_short_cshot")
    return (out, cnt) if want_counts else out


SHORT_CSHOT_COLOR_BINS = {d: SHORT_SHOT_AUTO_BINS[d] for d in (8, 16, 24, 32, 64, 96, 128)}


def short_cshot_color_grid(dims=32):
    """FeaturesSHORTCSHOT::configureSphericalColorGrid (features_short_cshot.cpp:592-646) -> (dims, (rc, ec, ac)): the seven sizes; any
    other falls back to 32 / (2, 2, 8) as the reference does (with its LOG_ERROR). There is no manual colour grid."""
    if int(dims) in SHORT_CSHOT_COLOR_BINS:
        return int(dims), SHORT_CSHOT_COLOR_BINS[int(dims)]
    return 32, (2, 2, 8)


COSPAIR_LEVELS, COSPAIR_BINS, COSPAIR_DIM = 7, 9, 378


def cospair(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius, want_counts=False, want_levels=False, want_snap=False):
    """ismhip_cospair -> [nkp, 378]; with want_counts the pairs per keypoint [nkp], with want_levels the pairs per level [nkp, 7], with
    want_snap the object-local original index of the snapped cloud point [nkp] (-1 for a NaN row), appended in this order"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, COSPAIR_DIM), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    lev = torch.empty((n, COSPAIR_LEVELS), dtype=torch.int32, device=kpx.device) if want_levels else None
    snap = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_snap else None
    ctx.check(lib().ismhip_cospair(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), _p(out), _p(cnt), _p(lev), _p(snap)),
              "ismhip_cospair")
    extra = [t for t in (cnt, lev, snap) if t is not None]
    return (out, *extra) if extra else out


SPIN_IMAGE_WIDTH = 8                                                   # setImageWidth(8), features_spin_image.cpp:67
SPIN_IMAGE_DIM = (SPIN_IMAGE_WIDTH + 1) * (2 * SPIN_IMAGE_WIDTH + 1)   # 153


def keypoint_normals(ctx, cloud, kp_offsets, kpx, kpy, kpz, want_index=False):
    """ismhip_keypoint_normals -> (nx, ny, nz) [nkp] each: the installed normal of the lowest-index cloud point whose coordinates equal the
    keypoint's, (0, 0, 0) when there is none; with want_index also that object-local index [nkp] int32 (-1: none)"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    nx, ny, nz = (torch.empty((n,), dtype=torch.float32, device=kpx.device) for _ in range(3))
    src = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_index else None
    ctx.check(lib().ismhip_keypoint_normals(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(nx), _p(ny), _p(nz), _p(src)),
              "ismhip_keypoint_normals")
    return (nx, ny, nz, src) if want_index else (nx, ny, nz)


def spin_image(ctx, cloud, kp_offsets, kpx, kpy, kpz, ax, ay, az, radius, image_width=SPIN_IMAGE_WIDTH, want_counts=False):
    """ismhip_spin_image about the axes (ax, ay, az) -> [nkp, (w + 1)(2w + 1)]; with want_counts the neighbours per keypoint [nkp]"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    w = int(image_width)
    out = torch.empty((n, (w + 1) * (2 * w + 1) if w >= 1 else 0), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_spin_image(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(ax), _p(ay), _p(az), C.c_float(radius), C.c_int(w),
                                      _p(out), _p(cnt)), "ismhip_spin_image")
    return (out, cnt) if want_counts else out


RSD_DIM, RSD_RADII_DIM = 25, 2


def rsd(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius, full_histogram=True, want_counts=False):
    """ismhip_rsd -> [nkp, 25] (the angle-distance histogram of all neighbour pairs over 300) or, without full_histogram, [nkp, 2] (the
    two principal radii); with want_counts the neighbours per keypoint [nkp]"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, RSD_DIM if full_histogram else RSD_RADII_DIM), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_rsd(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), C.c_int(1 if full_histogram else 0),
                               _p(out), _p(cnt)), "ismhip_rsd")
    return (out, cnt) if want_counts else out


ESF_DIM = 640                # ten blocks of 64 bins
ESF_SAMPLES = 20000          # PCL's sample_size (ISMHIP_ESF_SAMPLES)
ESF_SEED = 0x45534631        # ISMHIP_ESF_SEED


def esf_local(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius, n_samples=ESF_SAMPLES, seed=ESF_SEED, want_counts=False, want_bins=False,
              want_scale=False):
    """ismhip_esf_local -> [nkp, 640] (the ensemble of shape functions of every keypoint's ball); then, for every want_* set and in this
    order: the neighbours per keypoint [nkp] int32, the integer numerators of the bins in sixths [nkp, 640] int32, and (centroid x, y, z,
    largest distance from it) [nkp, 4] float32"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, ESF_DIM), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    bins = torch.empty((n, ESF_DIM), dtype=torch.int32, device=kpx.device) if want_bins else None
    scale = torch.empty((n, 4), dtype=torch.float32, device=kpx.device) if want_scale else None
    ctx.check(lib().ismhip_esf_local(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), C.c_int(int(n_samples)),
                                     C.c_uint32(int(seed) & 0xffffffff), _p(out), _p(cnt), _p(bins), _p(scale)), "ismhip_esf_local")
    extra = [t for t in (cnt, bins, scale) if t is not None]
    return (out, *extra) if extra else out


KNN_MAX_DIM = 2048                 # ISMHIP_KNN_MAX_DIM: the longest row of Codebook, knn (K <= 16), knn_ratio, knn_rule, train_activate, kmeans
USC_DIM = 1960                     # ISMHIP_USC_DIM: 14 azimuth x 14 elevation x 10 radial bins
USC_POINT_DENSITY_RADIUS = 0.1     # as ism3d.h: the value pcl::UniqueShapeContext's constructor is recalled to set; the reference leaves it there


def point_density(ctx, cloud, density_radius):
    """ismhip_point_density -> int32 [n_pts] in cloud order: the object's finite points within density_radius of every point, itself
    included (0 for a point that is not finite)"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    out = torch.zeros((n,), dtype=torch.int32, device=dev)
    ctx.check(lib().ismhip_point_density(ctx._h, cloud._h, C.c_float(density_radius), _p(out)), "ismhip_point_density")
    return out


def usc_tables(radius, min_radius):
    """ismhip_usc_tables -> (lut float64 [10, 14] by (radial, elevation) bin, edges float32 [11]); ValueError for radii ismhip_usc refuses"""
    import numpy as np
    lut = np.empty(140, np.float64)
    edges = np.empty(11, np.float32)
    rc = lib().ismhip_usc_tables(C.c_float(radius), C.c_float(min_radius), C.c_void_p(lut.ctypes.data), C.c_void_p(edges.ctypes.data))
    if rc != 0:
        raise ValueError(f"ismhip_usc_tables: radius {radius}, min_radius {min_radius} refused ({rc})")
    return lut.reshape(10, 14), edges


def usc(ctx, cloud, kp_offsets, kpx, kpy, kpz, lrf, radius, min_radius, density, want_counts=False, want_q=False):
    """ismhip_usc in the frames lrf [nkp, 9] with the densities of point_density -> [nkp, 1960]; then, for every want_* set and in this
    order: the neighbours per keypoint [nkp] int32 and the integer bins Q [nkp, 1960] int64"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, USC_DIM), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    q = torch.empty((n, USC_DIM), dtype=torch.int64, device=kpx.device) if want_q else None
    ctx.check(lib().ismhip_usc(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(lrf), C.c_float(radius), C.c_float(min_radius),
                               _p(density), _p(out), _p(cnt), _p(q)), "ismhip_usc")
    extra = [t for t in (cnt, q) if t is not None]
    return (out, *extra) if extra else out


RIFT_DISTANCE_BINS, RIFT_GRADIENT_BINS = 8, 16       # features_rift.cpp:38-39
RIFT_DIM = RIFT_DISTANCE_BINS * RIFT_GRADIENT_BINS   # 128


def intensity_gradients(ctx, cloud, radius, want_counts=False):
    """ismhip_intensity_gradients -> [n_pts, 3] float32 in the cloud's original point order (NaN where the ball holds fewer than three
    points or the position or normal is not finite); with want_counts the ball's points per cloud point [n_pts] int32"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    grad = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev) if want_counts else None
    ctx.check(lib().ismhip_intensity_gradients(ctx._h, cloud._h, C.c_float(radius), _p(grad), _p(cnt)), "ismhip_intensity_gradients")
    return (grad, cnt) if want_counts else grad


def rift(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius, grad, n_distance_bins=RIFT_DISTANCE_BINS, n_gradient_bins=RIFT_GRADIENT_BINS,
         want_counts=False):
    """ismhip_rift from the gradients of intensity_gradients -> [nkp, n_distance_bins * n_gradient_bins], gradient-major; with want_counts
    the neighbours per keypoint [nkp]"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    nd, ng = int(n_distance_bins), int(n_gradient_bins)
    out = torch.empty((n, max(nd, 0) * max(ng, 0)), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_rift(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), C.c_int(nd), C.c_int(ng), _p(grad),
                                _p(out), _p(cnt)), "ismhip_rift")
    return (out, cnt) if want_counts else out


CGF_RADIAL_BINS, CGF_POLAR_BINS, CGF_AZIMUTH_BINS = 17, 11, 12   # cgf.cpp:205-207 as features_cgf.cpp leaves them
CGF_RAW_DIM = CGF_RADIAL_BINS * CGF_POLAR_BINS * CGF_AZIMUTH_BINS  # 2244
CGF_CHUNK_ROWS = 32768                               # keypoints per raw + embedding chunk of cgf(): 294 MB of raw rows


def cgf_radii(radius):
    """the three lengths of features_cgf.cpp:50-52 after their trip through std::to_string ("%f") and stod: (R, rmin, LRF radius) as
    doubles; the normal radius is 0.1 times the first (cgf.cpp:93)"""
    r = float(np.float32(radius))
    return float("%f" % r), float("%f" % (r * 0.05)), float("%f" % (r * 0.75))


def keypoint_normals_pca(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius):
    """ismhip_keypoint_normals_pca -> (nx, ny, nz) [nkp] each: the PCA normal of the `radius` ball about every keypoint, towards (0,0,0)"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    nx, ny, nz = (torch.empty((n,), dtype=torch.float32, device=kpx.device) for _ in range(3))
    ctx.check(lib().ismhip_keypoint_normals_pca(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), _p(nx), _p(ny), _p(nz)),
              "ismhip_keypoint_normals_pca")
    return nx, ny, nz


def cgf_raw(ctx, cloud, kp_offsets, kpx, kpy, kpz, lrf, knx, kny, knz, radius, rmin, want_counts=False):
    """ismhip_cgf_raw -> [nkp, 2244]; radius and rmin as cgf_radii returns them; with want_counts the deposits per keypoint [nkp]"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, CGF_RAW_DIM), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_cgf_raw(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(lrf), _p(knx), _p(kny), _p(knz), C.c_double(radius),
                                   C.c_double(rmin), _p(out), _p(cnt)), "ismhip_cgf_raw")
    return (out, cnt) if want_counts else out


class Mlp:
    """ismhip_mlp: layers = [(W [in, out] float32, b [out] float32, relu), ...] on the host, or from_file(ctx, path) for a .cgfw"""

    def __init__(self, ctx, layers=None, _handle=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            n = len(layers)
            Ws = [np.ascontiguousarray(np.asarray(w, np.float32)) for w, _b, _r in layers]
            bs = [np.ascontiguousarray(np.asarray(b, np.float32)) for _w, b, _r in layers]
            for w, b in zip(Ws, bs):
                if w.ndim != 2 or b.shape != (w.shape[1],):
                    raise IsmHipError("Mlp: W must be [in, out] and b [out]")
            ins = (C.c_int * n)(*[w.shape[0] for w in Ws]); outs = (C.c_int * n)(*[w.shape[1] for w in Ws])
            relu = (C.c_int * n)(*[1 if r else 0 for _w, _b, r in layers])
            wp = (C.c_void_p * n)(*[w.ctypes.data for w in Ws]); bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
            ctx.check(lib().ismhip_mlp_create(ctx._h, C.c_int(n), ins, outs, relu, wp, bp, C.byref(self._h)), "ismhip_mlp_create")
        self.n_in = lib().ismhip_mlp_in(self._h)
        self.n_out = lib().ismhip_mlp_out(self._h)

    @classmethod
    def from_file(cls, ctx, path, expect_in=0):
        w = cgfw_open(path, expect_in)
        try:
            h = C.c_void_p()
            ctx.check(lib().ismhip_mlp_from_cgfw(ctx._h, w, C.byref(h)), "ismhip_mlp_from_cgfw")
        finally:
            lib().ismhip_cgfw_close(w)
        return cls(ctx, _handle=h)

    def forward(self, x, out=None):
        """x [n_rows, in] float32 on the device -> [n_rows, out]"""
        torch = _torch()
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.n_in
        y = torch.empty((x.shape[0], self.n_out), dtype=torch.float32, device=x.device) if out is None else out
        self.ctx.check(lib().ismhip_mlp_forward(self.ctx._h, self._h, _p(x), C.c_size_t(x.shape[0]), _p(y)), "ismhip_mlp_forward")
        return y

    def close(self):
        if self._h:
            lib().ismhip_mlp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cgfw_open(path, expect_in=0):
    """ismhip_cgfw_open -> an opaque handle (close it with lib().ismhip_cgfw_close); raises IsmHipError with the loader's reason"""
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = lib().ismhip_cgfw_open(os.fsencode(path), C.c_int(expect_in), C.byref(h), err, C.c_int(len(err)))
    if rc != 0:
        raise IsmHipError(err.value.decode())
    return h


def cgfw_read(path, expect_in=0):
    """the layers of a .cgfw through the library's loader: [(W [in, out], b [out], relu), ...] as numpy copies"""
    h = cgfw_open(path, expect_in)
    try:
        layers = []
        for l in range(lib().ismhip_cgfw_layers(h)):
            i, o, r = C.c_int(), C.c_int(), C.c_int()
            wp, bp = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
            lib().ismhip_cgfw_layer(h, C.c_int(l), C.byref(i), C.byref(o), C.byref(r), C.byref(wp), C.byref(bp))
            W = np.ctypeslib.as_array(wp, shape=(i.value, o.value)).copy()
            b = np.ctypeslib.as_array(bp, shape=(o.value,)).copy()
            layers.append((W, b, bool(r.value)))
        return layers
    finally:
        lib().ismhip_cgfw_close(h)


def cgfw_write(path, layers):
    """writes [(W [in, out], b [out], relu), ...] as a .cgfw: "CGFW", version 1, the layer count, then per layer in, out, activation,
    W row-major, b -- all little endian (include/ismhip.h)"""
    import struct
    with open(path, "wb") as f:
        f.write(b"CGFW" + struct.pack("<II", 1, len(layers)))
        for W, b, relu in layers:
            W = np.asarray(W, "<f4"); b = np.asarray(b, "<f4")
            if W.ndim != 2 or b.shape != (W.shape[1],):
                raise IsmHipError("cgfw_write: W must be [in, out] and b [out]")
            f.write(struct.pack("<III", W.shape[0], W.shape[1], 1 if relu else 0))
            f.write(np.ascontiguousarray(W).tobytes()); f.write(np.ascontiguousarray(b).tobytes())


def cgf(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius, mlp, chunk_rows=CGF_CHUNK_ROWS, want_counts=False):
    """The CGF rows [nkp, mlp.n_out] of features_cgf.cpp: SHOT frames at 0.75 R, keypoint normals at 0.1 R, raw histograms and the
    embedding. Raw rows exist for chunk_rows keypoints at a time (whole objects are cut where the chunk ends); the result does not depend
    on the chunk size."""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    R, rmin, rl = cgf_radii(radius)
    lrf = shot_lrf(ctx, cloud, ko, kpx, kpy, kpz, rl)
    knx, kny, knz = keypoint_normals_pca(ctx, cloud, ko, kpx, kpy, kpz, 0.1 * R)
    out = torch.empty((n, mlp.n_out), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device)
    step = max(1, int(chunk_rows))
    for b in range(0, n, step):
        e = min(n, b + step)
        sub = (np.clip(ko.astype(np.int64), b, e) - b).astype(np.uint32)      # the keypoints [b, e) of every object
        raw, c = cgf_raw(ctx, cloud, sub, kpx[b:e], kpy[b:e], kpz[b:e], lrf[b:e], knx[b:e], kny[b:e], knz[b:e], R, rmin, want_counts=True)
        mlp.forward(raw, out=out[b:e])
        cnt[b:e] = c
    return (out, cnt) if want_counts else out


GLOBAL_SHORT_SHOT_AUTO_BINS = dict(SHORT_SHOT_AUTO_BINS)
GLOBAL_SHORT_SHOT_AUTO_BINS[64] = (4, 2, 8)       # the one size where the global grid differs from the local one (features_short_shot_global.cpp:197-202)


def global_short_shot_grid(dims=32, bin_type="auto", bins=(1, 1, 8)):
    """FeaturesSHORTSHOTGlobal::configureSphericalGrid (features_short_shot_global.cpp:168-249) -> (dims, (r, e, a)); an unknown size or
    bin type falls back to 32 / (2, 2, 8) as the reference does (with its LOG_ERROR)"""
    if bin_type == "manual":
        r, e, a = (int(b) for b in bins)
        return r * e * a, (r, e, a)
    if bin_type == "auto" and int(dims) in GLOBAL_SHORT_SHOT_AUTO_BINS:
        return int(dims), GLOBAL_SHORT_SHOT_AUTO_BINS[int(dims)]
    return 32, (2, 2, 8)


def _regions(cloud, region_obj, region_center, region_radius, dev):
    """the three region arrays on the device; region_center None / region_radius None: whole objects"""
    torch = _torch()
    obj = torch.as_tensor(np.ascontiguousarray(np.asarray(region_obj, dtype=np.int32)), device=dev)
    n = int(obj.shape[0])
    cen = np.zeros((n, 3), np.float32) if region_center is None else np.ascontiguousarray(np.asarray(region_center, dtype=np.float32)).reshape(n, 3)
    rad = np.full((n,), -1.0, np.float32) if region_radius is None else np.ascontiguousarray(np.asarray(region_radius, dtype=np.float32)).reshape(n)
    return n, obj, torch.as_tensor(cen, device=dev), torch.as_tensor(rad, device=dev)


def _global_outputs(n, dim, dev):
    torch = _torch()
    return dict(n_sel=torch.empty((n,), dtype=torch.int32, device=dev), centroid=torch.empty((n, 3), dtype=torch.float32, device=dev),
                radius=torch.empty((n,), dtype=torch.float32, device=dev), lrf=torch.empty((n, 9), dtype=torch.float32, device=dev),
                desc=torch.empty((n, dim), dtype=torch.float32, device=dev))


def global_short_shot(ctx, cloud, dev, region_obj, region_center=None, region_radius=None, bins=(2, 2, 8), min_radius=0.1, log_radius=False,
                      want_counts=False):
    """ismhip_global_short_shot on regions (object, centre, radius; radius < 0 or None = the whole object) -> dict of device tensors n_sel [n],
    centroid [n, 3], radius [n], lrf [n, 9], desc [n, r * e * a] and, with want_counts, counts [n, r * e * a] (int32)"""
    torch = _torch()
    n, obj, cen, rad = _regions(cloud, region_obj, region_center, region_radius, dev)
    r, e, a = (int(b) for b in bins)
    out = _global_outputs(n, r * e * a if min(r, e, a) > 0 else 0, dev)
    if want_counts:
        out["counts"] = torch.empty_like(out["desc"], dtype=torch.int32)
    ctx.check(lib().ismhip_global_short_shot(ctx._h, cloud._h, C.c_int(n), _p(obj), _p(cen), _p(rad), C.c_double(min_radius),
                                             C.c_int(1 if log_radius else 0), C.c_int(r), C.c_int(e), C.c_int(a), _p(out["n_sel"]),
                                             _p(out["centroid"]), _p(out["radius"]), _p(out["lrf"]), _p(out["desc"]), _p(out.get("counts"))),
              "ismhip_global_short_shot")
    return out


def global_shot352(ctx, cloud, dev, region_obj, region_center=None, region_radius=None):
    """ismhip_global_shot352 on regions as global_short_shot -> dict with desc [n, 352]"""
    n, obj, cen, rad = _regions(cloud, region_obj, region_center, region_radius, dev)
    out = _global_outputs(n, 352, dev)
    ctx.check(lib().ismhip_global_shot352(ctx._h, cloud._h, C.c_int(n), _p(obj), _p(cen), _p(rad), _p(out["n_sel"]), _p(out["centroid"]),
                                          _p(out["radius"]), _p(out["lrf"]), _p(out["desc"])), "ismhip_global_shot352")
    return out


def global_vfh(ctx, cloud, dev, region_obj, region_center=None, region_radius=None, viewpoint=(0.0, 0.0, 0.0), fill_size_component=False,
               want_counts=False):
    """ismhip_global_vfh on regions as global_short_shot -> dict of device tensors n_sel [n], centroid [n, 3], radius [n], normal_centroid
    [n, 3], desc [n, 308] and, with want_counts, counts [n, 308] (int32); there is no frame"""
    torch = _torch()
    n, obj, cen, rad = _regions(cloud, region_obj, region_center, region_radius, dev)
    out = _global_outputs(n, 308, dev)
    del out["lrf"]
    out["normal_centroid"] = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if want_counts:
        out["counts"] = torch.empty_like(out["desc"], dtype=torch.int32)
    vp = (C.c_float * 3)(*[float(v) for v in viewpoint])
    ctx.check(lib().ismhip_global_vfh(ctx._h, cloud._h, C.c_int(n), _p(obj), _p(cen), _p(rad), vp, C.c_int(1 if fill_size_component else 0),
                                      _p(out["n_sel"]), _p(out["centroid"]), _p(out["radius"]), _p(out["normal_centroid"]), _p(out["desc"]),
                                      _p(out.get("counts"))), "ismhip_global_vfh")
    return out


def global_gasd(ctx, cloud, dev, region_obj, region_center=None, region_radius=None, view_direction=(0.0, 0.0, 1.0), with_color=True,
                want_counts=False):
    """ismhip_global_gasd on regions as global_short_shot -> dict of device tensors n_sel [n], centroid [n, 3], radius [n], frame [n, 9] (the
    covariance frame, rows x, y, z), max_coord [n], desc [n, D] and, with want_counts, counts [n, D] (int32); D = 984 with_color
    (the cloud must have been made with rgba), else 512"""
    torch = _torch()
    n, obj, cen, rad = _regions(cloud, region_obj, region_center, region_radius, dev)
    out = _global_outputs(n, 984 if with_color else 512, dev)
    out["frame"] = out.pop("lrf")
    out["max_coord"] = torch.empty((n,), dtype=torch.float32, device=dev)
    if want_counts:
        out["counts"] = torch.empty_like(out["desc"], dtype=torch.int32)
    vd = (C.c_float * 3)(*[float(v) for v in view_direction])
    ctx.check(lib().ismhip_global_gasd(ctx._h, cloud._h, C.c_int(n), _p(obj), _p(cen), _p(rad), vd, C.c_int(1 if with_color else 0),
                                       _p(out["n_sel"]), _p(out["centroid"]), _p(out["radius"]), _p(out["frame"]), _p(out["max_coord"]),
                                       _p(out["desc"]), _p(out.get("counts"))), "ismhip_global_gasd")
    return out


def global_cvfh(ctx, cloud, dev, region_obj, region_center=None, region_radius=None, viewpoint=(0.0, 0.0, 0.0), cluster_tolerance=0.015,
                normal_radius=0.015, min_points=50, angle_threshold=10.0 / 180.0 * np.pi, max_rows=4, want_counts=False, label_stride=0):
    """ismhip_global_cvfh on regions as global_short_shot -> dict of device tensors n_sel [n], centroid [n, 3], radius [n], n_clusters [n]
    (never clipped by max_rows), row_centroid / row_normal [n, max_rows, 3], row_size [n, max_rows], desc [n, max_rows, 308] and, with
    want_counts, counts [n, max_rows, 308] (int32); label_stride = the cloud's largest object asks for labels [n, label_stride] (int64 view
    of the uint32 labels, 0xffffffff for an unselected point)"""
    torch = _torch()
    n, obj, cen, rad = _regions(cloud, region_obj, region_center, region_radius, dev)
    m = int(max_rows)
    out = _global_outputs(n, 1, dev)
    del out["lrf"]
    out["desc"] = torch.empty((n, max(m, 0), 308), dtype=torch.float32, device=dev)
    out["n_clusters"] = torch.empty((n,), dtype=torch.int32, device=dev)
    out["row_centroid"] = torch.empty((n, max(m, 0), 3), dtype=torch.float32, device=dev)
    out["row_normal"] = torch.empty((n, max(m, 0), 3), dtype=torch.float32, device=dev)
    out["row_size"] = torch.empty((n, max(m, 0)), dtype=torch.int32, device=dev)
    if want_counts:
        out["counts"] = torch.empty_like(out["desc"], dtype=torch.int32)
    labels = torch.empty((n, int(label_stride)), dtype=torch.int32, device=dev) if label_stride else None
    vp = (C.c_float * 3)(*[float(v) for v in viewpoint])
    ctx.check(lib().ismhip_global_cvfh(ctx._h, cloud._h, C.c_int(n), _p(obj), _p(cen), _p(rad), vp, C.c_float(cluster_tolerance),
                                       C.c_float(normal_radius), C.c_int(int(min_points)), C.c_double(angle_threshold), C.c_int(m),
                                       _p(out["n_sel"]), _p(out["centroid"]), _p(out["radius"]), _p(out["n_clusters"]), _p(out["row_centroid"]),
                                       _p(out["row_normal"]), _p(out["row_size"]), _p(out["desc"]), _p(out.get("counts")), _p(labels)),
              "ismhip_global_cvfh")
    if labels is not None:
        out["labels"] = labels.to(torch.int64) & 0xffffffff
    return out


MVBB_ROUNDS, MVBB_TRACE = 10, 48   # ISMHIP_MVBB_ROUNDS, ISMHIP_MVBB_TRACE


def region_mvbb(ctx, cloud, dev, region_obj, region_center=None, region_radius=None, want_volume=True, want_trace=True):
    """ismhip_region_mvbb on regions as global_short_shot -> dict of device tensors n_sel [n], center [n, 3] (world), size [n, 3]
    (descending), axes [n, 9] (rows = axes) and, unless switched off, volume [n] (float64) and trace [n, 48] (int32)"""
    torch = _torch()
    n, obj, cen, rad = _regions(cloud, region_obj, region_center, region_radius, dev)
    out = dict(n_sel=torch.empty((n,), dtype=torch.int32, device=dev), center=torch.empty((n, 3), dtype=torch.float32, device=dev),
               size=torch.empty((n, 3), dtype=torch.float32, device=dev), axes=torch.empty((n, 9), dtype=torch.float32, device=dev))
    if want_volume:
        out["volume"] = torch.empty((n,), dtype=torch.float64, device=dev)
    if want_trace:
        out["trace"] = torch.empty((n, MVBB_TRACE), dtype=torch.int32, device=dev)
    ctx.check(lib().ismhip_region_mvbb(ctx._h, cloud._h, C.c_int(n), _p(obj), _p(cen), _p(rad), _p(out["n_sel"]), _p(out["center"]),
                                       _p(out["size"]), _p(out["axes"]), _p(out.get("volume")), _p(out.get("trace"))), "ismhip_region_mvbb")
    return out


def gasd_hue_bins(ctx, rgba):
    """ismhip_gasd_hue_bins (diagnostic): the hue bin 0..11 of ismhip_global_gasd's colour block for the packed colours rgba (int32 device
    tensor [n]) -> uint8 [n] on the same device, 255 where the rule deposits nothing"""
    torch = _torch()
    assert rgba.dim() == 1 and rgba.dtype == torch.int32
    out = torch.empty((rgba.shape[0],), dtype=torch.uint8, device=rgba.device)
    ctx.check(lib().ismhip_gasd_hue_bins(ctx._h, C.c_int(rgba.shape[0]), _p(rgba), _p(out)), "ismhip_gasd_hue_bins")
    return out


def fpfh33(ctx, cloud, kp_offsets, kpx, kpy, kpz, radius, want_counts=False):
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    out = torch.empty((n, 33), dtype=torch.float32, device=kpx.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=kpx.device) if want_counts else None
    ctx.check(lib().ismhip_fpfh33(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), C.c_float(radius), _p(out), _p(cnt)),
              "ismhip_fpfh33")
    return (out, cnt) if want_counts else out


def cloud_centroids(ctx, cloud, device):
    torch = _torch()
    out = torch.empty((cloud.n_obj, 3), dtype=torch.float32, device=device)
    ctx.check(lib().ismhip_cloud_centroids(ctx._h, cloud._h, _p(out)), "ismhip_cloud_centroids")
    return out


def cloud_radii(ctx, cloud, centroid):
    """SingleObjectHelper::getModelRadius per object: farthest point from centroid [n_obj, 3] (device)"""
    torch = _torch()
    out = torch.empty((cloud.n_obj,), dtype=torch.float32, device=centroid.device)
    ctx.check(lib().ismhip_cloud_radii(ctx._h, cloud._h, _p(centroid), _p(out)), "ismhip_cloud_radii")
    return out


def center_dist(ctx, cloud, kp_offsets, kpx, kpy, kpz):
    torch = _torch()
    ko = _u32(kp_offsets)
    out = torch.empty((int(ko[-1]),), dtype=torch.float32, device=kpx.device)
    ctx.check(lib().ismhip_center_dist(ctx._h, cloud._h, _p(ko), _p(kpx), _p(kpy), _p(kpz), _p(out)), "ismhip_center_dist")
    return out


def estimate_normals(ctx, cloud, radius, nx, ny, nz):
    """ImplicitShapeModel::computeNormals (method 2): fills nx, ny, nz (device tensors, original order) and the cloud's own copies"""
    ctx.check(lib().ismhip_estimate_normals(ctx._h, cloud._h, C.c_float(radius), _p(nx), _p(ny), _p(nz)), "ismhip_estimate_normals")
    cloud._keep = getattr(cloud, "_keep", ()) + (nx, ny, nz)
    return nx, ny, nz


def estimate_normals_pca(ctx, cloud, radius, orientation, nx, ny, nz):
    """ConsistentNormalsMethod 0 (orientation 0: towards the origin) / 1 (orientation 1: away from the object's centroid)"""
    ctx.check(lib().ismhip_estimate_normals_pca(ctx._h, cloud._h, C.c_float(radius), C.c_int(orientation), _p(nx), _p(ny), _p(nz)), "ismhip_estimate_normals_pca")
    cloud._keep = getattr(cloud, "_keep", ()) + (nx, ny, nz)
    return nx, ny, nz


class _PointArrays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "y", "z", "nx", "ny", "nz", "rgba")]


def _compact_point_arrays(ctx, symbol, pt_offsets, arrays, rgba, *mask):
    """ismhip_filter_normals / ismhip_compact_points (which takes its keep mask between the two array sets) on x, y, z, nx, ny, nz and
    rgba or None: returns (new_offsets numpy, x, y, z, nx, ny, nz, rgba or None)"""
    torch = _torch()
    po = _u32(pt_offsets)
    n_obj = len(po) - 1
    ins = list(arrays) + ([rgba] if rgba is not None else [])
    outs = [torch.empty_like(t) for t in ins]
    a_in = _PointArrays(*[t.data_ptr() for t in ins], *([None] if rgba is None else []))
    a_out = _PointArrays(*[t.data_ptr() for t in outs], *([None] if rgba is None else []))
    new = np.zeros(n_obj + 1, dtype=np.uint32)
    ctx.check(getattr(lib(), symbol)(ctx._h, C.c_int(n_obj), _p(po), C.byref(a_in), *[_p(m) for m in mask], C.byref(a_out), _p(new)), symbol)
    m = int(new[-1])
    outs = [t[:m] for t in outs]
    return (new, *outs, *([None] if rgba is None else []))


def filter_normals(ctx, pt_offsets, x, y, z, nx, ny, nz, rgba=None):
    """ImplicitShapeModel::filterNormals on the device: returns (new_offsets numpy, x, y, z, nx, ny, nz, rgba or None) without the
    points whose normal holds a NaN (order kept)"""
    return _compact_point_arrays(ctx, "ismhip_filter_normals", pt_offsets, (x, y, z, nx, ny, nz), rgba)


def filter_statistical(ctx, cloud, mean_k=20, stddev_mul=2.0, want_mean_dist=True):
    """pcl::StatisticalOutlierRemoval on the device: returns (keep uint8[n_pts], mean_dist float32[n_pts] or None, thresholds float64[n_obj])"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    md = torch.empty((n,), dtype=torch.float32, device=dev) if want_mean_dist else None
    thr = np.zeros(cloud.n_obj, dtype=np.float64)
    ctx.check(lib().ismhip_filter_statistical(ctx._h, cloud._h, C.c_int(mean_k), C.c_float(stddev_mul), _p(keep), _p(md), _p(thr)),
              "ismhip_filter_statistical")
    return keep, md, thr


def filter_radius(ctx, cloud, radius, min_neighbors, want_counts=False):
    """pcl::RadiusOutlierRemoval on the device: returns (keep uint8[n_pts], counts int32[n_pts] or None)"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev) if want_counts else None
    ctx.check(lib().ismhip_filter_radius(ctx._h, cloud._h, C.c_float(radius), C.c_int(min_neighbors), _p(keep), _p(cnt)), "ismhip_filter_radius")
    return keep, cnt


def filter_passthrough_z(ctx, x, y, z, z_min, z_max):
    """pcl::PassThrough on z: keep uint8[n_pts], 1 where the point is finite and z_min <= z <= z_max"""
    torch = _torch()
    keep = torch.zeros((x.numel(),), dtype=torch.uint8, device=x.device)
    ctx.check(lib().ismhip_filter_passthrough_z(ctx._h, C.c_uint32(x.numel()), _p(x), _p(y), _p(z), C.c_float(z_min), C.c_float(z_max), _p(keep)),
              "ismhip_filter_passthrough_z")
    return keep


def compact_points(ctx, pt_offsets, keep, x, y, z, nx, ny, nz, rgba=None):
    """the points with keep == 1, order kept: returns (new_offsets numpy, x, y, z, nx, ny, nz, rgba or None)"""
    return _compact_point_arrays(ctx, "ismhip_compact_points", pt_offsets, (x, y, z, nx, ny, nz), rgba, keep)


def voxel_keypoints(ctx, pt_offsets, x, y, z, leaf, rgba=None):
    """KeypointsVoxelGrid on the device: returns (kp_offsets[n_obj+1] numpy, kx, ky, kz, krgba or None) packed object after object"""
    torch = _torch()
    po = _u32(pt_offsets)
    n_obj = len(po) - 1
    n = int(po[-1])
    kx = torch.empty((n,), dtype=torch.float32, device=x.device); ky = torch.empty_like(kx); kz = torch.empty_like(kx)
    kc = torch.empty((n,), dtype=torch.int32, device=x.device) if rgba is not None else None
    ko = np.zeros(n_obj + 1, dtype=np.uint32)
    ctx.check(lib().ismhip_voxel_keypoints(ctx._h, C.c_int(n_obj), _p(po), _p(x), _p(y), _p(z), _p(rgba), C.c_float(leaf), C.c_uint32(n),
                                           _p(kx), _p(ky), _p(kz), _p(kc), _p(ko)), "ismhip_voxel_keypoints")
    m = int(ko[-1])
    return ko, kx[:m], ky[:m], kz[:m], (kc[:m] if kc is not None else None)


def iss3d_saliency(ctx, cloud, salient_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5, want_eig=True, want_counts=True):
    """ismhip_iss3d_saliency: returns (saliency float64[n_pts], eig float64[n_pts, 3] (e1 >= e2 >= e3) or None, counts int32[n_pts] or None)
    in the cloud's original point order"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    sal = torch.zeros((n,), dtype=torch.float64, device=dev)
    eig = torch.zeros((n, 3), dtype=torch.float64, device=dev) if want_eig else None
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev) if want_counts else None
    ctx.check(lib().ismhip_iss3d_saliency(ctx._h, cloud._h, C.c_float(salient_radius), C.c_double(gamma21), C.c_double(gamma32), C.c_int(min_neighbors),
                                          _p(sal), _p(eig), _p(cnt)), "ismhip_iss3d_saliency")
    return sal, eig, cnt


def iss3d_keypoints(ctx, cloud, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5, capacity=None):
    """KeypointsISS3D on the device: returns (kp_offsets[n_obj+1] numpy, kx, ky, kz, krgba or None, src int32: the point's index inside its
    object) packed object after object. capacity: entries of the output arrays (default: the number of points, which always suffices)"""
    torch = _torch()
    x, rgba = cloud._keep[0], cloud._keep[6]
    n = int(cloud.pt_offsets[-1])
    cap = n if capacity is None else int(capacity)
    kx = torch.empty((max(cap, 1),), dtype=torch.float32, device=x.device); ky = torch.empty_like(kx); kz = torch.empty_like(kx)
    kc = torch.empty((max(cap, 1),), dtype=torch.int32, device=x.device) if rgba is not None else None
    src = torch.empty((max(cap, 1),), dtype=torch.int32, device=x.device)
    ko = np.zeros(cloud.n_obj + 1, dtype=np.uint32)
    ctx.check(lib().ismhip_iss3d_keypoints(ctx._h, cloud._h, C.c_float(salient_radius), C.c_float(non_max_radius), C.c_double(gamma21), C.c_double(gamma32),
                                           C.c_int(min_neighbors), C.c_uint32(cap), _p(kx), _p(ky), _p(kz), _p(kc), _p(src), _p(ko)), "ismhip_iss3d_keypoints")
    m = int(ko[-1])
    return ko, kx[:m], ky[:m], kz[:m], (kc[:m] if kc is not None else None), src[:m]


def principal_curvatures(ctx, cloud, radius, want_counts=True):
    """ismhip_principal_curvatures: returns (pc1 float32[n_pts], pc2 float32[n_pts], counts int32[n_pts] or None) in the cloud's original
    point order; NaN, NaN, 0 where the position or the point's own normal is not finite"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    pc1 = torch.zeros((n,), dtype=torch.float32, device=dev); pc2 = torch.zeros_like(pc1)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev) if want_counts else None
    ctx.check(lib().ismhip_principal_curvatures(ctx._h, cloud._h, C.c_float(radius), _p(pc1), _p(pc2), _p(cnt)), "ismhip_principal_curvatures")
    return pc1, pc2, cnt


def _culling_code(table, value, what):
    key = value if what == "CombineFilters" else str(value).lower()       # method and type strings are lower-cased, CombineFilters is not
    if key not in table:
        raise ValueError(f"VoxelGridCulling {what} {value!r} (one of {sorted(table)})")
    return table[key]


def culling_scores(ctx, cloud, kp_offsets, kx, ky, kz, krgba, leaf, geometry="none", color="none", max_similar_color_distance=0.01, pc1=None, pc2=None,
                   want_counts=True):
    """ismhip_culling_scores: returns (geo float32[n_kp], color float32[n_kp], counts int32[n_kp] or None); a method "none" leaves zeros.
    geometry "kpq" takes pc1, pc2 of principal_curvatures"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n = int(ko[-1])
    dev = cloud._keep[0].device
    geo = torch.zeros((n,), dtype=torch.float32, device=dev); col = torch.zeros_like(geo)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev) if want_counts else None
    ctx.check(lib().ismhip_culling_scores(ctx._h, cloud._h, _p(ko), _p(kx), _p(ky), _p(kz), _p(krgba), C.c_float(leaf),
                                          C.c_int(_culling_code(CULLING_GEOMETRY, geometry, "FilterMethodGeometry")),
                                          C.c_int(_culling_code(CULLING_COLOR, color, "FilterMethodColor")), C.c_float(max_similar_color_distance),
                                          _p(pc1), _p(pc2), _p(geo), _p(col), _p(cnt)), "ismhip_culling_scores")
    return geo, col, cnt


def culling_select(ctx, kp_offsets, geo, color, kx, ky, kz, krgba=None, geometry_on=True, color_on=True, geometry_type="cutoff", color_type="cutoff",
                   geometry_threshold=0.005, color_threshold=0.02, cutoff_ratio=0.5, combine="RequireCombinedList", capacity=None):
    """ismhip_culling_select: returns a dict with kp_offsets (numpy [n_obj+1]), kx, ky, kz, krgba (or None): the accepted keypoints in their
    order; keep uint8[n_kp], combined float32[n_kp], thresholds float32[n_obj, 3] (geometry, colour, combined)"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n_obj, n = len(ko) - 1, int(ko[-1])
    dev = geo.device
    cap = n if capacity is None else int(capacity)
    ox = torch.empty((max(cap, 1),), dtype=torch.float32, device=dev); oy = torch.empty_like(ox); oz = torch.empty_like(ox)
    oc = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev) if krgba is not None else None
    keep = torch.zeros((max(n, 1),), dtype=torch.uint8, device=dev)
    comb = torch.zeros((max(n, 1),), dtype=torch.float32, device=dev)
    thr = torch.zeros((n_obj, 3), dtype=torch.float32, device=dev)
    out = np.zeros(n_obj + 1, dtype=np.uint32)
    ctx.check(lib().ismhip_culling_select(ctx._h, C.c_int(n_obj), _p(ko), _p(geo), _p(color), C.c_int(1 if geometry_on else 0), C.c_int(1 if color_on else 0),
                                          C.c_int(_culling_code(CULLING_TYPE, geometry_type, "FilterTypeGeometry")),
                                          C.c_int(_culling_code(CULLING_TYPE, color_type, "FilterTypeColor")), C.c_float(geometry_threshold),
                                          C.c_float(color_threshold), C.c_float(cutoff_ratio), C.c_int(_culling_code(CULLING_COMBINE, combine, "CombineFilters")),
                                          _p(kx), _p(ky), _p(kz), _p(krgba), C.c_uint32(cap), _p(ox), _p(oy), _p(oz), _p(oc), _p(keep), _p(comb), _p(thr),
                                          _p(out)), "ismhip_culling_select")
    m = int(out[-1])
    return dict(kp_offsets=out, kx=ox[:m], ky=oy[:m], kz=oz[:m], krgba=(oc[:m] if oc is not None else None), keep=keep[:n], combined=comb[:n],
                thresholds=thr)


def voxel_culling_keypoints(ctx, cloud, leaf, geometry="none", color="none", geometry_type="cutoff", color_type="cutoff", geometry_threshold=0.005,
                            color_threshold=0.02, max_similar_color_distance=0.01, cutoff_ratio=0.5, combine="RequireCombinedList",
                            disable_filter_in_training=True, is_training=False):
    """KeypointsVoxelGridCulling on the device, on the points the cloud was created with: the voxel keypoints at `leaf`, their scores and the
    selection; returns (kp_offsets[n_obj+1] numpy, kx, ky, kz, krgba or None). Both methods "none", or training with
    disable_filter_in_training: the plain voxel grid"""
    x, y, z, rgba = cloud._keep[0], cloud._keep[1], cloud._keep[2], cloud._keep[6]
    ko, kx, ky, kz, kc = voxel_keypoints(ctx, cloud.pt_offsets, x, y, z, leaf, rgba=rgba)
    g, c = str(geometry).lower(), str(color).lower()
    _culling_code(CULLING_GEOMETRY, g, "FilterMethodGeometry"); _culling_code(CULLING_COLOR, c, "FilterMethodColor")
    if (is_training and disable_filter_in_training) or (g == "none" and c == "none"):
        return ko, kx, ky, kz, kc
    pc1 = pc2 = None
    if g == "kpq":
        pc1, pc2, _ = principal_curvatures(ctx, cloud, leaf, want_counts=False)
    geo, col, _ = culling_scores(ctx, cloud, ko, kx, ky, kz, kc, leaf, g, c, max_similar_color_distance, pc1, pc2, want_counts=False)
    r = culling_select(ctx, ko, geo, col, kx, ky, kz, kc, g != "none", c != "none", geometry_type, color_type, geometry_threshold, color_threshold,
                       cutoff_ratio, combine)
    return r["kp_offsets"], r["kx"], r["ky"], r["kz"], r["krgba"]


def normal_curvature(ctx, cloud, radius, want_counts=True):
    """ismhip_normal_curvature: returns (curvature float32[n_pts], counts int32[n_pts] or None) in the cloud's original point order; NaN
    where the point is not finite or its ball holds fewer than 3 points"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    curv = torch.zeros((n,), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev) if want_counts else None
    ctx.check(lib().ismhip_normal_curvature(ctx._h, cloud._h, C.c_float(radius), _p(curv), _p(cnt)), "ismhip_normal_curvature")
    return curv, cnt


def voxel_downsample_xyzi(ctx, pt_offsets, x, y, z, intensity, leaf):
    """ismhip_voxel_downsample_xyzi: returns (offsets[n_obj+1] numpy, kx, ky, kz, ki) packed object after object"""
    torch = _torch()
    po = _u32(pt_offsets)
    n_obj = len(po) - 1
    n = int(po[-1])
    kx = torch.empty((max(n, 1),), dtype=torch.float32, device=x.device); ky = torch.empty_like(kx); kz = torch.empty_like(kx); ki = torch.empty_like(kx)
    ko = np.zeros(n_obj + 1, dtype=np.uint32)
    ctx.check(lib().ismhip_voxel_downsample_xyzi(ctx._h, C.c_int(n_obj), _p(po), _p(x), _p(y), _p(z), _p(intensity), C.c_float(leaf), C.c_uint32(n),
                                                 _p(kx), _p(ky), _p(kz), _p(ki), _p(ko)), "ismhip_voxel_downsample_xyzi")
    m = int(ko[-1])
    return ko, kx[:m], ky[:m], kz[:m], ki[:m]


def sift3d_scales(base_scale, nr_scales):
    """scales[i] = base_scale * powf(2.0f, (i - 1.0f) / nr_scales), i = 0 .. nr_scales + 2, every step in float and with the C library's
    powf, as ismhip_sift3d_keypoints takes them"""
    import ctypes.util
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.powf.restype = C.c_float
    libm.powf.argtypes = [C.c_float, C.c_float]
    f = np.float32
    return np.array([f(base_scale) * f(libm.powf(2.0, f(f(i) - f(1.0)) / f(nr_scales))) for i in range(nr_scales + 3)], dtype=np.float32)


def sift3d_scale_space(ctx, cloud, intensity, scales, want_counts=True):
    """ismhip_sift3d_scale_space: returns (dog float32[n_pts, len(scales) - 1], counts int32[n_pts] or None), original point order"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    sc = np.ascontiguousarray(np.asarray(scales, dtype=np.float32))
    dog = torch.zeros((n, max(len(sc) - 1, 1)), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev) if want_counts else None
    ctx.check(lib().ismhip_sift3d_scale_space(ctx._h, cloud._h, _p(intensity), _p(sc), C.c_int(len(sc)), _p(dog), _p(cnt)), "ismhip_sift3d_scale_space")
    return dog, cnt


def sift3d_extrema(ctx, cloud, dog, k=SIFT3D_MIN_POINTS, min_contrast=0.0, want_nn=True):
    """ismhip_sift3d_extrema: returns (flags uint8[n_pts, n_cols]: 0 none, 1 minimum, 2 maximum; nn int32[n_pts, k] padded with -1, or None)"""
    torch = _torch()
    n, n_cols = dog.shape
    flags = torch.zeros((n, n_cols), dtype=torch.uint8, device=dog.device)
    nn = torch.full((n, max(k, 1)), -1, dtype=torch.int32, device=dog.device) if want_nn else None
    ctx.check(lib().ismhip_sift3d_extrema(ctx._h, cloud._h, _p(dog), C.c_int(n_cols), C.c_int(k), C.c_float(min_contrast), _p(flags), _p(nn)),
              "ismhip_sift3d_extrema")
    return flags, nn


def sift3d_keypoints(ctx, cloud, intensity, min_scale, nr_octaves=4, nr_scales=3, min_contrast=0.0, capacity=None):
    """KeypointsSIFT3D on the device: returns (kp_offsets[n_obj+1] numpy, kx, ky, kz, kscale, octave_sizes uint32[n_obj, nr_octaves]).
    capacity: entries of the output arrays (default: 4 * nr_scales per point; the count is not bounded by the number of points)"""
    torch = _torch()
    dev = cloud._keep[0].device
    n = int(cloud.pt_offsets[-1])
    cap = n * 4 * nr_scales if capacity is None else int(capacity)
    kx = torch.zeros((max(cap, 1),), dtype=torch.float32, device=dev); ky = torch.zeros_like(kx); kz = torch.zeros_like(kx); ks = torch.zeros_like(kx)
    ko = np.zeros(cloud.n_obj + 1, dtype=np.uint32)
    sizes = np.zeros((cloud.n_obj, max(nr_octaves, 1)), dtype=np.uint32)
    ctx.check(lib().ismhip_sift3d_keypoints(ctx._h, cloud._h, _p(intensity), C.c_float(min_scale), C.c_int(nr_octaves), C.c_int(nr_scales),
                                            C.c_float(min_contrast), C.c_uint32(cap), _p(kx), _p(ky), _p(kz), _p(ks), _p(ko), _p(sizes)),
              "ismhip_sift3d_keypoints")
    m = int(ko[-1])
    return ko, kx[:m], ky[:m], kz[:m], ks[:m], sizes


def _compact_feature_rows(ctx, symbol, report_all_kept, kp_offsets, desc, lrf, kpx, kpy, kpz):
    """ismhip_compact_features / ismhip_compact_descriptor_rows (which reports "nothing dropped": the inputs are then returned)"""
    torch = _torch()
    ko = _u32(kp_offsets)
    n_obj = len(ko) - 1
    n, dim = desc.shape
    d_o = torch.empty_like(desc)
    l_o = torch.empty_like(lrf) if lrf is not None else None
    x_o, y_o, z_o = torch.empty_like(kpx), torch.empty_like(kpy), torch.empty_like(kpz)
    src = torch.empty((n,), dtype=torch.int32, device=desc.device)
    keep = np.zeros(n_obj + 1, dtype=np.uint32)
    all_kept = C.c_int(0)
    ctx.check(getattr(lib(), symbol)(ctx._h, C.c_int(n_obj), _p(ko), C.c_int(dim), _p(desc), _p(lrf), _p(kpx), _p(kpy), _p(kpz),
                                     _p(d_o), _p(l_o), _p(x_o), _p(y_o), _p(z_o), _p(src), _p(keep), *([C.byref(all_kept)] if report_all_kept else [])),
              symbol)
    if all_kept.value:
        return keep, desc, lrf, kpx, kpy, kpz, src
    m = int(keep[-1])
    return keep, d_o[:m], (l_o[:m] if l_o is not None else None), x_o[:m], y_o[:m], z_o[:m], src[:m]


def compact_descriptor_rows(ctx, kp_offsets, desc, lrf, kpx, kpy, kpz):
    """compact_features for descriptor matrices of this library (rows are NaN as a whole): when nothing is dropped the INPUT tensors are
    returned, no copy is made"""
    return _compact_feature_rows(ctx, "ismhip_compact_descriptor_rows", True, kp_offsets, desc, lrf, kpx, kpy, kpz)


def compact_features(ctx, kp_offsets, desc, lrf, kpx, kpy, kpz):
    """returns (keep_offsets, desc, lrf, kpx, kpy, kpz, src_index) with NaN rows removed (order preserved)"""
    return _compact_feature_rows(ctx, "ismhip_compact_features", False, kp_offsets, desc, lrf, kpx, kpy, kpz)


def _knn_outputs(q, k):
    """(nq, idx [nq, k] int32, dist [nq, k] float32) for the queries q"""
    torch = _torch()
    nq = q.shape[0]
    return nq, torch.empty((nq, k), dtype=torch.int32, device=q.device), torch.empty((nq, k), dtype=torch.float32, device=q.device)


def knn(ctx, cb, metric, q, k=1):
    nq, idx, dist = _knn_outputs(q, k)
    ctx.check(lib().ismhip_knn(ctx._h, cb._h, C.c_int(metric), C.c_int(nq), _p(q), C.c_int(k), _p(idx), _p(dist)), "ismhip_knn")
    return idx, dist


def knn_binary(ctx, cb, q, k=1):
    """ismhip_knn_binary: knn for rows of zeros and ones on a codebook with a binary image (Codebook.make_binary), either metric; synchronises"""
    nq, idx, dist = _knn_outputs(q, k)
    ctx.check(lib().ismhip_knn_binary(ctx._h, cb._h, C.c_int(nq), _p(q), C.c_int(k), _p(idx), _p(dist)), "ismhip_knn_binary")
    return idx, dist


def knn_large_k(ctx, cb, metric, q, k):
    """ismhip_knn_large_k: the contract of knn for any 1 <= k <= 1024 (k <= 16 is knn itself); synchronises"""
    nq, idx, dist = _knn_outputs(q, k)
    ctx.check(lib().ismhip_knn_large_k(ctx._h, cb._h, C.c_int(metric), C.c_int(nq), _p(q), C.c_int(k), _p(idx), _p(dist)), "ismhip_knn_large_k")
    return idx, dist


def knn_ratio(ctx, cb, metric, q, ratio_threshold):
    nq, idx, dist = _knn_outputs(q, 1)
    ctx.check(lib().ismhip_knn_ratio(ctx._h, cb._h, C.c_int(metric), C.c_int(nq), _p(q), C.c_float(ratio_threshold), _p(idx), _p(dist)),
              "ismhip_knn_ratio")
    return idx, dist


def knn_rule(ctx, cb, metric, q, ratio_threshold):
    nq, idx, dist = _knn_outputs(q, 1)
    ctx.check(lib().ismhip_knn_rule(ctx._h, cb._h, C.c_int(metric), C.c_int(nq), _p(q), C.c_float(ratio_threshold), _p(idx), _p(dist)),
              "ismhip_knn_rule")
    return idx, dist


def _act_offsets(act_offsets, dev):
    """activation offsets as the device int32 tensor the C ABI takes: a host array is converted and uploaded"""
    if isinstance(act_offsets, np.ndarray):
        return _torch().from_numpy(np.ascontiguousarray(act_offsets.astype(np.uint32)).view(np.int32)).to(dev)
    return act_offsets


def _vote_outputs(ns, dev, want_bbox):
    """the output tensors of cast_votes / cast_votes_csr for ns vote slots, in the order of the C arguments"""
    torch = _torch()
    return dict(pos=torch.empty((ns, 3), dtype=torch.float32, device=dev), weight=torch.empty((ns,), dtype=torch.float32, device=dev),
                cls=torch.empty((ns,), dtype=torch.int32, device=dev), inst=torch.empty((ns,), dtype=torch.int32, device=dev),
                codeword=torch.empty((ns,), dtype=torch.int32, device=dev),
                bbox_quat=torch.empty((ns, 4), dtype=torch.float32, device=dev) if want_bbox else None,
                bbox_size=torch.empty((ns, 3), dtype=torch.float32, device=dev) if want_bbox else None)


def _vote_keypoint_outputs(ns, dev):
    """(keypoint, keypoint_training) [ns, 3] of vote_keypoints / vote_keypoints_csr; zero where a slot holds no vote"""
    torch = _torch()
    return torch.zeros((ns, 3), dtype=torch.float32, device=dev), torch.zeros((ns, 3), dtype=torch.float32, device=dev)


def cast_votes(ctx, cb, weight_flags, lrf, kpx, kpy, kpz, idx, dist, want_bbox=False):
    nq, k = idx.shape
    out = _vote_outputs(nq * k * max(cb.max_votes, 0), idx.device, want_bbox)
    ctx.check(lib().ismhip_cast_votes(ctx._h, cb._h, C.c_uint32(weight_flags), C.c_int(nq), _p(lrf), _p(kpx), _p(kpy), _p(kpz), C.c_int(k),
                                      _p(idx), _p(dist), *[_p(t) for t in out.values()]), "ismhip_cast_votes")
    return out


def knn_threshold(ctx, cb, metric, q, threshold, capacity=None):
    """ActivationStrategyThreshold: every codeword with functor value < threshold, ascending row order, as a CSR ->
    (act_offsets [nq+1] int64 host, idx [n_act] int32 device, dist [n_act] float32 device). capacity=None: count first, then fetch
    the lists with a buffer of exactly the total; otherwise one call with that capacity (lists None when the total does not fit)."""
    torch = _torch()
    nq = q.shape[0]
    off = torch.empty((nq + 1,), dtype=torch.int32, device=q.device)
    n_act = C.c_int64(0)
    cap = 0 if capacity is None else int(capacity)
    idx = torch.empty((max(cap, 1),), dtype=torch.int32, device=q.device)
    dist = torch.empty((max(cap, 1),), dtype=torch.float32, device=q.device)

    def call():
        ctx.check(lib().ismhip_knn_threshold(ctx._h, cb._h, C.c_int(metric), C.c_int(nq), _p(q), C.c_float(threshold), C.c_int64(cap),
                                             _p(off), _p(idx), _p(dist), C.byref(n_act)), "ismhip_knn_threshold")
    call()
    total = n_act.value
    if capacity is None and total > 0:
        cap = total
        idx = torch.empty((cap,), dtype=torch.int32, device=q.device)
        dist = torch.empty((cap,), dtype=torch.float32, device=q.device)
        call()
    offsets = off.cpu().numpy().view(np.uint32).astype(np.int64)
    if total > cap:
        return offsets, None, None
    return offsets, idx[:total], dist[:total]


def cast_votes_csr(ctx, cb, weight_flags, lrf, kpx, kpy, kpz, act_offsets, idx, dist, want_bbox=False):
    """ismhip_cast_votes_csr: act_offsets [nq+1] (host array or device int32 tensor), idx / dist [n_act] device. Slot of (activation a,
    stored vote v) = a * max_votes + v."""
    act_offsets = _act_offsets(act_offsets, idx.device)
    nq = act_offsets.shape[0] - 1
    n_act = idx.shape[0]
    out = _vote_outputs(n_act * max(cb.max_votes, 0), idx.device, want_bbox)
    ctx.check(lib().ismhip_cast_votes_csr(ctx._h, cb._h, C.c_uint32(weight_flags), C.c_int(nq), _p(lrf), _p(kpx), _p(kpy), _p(kpz), _p(act_offsets),
                                          C.c_int64(n_act), _p(idx), _p(dist), *[_p(t) for t in out.values()]), "ismhip_cast_votes_csr")
    return out


def vote_keypoints(ctx, cb, kpx, kpy, kpz, idx):
    """ismhip_vote_keypoints: (keypoint, keypoint_training) [n_slots, 3] of every vote slot of cast_votes(idx [nq, k])"""
    nq, k = idx.shape
    kp, kpt = _vote_keypoint_outputs(nq * k * max(cb.max_votes, 0), idx.device)
    ctx.check(lib().ismhip_vote_keypoints(ctx._h, cb._h, C.c_int(nq), _p(kpx), _p(kpy), _p(kpz), C.c_int(k), _p(idx), _p(kp), _p(kpt)), "ismhip_vote_keypoints")
    return kp, kpt


def vote_keypoints_csr(ctx, cb, kpx, kpy, kpz, act_offsets, idx):
    """ismhip_vote_keypoints_csr: the same in the slot layout of cast_votes_csr"""
    act_offsets = _act_offsets(act_offsets, idx.device)
    nq = act_offsets.shape[0] - 1
    n_act = idx.shape[0]
    kp, kpt = _vote_keypoint_outputs(n_act * max(cb.max_votes, 0), idx.device)
    ctx.check(lib().ismhip_vote_keypoints_csr(ctx._h, cb._h, C.c_int(nq), _p(kpx), _p(kpy), _p(kpz), _p(act_offsets), C.c_int64(n_act), _p(idx), _p(kp), _p(kpt)),
              "ismhip_vote_keypoints_csr")
    return kp, kpt


def ransac_filter(ctx, cluster_offsets, src_xyz, tgt_xyz, threshold, max_iterations=RANSAC_MAX_ITERATIONS, seed=RANSAC_SEED, want_transform=True):
    """ismhip_ransac_filter over a CSR of clusters: src_xyz / tgt_xyz device [n, 3] (training / scene keypoints), threshold a scalar or
    one value per cluster -> dict(inlier [n] uint8, kept, n_inliers, best_hypothesis, iterations [n_clusters] int32, transform
    [n_clusters, 4, 4]) of device tensors"""
    torch = _torch()
    off = _u32(cluster_offsets)
    nc = len(off) - 1
    n = int(off[-1])
    dev = src_xyz.device
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(threshold, dtype=np.float32), (nc,)))
    out = dict(inlier=torch.zeros((n,), dtype=torch.uint8, device=dev), kept=torch.zeros((nc,), dtype=torch.int32, device=dev),
               n_inliers=torch.zeros((nc,), dtype=torch.int32, device=dev), best_hypothesis=torch.zeros((nc,), dtype=torch.int32, device=dev),
               iterations=torch.zeros((nc,), dtype=torch.int32, device=dev),
               transform=torch.zeros((nc, 4, 4), dtype=torch.float32, device=dev) if want_transform else None)
    ctx.check(lib().ismhip_ransac_filter(ctx._h, C.c_int(nc), _p(off), _p(src_xyz), _p(tgt_xyz), _p(thr), C.c_int(max_iterations), C.c_ulonglong(seed),
                                         _p(out["inlier"]), _p(out["kept"]), _p(out["n_inliers"]), _p(out["best_hypothesis"]), _p(out["iterations"]),
                                         _p(out["transform"])), "ismhip_ransac_filter")
    return out


def ransac_hypothesis(ctx, cluster_offsets, src_xyz, tgt_xyz, threshold, hypothesis, seed=RANSAC_SEED):
    """ismhip_ransac_hypothesis (diagnostic): hypothesis[c] of every cluster -> dict(inlier, valid, n_inliers, d2 [n] float64,
    transform [n_clusters, 12] float64 = R row-major, then t)"""
    torch = _torch()
    off = _u32(cluster_offsets)
    nc = len(off) - 1
    n = int(off[-1])
    dev = src_xyz.device
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(threshold, dtype=np.float32), (nc,)))
    hyp = np.ascontiguousarray(np.broadcast_to(np.asarray(hypothesis, dtype=np.int32), (nc,)))
    out = dict(inlier=torch.zeros((n,), dtype=torch.uint8, device=dev), valid=torch.zeros((nc,), dtype=torch.int32, device=dev),
               n_inliers=torch.zeros((nc,), dtype=torch.int32, device=dev), d2=torch.zeros((n,), dtype=torch.float64, device=dev),
               transform=torch.zeros((nc, 12), dtype=torch.float64, device=dev))
    ctx.check(lib().ismhip_ransac_hypothesis(ctx._h, C.c_int(nc), _p(off), _p(src_xyz), _p(tgt_xyz), _p(thr), C.c_ulonglong(seed), _p(hyp),
                                             _p(out["inlier"]), _p(out["valid"]), _p(out["n_inliers"]), _p(out["d2"]), _p(out["transform"])),
              "ismhip_ransac_hypothesis")
    return out


def _ransac_params(ransac, n_classes):
    """ransac: dict(vote_keypoint, vote_keypoint_training [n_slots, 3] device; inlier_threshold; optional class_inlier_threshold [n_classes],
    max_iterations, seed) -> (RansacParams, objects to keep alive)"""
    cthr = ransac.get("class_inlier_threshold")
    if cthr is not None:
        cthr = np.ascontiguousarray(np.asarray(cthr, dtype=np.float32))
        assert cthr.shape == (n_classes,)
    R = RansacParams(_p(ransac["vote_keypoint"]).value, _p(ransac["vote_keypoint_training"]).value, float(ransac.get("inlier_threshold", 0.1)),
                     cthr.ctypes.data if cthr is not None else None, int(ransac.get("max_iterations", RANSAC_MAX_ITERATIONS)),
                     int(ransac.get("seed", RANSAC_SEED)))
    return R, cthr


def _maxima_outputs(n_obj, max_maxima, n_classes, dev):
    """the output tensors of find_maxima / hough3d_maxima"""
    torch = _torch()
    return dict(
        n=torch.empty((n_obj,), dtype=torch.int32, device=dev),
        pos=torch.empty((n_obj, max_maxima, 3), dtype=torch.float32, device=dev),
        weight=torch.empty((n_obj, max_maxima), dtype=torch.float32, device=dev),
        cls=torch.empty((n_obj, max_maxima), dtype=torch.int32, device=dev),
        inst=torch.empty((n_obj, max_maxima), dtype=torch.int32, device=dev),
        inst_weight=torch.empty((n_obj, max_maxima), dtype=torch.float32, device=dev),
        bbox_size=torch.empty((n_obj, max_maxima, 3), dtype=torch.float32, device=dev),
        n_votes=torch.empty((n_obj, max_maxima), dtype=torch.int32, device=dev),
        class_score=torch.empty((n_obj, n_classes), dtype=torch.float32, device=dev),
    )


def _maxima_call(ctx, symbol, so, votes, P, out, bq_out, ransac):
    """calls `symbol` (with ransac: symbol + "_ransac", which also fills out["transform"]) on the arguments both voting back ends
    share; P is the back end's params struct, bq_out the AverageRotation output or None"""
    n_obj, max_maxima = out["weight"].shape
    args = (ctx._h, C.c_int(n_obj), _p(so), _p(votes["pos"]), _p(votes["weight"]), _p(votes["cls"]),
            _p(votes["inst"]), _p(votes.get("bbox_size")), C.byref(P), _p(out["n"]), _p(out["pos"]),
            _p(out["weight"]), _p(out["cls"]), _p(out["inst"]), _p(out["inst_weight"]), _p(out["bbox_size"]),
            _p(out["n_votes"]), _p(out["class_score"]))
    if ransac is not None:
        symbol += "_ransac"
        R, _keep = _ransac_params(ransac, out["class_score"].shape[1])
        out["transform"] = _torch().zeros((n_obj, max_maxima, 4, 4), dtype=out["weight"].dtype, device=out["weight"].device)
        args += (C.byref(R), _p(out["transform"]))
    ctx.check(getattr(lib(), symbol)(*args), symbol)
    if bq_out is not None:
        out["bbox_quat"] = bq_out
    return out


def find_maxima(ctx, slot_offsets, votes, n_classes, bandwidth, threshold=1e-3, max_iter=1000, kernel=KERNEL_GAUSSIAN,
                suppression=SUPPRESS_AVERAGE, min_votes_threshold=1, min_threshold=0.0, best_k=-1, max_maxima=16,
                class_bandwidth=None, max_filter=0, average_rotation=False, single_object_max_type=SOM_MEANSHIFT,
                object_centroid=None, object_radius=None, ransac=None):
    """average_rotation: votes["bbox_quat"] in, out["bbox_quat"] per maximum; single_object_max_type != SOM_MEANSHIFT needs
    object_centroid [n_obj,3] (and object_radius [n_obj] for SOM_MODEL_RADIUS) as device tensors; ransac (see _ransac_params):
    Voting.RansacVoteFiltering through ismhip_find_maxima_ransac, out["transform"] [n_obj, max_maxima, 4, 4]"""
    torch = _torch()
    so = _u32(slot_offsets)
    n_obj = len(so) - 1
    dev = votes["pos"].device
    cbw = None if class_bandwidth is None else np.ascontiguousarray(np.asarray(class_bandwidth, dtype=np.float32))
    bq_out = torch.empty((n_obj, max_maxima, 4), dtype=torch.float32, device=dev) if average_rotation else None
    P = MaximaParams(n_classes, cbw.ctypes.data if cbw is not None else None, bandwidth, threshold, max_iter, kernel, suppression,
                     min_votes_threshold, min_threshold, best_k, max_maxima, max_filter,
                     _p(votes["bbox_quat"]).value if average_rotation else None, _p(bq_out).value, single_object_max_type,
                     _p(object_centroid).value, _p(object_radius).value)
    return _maxima_call(ctx, "ismhip_find_maxima", so, votes, P, _maxima_outputs(n_obj, max_maxima, n_classes, dev), bq_out, ransac)


def hough3d_maxima(ctx, slot_offsets, votes, n_classes, bin_size, min_coord=(-5, -5, -5), max_coord=(5, 5, 5), use_interpolation=True,
                   rel_threshold=0.8, min_votes_threshold=1, min_threshold=0.0, best_k=-1, max_maxima=16, class_bin=None, max_filter=0,
                   average_rotation=False, ransac=None):
    """VotingHough3D on the device: same outputs as find_maxima (ransac: as there, through ismhip_hough3d_maxima_ransac)"""
    torch = _torch()
    so = _u32(slot_offsets)
    n_obj = len(so) - 1
    dev = votes["pos"].device
    cb = None if class_bin is None else np.ascontiguousarray(np.asarray(class_bin, dtype=np.float32))
    bq_out = torch.empty((n_obj, max_maxima, 4), dtype=torch.float32, device=dev) if average_rotation else None
    P = HoughParams(n_classes, (C.c_float * 3)(*min_coord), (C.c_float * 3)(*max_coord), bin_size, cb.ctypes.data if cb is not None else None,
                    1 if use_interpolation else 0, rel_threshold, min_votes_threshold, min_threshold, best_k, max_maxima, max_filter,
                    _p(votes["bbox_quat"]).value if average_rotation else None, _p(bq_out).value)
    return _maxima_call(ctx, "ismhip_hough3d_maxima", so, votes, P, _maxima_outputs(n_obj, max_maxima, n_classes, dev), bq_out, ransac)


def _train_activate(ctx, symbol, metric, desc, lrf, kx, ky, kz, feat_class, feat_model, feat_center, n_classes, codewords, vote_cap, activation):
    """the two training entries: host output buffers for at most vote_cap votes, the call (`activation` = the arguments between the
    codewords and n_classes, where the two differ) and the dict of host arrays trimmed to the words and votes that were written"""
    n, dim = desc.shape
    fc, fm = _u32(feat_class), _u32(feat_model)
    ctr = np.ascontiguousarray(np.asarray(feat_center, dtype=np.float32))
    C_ = int(n_classes if n_classes is not None else fc.max() + 1)
    ncw = n if codewords is None else int(codewords.shape[0])
    nw = C.c_int32(0)
    word_src = np.empty(ncw, np.uint32); vo = np.empty(ncw + 1, np.uint32); vf = np.empty(vote_cap, np.uint32)
    vxyz = np.empty((vote_cap, 3), np.float32); vw = np.empty(vote_cap, np.float32); vcw = np.empty(vote_cap, np.float32); sig = np.empty(C_, np.float32)
    ctx.check(getattr(lib(), symbol)(ctx._h, C.c_int(metric), C.c_int(n), C.c_int(dim), _p(desc), _p(lrf), _p(kx), _p(ky), _p(kz), _p(fc), _p(fm),
                                     _p(ctr), C.c_int(ncw), _p(codewords), *activation, C.c_int(C_), C.byref(nw), _p(word_src),
                                     _p(vo), _p(vf), _p(vxyz), _p(vw), _p(vcw), _p(sig)), symbol)
    m = nw.value; nv = int(vo[m])
    return dict(word_src=word_src[:m].copy(), vote_offsets=vo[:m + 1].copy(), vote_feature=vf[:nv].copy(), vote_xyz=vxyz[:nv].copy(),
                vote_weight=vw[:nv].copy(), vote_class_weight=vcw[:nv].copy(), class_sigma=sig)


def train_activate(ctx, metric, desc, lrf, kx, ky, kz, feat_class, feat_model, feat_center, k=1, clean_up=True, n_classes=None, codewords=None):
    """Codebook::activate on the device (features class-major; codewords = device matrix of cluster centres, None = the features
    themselves) -> dict of host arrays (word_src, vote_offsets, vote_feature, vote_xyz, vote_weight, vote_class_weight, class_sigma)"""
    return _train_activate(ctx, "ismhip_train_activate", metric, desc, lrf, kx, ky, kz, feat_class, feat_model, feat_center, n_classes, codewords,
                           desc.shape[0] * k, (C.c_int(k), C.c_int(1 if clean_up else 0)))


def train_activate_lists(ctx, metric, desc, lrf, kx, ky, kz, feat_class, feat_model, feat_center, act_offsets, act_idx, n_classes=None, codewords=None):
    """Codebook::activate with a variable number of activations per feature (ActivationStrategyThreshold): act_offsets [n+1] (host
    array or device int32 tensor), act_idx [n_act] device int32 rows of the codewords -> the dict of train_activate"""
    act_offsets = _act_offsets(act_offsets, desc.device)
    na = int(act_idx.shape[0])
    return _train_activate(ctx, "ismhip_train_activate_lists", metric, desc, lrf, kx, ky, kz, feat_class, feat_model, feat_center, n_classes, codewords,
                           max(na, 1), (_p(act_offsets), _p(act_idx), C.c_int64(na)))


CENTERS_INIT = {"FLANN_CENTERS_RANDOM": 0, "FLANN_CENTERS_GONZALES": 1, "FLANN_CENTERS_KMEANSPP": 2}


def kmeans(ctx, metric, desc, n_clusters, max_iterations=1000, centers_init="FLANN_CENTERS_KMEANSPP", seed=0):
    """ClusteringKMeans::cluster on the device -> (centers [m, dim] device, assign [n] device int32, dist [n] device, iterations)"""
    torch = _torch()
    n, dim = desc.shape
    kc = min(int(n_clusters), n)
    centers = torch.empty((kc, dim), dtype=torch.float32, device=desc.device)
    assign = torch.empty(n, dtype=torch.int32, device=desc.device)
    dist = torch.empty(n, dtype=torch.float32, device=desc.device)
    m = C.c_int32(0); it = C.c_int32(0)
    ctx.check(lib().ismhip_kmeans(ctx._h, C.c_int(metric), C.c_int(n), C.c_int(dim), _p(desc), C.c_int(kc), C.c_int(max_iterations),
                                  C.c_int(CENTERS_INIT[centers_init] if isinstance(centers_init, str) else int(centers_init)), C.c_ulonglong(seed),
                                  _p(centers), _p(assign), _p(dist), C.byref(m), C.byref(it)), "ismhip_kmeans")
    return centers[:m.value], assign, dist, it.value


RANK_TYPES = {"KNNActivation": 0, "Incremental": 1, "Strangeness": 2, "NaiveBayes": 3}


def rank_scores(ctx, rank_type, desc, class_offsets, k_search=10, dist_threshold=0.1, increment_type=0, out=None):
    """FeatureRanking::iComputeScores of one subclass on the device (desc [n, dim] class-major, class_offsets host [n_classes + 1])
    -> score [n] device float32 (`out` when given: an error leaves it unwritten)"""
    torch = _torch()
    n, dim = desc.shape
    off = _u32(class_offsets)
    score = torch.empty(n, dtype=torch.float32, device=desc.device) if out is None else out
    t = RANK_TYPES[rank_type] if isinstance(rank_type, str) else int(rank_type)
    ctx.check(lib().ismhip_rank_scores(ctx._h, C.c_int(t), C.c_int(n), C.c_int(dim), _p(desc), C.c_int(len(off) - 1), _p(off), C.c_int(k_search),
                                       C.c_float(dist_threshold), C.c_int(increment_type), _p(score)), "ismhip_rank_scores")
    return score


def rank_select(ctx, score, class_offsets, factor=0.75, extract_offset=0.0, out=None):
    """rankFeaturesWithScores + extractSubsetFromRankedList -> (keep [n] device uint8, n_keep host [n_classes] uint32); `out` =
    (keep, n_keep) buffers to write into (an error leaves them unwritten)"""
    torch = _torch()
    n = score.shape[0]
    off = _u32(class_offsets)
    keep, n_keep = out if out is not None else (torch.empty(n, dtype=torch.uint8, device=score.device), np.zeros(len(off) - 1, np.uint32))
    ctx.check(lib().ismhip_rank_select(ctx._h, C.c_int(n), C.c_int(len(off) - 1), _p(off), _p(score), C.c_float(factor), C.c_float(extract_offset),
                                       _p(keep), _p(n_keep)), "ismhip_rank_select")
    return keep, n_keep


PARTIAL_SHOT_SIGNATURES = {          # Codebook::getSignatureMask (codebook/codebook.cpp:952-1036): kept signatures of the 32
    "front": range(8, 24), "dense_x": range(8, 24), "back": list(range(0, 8)) + list(range(24, 32)), "sparse_x": list(range(0, 8)) + list(range(24, 32)),
    "left": range(16, 32), "positive_y": range(16, 32), "right": range(0, 16), "negative_y": range(0, 16),
    "top": range(1, 32, 2), "dense_z": range(1, 32, 2), "bottom": range(0, 32, 2), "sparse_z": range(0, 32, 2),
    "dense_x_or_z": sorted(set(range(8, 24)) | set(range(1, 32, 2))), "dense_x_and_z": range(9, 24, 2),
    "front_turn_left": range(12, 28), "front_turn_right": range(4, 20),
}


def partial_shot_columns(kind):
    """descriptor columns of SHOT-352 kept by UsePartialShot / PartialShotType (unknown type: the complete descriptor, with the reference's warning)"""
    sig = PARTIAL_SHOT_SIGNATURES.get(kind, range(32))
    return np.asarray([s * 11 + j for s in sig for j in range(11)], np.int32)


def gather_columns(ctx, src, cols):
    torch = _torch()
    cols = np.ascontiguousarray(cols, np.int32)
    out = torch.empty((src.shape[0], len(cols)), dtype=torch.float32, device=src.device)
    ctx.check(lib().ismhip_gather_columns(ctx._h, C.c_int(src.shape[0]), C.c_int(src.shape[1]), _p(src), C.c_int(len(cols)), _p(cols), _p(out)), "ismhip_gather_columns")
    return out
