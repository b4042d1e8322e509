// spin_image.hip — the SpinImage descriptor (Features type "SpinImage"), (w + 1)(2w + 1) floats, 153 at the reference's width 8: the
// support cylinder round an axis through the keypoint, every neighbour deposited bilinearly at (alpha, beta) = (distance from the axis,
// height along it). Reference seam: FeaturesSpinImage::iComputeDescriptors (features/features_spin_image.cpp:28-87) -> PCL 1.10
// SpinImageEstimation::computeSiForPoint as :61-69 configure it (image width 8, rectangular, support-angle cosine 0, min_pts_neighb 0);
// the keypoint's normal is looked up by coordinate equality (:36-53). Definition and the named deviations: DESIGN.md 4.15.
//
// Two entries, one launch each:
//   k_keypoint_normals (timer "keypoint_normals"): per keypoint one THREAD reads the keypoint's own grid cell -- a point with equal
//                        coordinates was binned by the same cell_coord -- and keeps the lowest original index among the equal points
//   k_spin_image       (timer "spin_image"): per keypoint one wavefront sweeps the ball (shot_wave.h) and deposits into its LDS histogram
// Gather model: sum_k M_k * 16 + K (24 + 4 D) bytes (M_k = candidates of the ball: the 16-byte position record; neighbour normals are
// never read; the centre, the axis, the row).
//
// The per-neighbour decisions (skip, bad cosine, cylinder test, the two floors) are taken in FP64 from float inputs, in the sequence of
// the definition, so they are those of the float64 restatement (tests/spin_image_ref.py). The deposits are 2^-28 fixed point
// (shot_dep), the row sum an integer wave reduction: the row does not depend on the order the neighbours arrive in.
#include "shot_deposit.h"
#include <cfloat>

namespace {

#define SPIN_MAX_WIDTH 25                            // the widest image whose row ismhip_knn takes
static_assert((SPIN_MAX_WIDTH + 1) * (2 * SPIN_MAX_WIDTH + 1) <= ISMHIP_SHORT_CSHOT_MAX_DIM &&
              (SPIN_MAX_WIDTH + 2) * (2 * SPIN_MAX_WIDTH + 3) > ISMHIP_SHORT_CSHOT_MAX_DIM, "SPIN_MAX_WIDTH");

struct SpinArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *sn4;
    const uint32_t* kp_off; const float *kx, *ky, *kz;
    const float *ax, *ay, *az;            // k_spin_image: the axes
    float radius, r2;
    int w, dim;                           // image width, (w + 1)(2w + 1)
    double bin, lim;                      // (double)radius / w / sqrt(2.0), bin * w
    float* desc; uint32_t* count;
    float *nxo, *nyo, *nzo; int32_t* src; // k_keypoint_normals: the outputs
    int n_obj, nbx;
    const uint32_t* kp_perm;
};

// ---- the lookup ---------------------------------------------------------------------------------------------------------------
// features_spin_image.cpp:41-53: the first point (lowest index) of the cloud whose coordinates compare == to the keypoint's hands over its
// normal; none: the default-constructed pcl::Normal, all zero.
__global__ __launch_bounds__(256) void k_keypoint_normals(SpinArgs a) {
    const int o = blockIdx.y;
    const uint32_t k = a.kp_off[o] + blockIdx.x * 256u + threadIdx.x;
    if (k >= a.kp_off[o + 1]) return;
    const float qx = a.kx[k], qy = a.ky[k], qz = a.kz[k];
    const GridMeta& m = a.meta[o];
    const uint32_t base = a.pt_off[o];
    uint32_t best = 0xffffffffu, best_i = 0;
    if (isfinite(qx) && isfinite(qy) && isfinite(qz) && m.n_finite > 0) {
        const uint32_t* cs = a.cell_start + (size_t)o * ISM_GRID_STRIDE;
        const int c = (cell_coord(qz, m.minv[2], m.inv_cell[2], m.dim[2]) * m.dim[1] + cell_coord(qy, m.minv[1], m.inv_cell[1], m.dim[1])) * m.dim[0] +
                      cell_coord(qx, m.minv[0], m.inv_cell[0], m.dim[0]);
        const uint32_t e = cs[c + 1];
        for (uint32_t i = cs[c]; i < e; ++i) {
            const float4 p = a.sp4[base + i];
            const uint32_t idx = __float_as_uint(p.w);
            if (p.x == qx && p.y == qy && p.z == qz && idx < best) { best = idx; best_i = i; }
        }
    }
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
    if (best != 0xffffffffu) n = a.sn4[base + best_i];
    a.nxo[k] = n.x; a.nyo[k] = n.y; a.nzo[k] = n.z;
    if (a.src) a.src[k] = best != 0xffffffffu ? (int32_t)best : -1;
}

// ---- the descriptor -----------------------------------------------------------------------------------------------------------
struct SpinSmem {
    float4 qd[4][128];                    // dx, dy, dz, d2 of queued neighbours
    WaveRows rows[4];
};

// 12 KiB static LDS per workgroup (queue 8 KiB, row tables 4 KiB) and 4 * dim * 8 bytes dynamic: 4.8 KiB at width 8, 41.4 KiB at 25
__global__ __launch_bounds__(256) void k_spin_image(SpinArgs a) {
    extern __shared__ __attribute__((aligned(16))) shot_bin_t spin_hist[];   // behind the 12 288 static bytes: 8-byte aligned for ds_add_u64
    __shared__ SpinSmem sm;
    ShotWave w;
    const int D = a.dim;
    if (!shot_wave_place(a, D, w)) return;
    const int lane = w.lane;
    const float nx = a.ax[w.k], ny = a.ay[w.k], nz = a.az[w.k];
    // A keypoint or an axis that is not finite: the whole row NaN, count 0. A ball that misses the grid holds no point: a ZERO row,
    // count 0, as the reference keeps it (not shot_wave_ball, whose rule for the other descriptors is NaN).
    const bool fin = isfinite(w.cx) && isfinite(w.cy) && isfinite(w.cz) && isfinite(nx) && isfinite(ny) && isfinite(nz);
    if (!fin || !ball_cells(w.m, w.cx, w.cy, w.cz, a.radius, w.cr)) {
        const float v = fin ? 0.f : __builtin_nanf("");
        for (int i = lane; i < D; i += 64) w.row[i] = v;
        if (a.count && lane == 0) a.count[w.k] = 0;
        return;
    }
    shot_bin_t* hist = spin_hist + (size_t)w.wv * D;
    for (int i = lane; i < D; i += 64) hist[i] = 0ull;
    const int iw = a.w, stride = 2 * a.w + 1;
    const double bin = a.bin, lim = a.lim;
    bool bad = false;                                                     // a cosine outside [-1, 1] by more than rounding: PCL throws
    const uint32_t total = shot_wave_neighbours<16, false>(a, w, sm.qd[w.wv], nullptr, sm.rows[w.wv],
        [&](bool act, uint32_t, float dx, float dy, float dz, float d2) {
            if (!act) return;
            const float norm = sqrtf(d2);
            if ((double)norm < 10.0 * DBL_EPSILON) return;                // the keypoint's own point and its coincident twins
            const float dot = (dx * nx + dy * ny) + dz * nz;
            double c = (double)dot / (double)norm;
            if (!(fabs(c) <= 1.0 + 10.0 * (double)FLT_EPSILON)) { bad = true; return; }   // (or no number: a dot product that overflowed)
            c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
            const double beta = (double)norm * c, alpha = (double)norm * sqrt(1.0 - c * c);
            if (fabs(beta) >= lim || alpha >= lim) return;                // outside the support cylinder
            const double tb = beta / bin, ta = alpha / bin;
            const int fb = (int)floor(tb), ia = (int)floor(ta), ib = fb + iw;
            const double wa = ta - (double)ia, wb = tb - (double)fb;
            // ia = w or ib = 2w is reached only when the quotient rounds up onto w; the entries past the matrix then carry a weight of an
            // ulp of w, dropped here and in the restatement
            const bool ina = ia + 1 <= iw, inb = ib + 1 <= 2 * iw;
            shot_bin_t* h = hist + ia * stride + ib;
            shot_dep(h, 0, (1.0 - wa) * (1.0 - wb));
            if (ina) shot_dep(h, stride, wa * (1.0 - wb));
            if (inb) shot_dep(h, 1, (1.0 - wa) * wb);
            if (ina && inb) shot_dep(h, stride + 1, wa * wb);
        });
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // the deposits of the other lanes are read below
    const bool nan_row = __ballot(bad) != 0ull;
    unsigned long long s = 0ull;
    for (int i = lane; i < D; i += 64) s += hist[i];
    s = wave_sum_u64(s);
    // more than one neighbour: every bin over the sum of the bins (in double; no deposit at all: 0 / 0, the reference's NaN row);
    // otherwise the bins as they are
    for (int i = lane; i < D; i += 64) {
        const double h = (double)hist[i];
        w.row[i] = nan_row ? __builtin_nanf("") : (total > 1 ? (float)(h / (double)s) : (float)(h * SHOT_FIX_INV));
    }
}

int spin_common(ismhip_ctx* ctx, const char* name, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h, const float* kpx, const float* kpy,
                const float* kpz, SpinArgs& a, uint32_t& maxk) {
    RaggedOffsets kp;
    maxk = 0;
    int rc = ism_ragged_offsets(ctx, name, kp_offsets_h, cloud->n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK) return rc;
    maxk = kp.max_run;
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4; a.sn4 = cloud->sn4;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz;
    a.n_obj = ctx->xcd_map ? cloud->n_obj : 0; a.nbx = (int)((maxk + 3) / 4);
    return ISMHIP_OK;
}

}  // namespace

extern "C" {

int ismhip_keypoint_normals(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                            const float* kpx, const float* kpy, const float* kpz,
                            float* knx_out, float* kny_out, float* knz_out, int32_t* src_index_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !knx_out || !kny_out || !knz_out)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "keypoint_normals: bad argument");
    SpinArgs a = {};
    uint32_t maxk;
    int rc = spin_common(ctx, "keypoint_normals", cloud, kp_offsets_h, kpx, kpy, kpz, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.nxo = knx_out; a.nyo = kny_out; a.nzo = knz_out; a.src = src_index_out;
    TimerScope ts(ctx, "keypoint_normals");
    hipLaunchKernelGGL(k_keypoint_normals, dim3((maxk + 255) / 256, cloud->n_obj), dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_keypoint_normals");
    return ISMHIP_OK;
}

int ismhip_spin_image(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                      const float* kpx, const float* kpy, const float* kpz, const float* ax, const float* ay, const float* az,
                      float radius, int image_width, float* desc_out, uint32_t* neighbour_count_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !ax || !ay || !az || !desc_out || !(radius > 0.f) || image_width < 1)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "spin_image: bad argument");
    if (image_width > SPIN_MAX_WIDTH)
        return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "spin_image: image width above 25 (rows longer than 1344)");
    SpinArgs a = {};
    uint32_t maxk;
    int rc = spin_common(ctx, "spin_image", cloud, kp_offsets_h, kpx, kpy, kpz, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.ax = ax; a.ay = ay; a.az = az;
    a.radius = radius; a.r2 = (float)((double)radius * (double)radius);
    a.w = image_width; a.dim = (image_width + 1) * (2 * image_width + 1);
    a.bin = (double)radius / image_width / sqrt(2.0); a.lim = a.bin * image_width;
    a.desc = desc_out; a.count = neighbour_count_out;
    const ShotCall c = {ctx, cloud, kp_offsets_h, kpx, kpy, kpz, nullptr, nullptr, radius, desc_out, neighbour_count_out, "spin_image"};
    return shot_launch(c, a, maxk, k_spin_image, (size_t)4 * a.dim * sizeof(shot_bin_t));
}

}  // extern "C"
