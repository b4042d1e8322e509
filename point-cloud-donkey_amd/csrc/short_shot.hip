// short_shot.hip — the generalised Short SHOT descriptor (Features type "SHORT_SHOT"), one 64-lane wavefront per keypoint.
// Reference seam: FeaturesSHORTSHOT::compute_descriptor / compute_shape_descriptor / linear_interpolation / correct_bin
// (features/features_short_shot.cpp:77-283). Unlike SHOT-352 its arithmetic is written out completely in the reference's own source:
// a spherical grid of r x e x a bins in the keypoint's SHOT frame, a three-way linear interpolation, double accumulation, an L2 norm.
// No normals, no five-neighbour rule.
//
// Gather model: algorithmic bytes per keypoint = M_k * 16 + 12 + 36 + 4 * D (M_k = radius neighbours, D = r e a <= 256): 16 bytes fewer
// per neighbour than SHOT-352 (the normal array is not read) and a row of 32-1024 bytes instead of 1408. The gather does not bound the
// kernel: the per-neighbour arithmetic and the LDS deposits do (0.28 of the HBM peak on the model's bytes).
//
// Structure per wave: that of k_shot (shot.hip) -- the candidate x-runs of the query ball in 16 interleaved segments, the lanes inside
// the ball compacted by ballot + prefix popcount into a 128-entry LDS queue, the per-neighbour math on full waves, deposits into a
// per-wave LDS histogram in 2^-28 fixed point (ds_add_u64: order-independent, bitwise reproducible).
//
// The histogram is continuous in the raw bin coordinates EXCEPT where a coordinate's fraction is exactly 0.5 (the secondary bin of that
// axis jumps to the other side and still carries the other two axes' shares) and at the int() truncations (the other axes' secondary
// bins ride on the primary bin), so every hard decision must be the reference's. The reference's sequence -- steps 4 and 5 in FP64 with
// libm's acos / atan2, then a cast to float -- costs ~400 FP64 lane-operations per neighbour: at bench size (1786 neighbours per
// keypoint) that, not the gather, bounds the kernel (measured 5.9 ms per 256 objects against 2.9 ms for k_shot). So every neighbour is
// first ESTIMATED in float (sshot_polar and sshot_scaled in short_common.h: raw values to a few 1e-7 per bin, bound there); only where an estimate comes within eps of
// a value at which a decision changes -- an integer n >= 1, or n + 0.5 -- does the wave re-take that neighbour in FP64 exactly as
// written in the reference (sqrt and division IEEE-exact; acos, atan2, log from the device's libm, a few ulp of double from the
// host's, ~1e-13 in raw units). Away from the decisions the interpolation shares are continuous, and a raw value off by 1e-6 moves a
// share by 1e-6: far inside the 1e-4 parity tolerance. A logarithmic radius always takes the FP64 sequence.
#include "short_common.h"

namespace {

struct ShortShotArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    const uint32_t* kp_off; const float *kx, *ky, *kz;
    const float* lrf; float radius, r2;
    double radius_d, min_radius, ln_rmin, ln_rmax_rmin;
    SshotScale g;                              // the float estimate's scales and eps (short_common.h)
    float min_radius_f;
    int log_radius, r_bins, e_bins, a_bins;
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;   // keypoints in cell order (nullptr: as they come)
};

#define SSHOT_MAX_DIM   256

struct ShortShotSmem {
    // A short histogram draws many lanes of one deposit onto the same address, and same-address LDS atomics of a wave instruction
    // serialise. The 256 slots a wave owns therefore hold 256 / D COPIES of the D bins; lane l deposits into copy l % copies and the
    // copies are summed (integers: exactly) before the norm.
    sshot_bin_t hist[4][SSHOT_MAX_DIM];
    float4 qd[4][128];       // dx, dy, dz, d2 of queued neighbours
    WaveRows rows[4];
};

// Per-neighbour update (:125-140, :159-243). All 64 lanes call it; 'act' marks lanes that hold a neighbour. The steps are those of
// short_common.h: estimate, FP64 re-take where the estimate is not clear of a decision, deposits.
__device__ __forceinline__ void sshot_neighbour(const ShortShotArgs& a, sshot_bin_t* hist, int dim, bool act,
                                                float dx, float dy, float dz, float d2,
                                                const float fx[3], const float fy[3], const float fz[3]) {
    if (!act) return;
    if (d2 <= 1e-15f) return;                                                     // distances[j] > 1E-15 on the SQUARED distance (:127)
    const float xf = (dx * fx[0] + dy * fx[1]) + dz * fx[2];                      // float products, unfused, in this order
    const float yf = (dx * fy[0] + dy * fy[1]) + dz * fy[2];
    const float zf = (dx * fz[0] + dy * fz[1]) + dz * fz[2];
    const int rb = a.r_bins, eb = a.e_bins, ab = a.a_bins;
    float r, theta, phi, raw_r, raw_theta, raw_phi;
    bool below_min;
    sshot_polar(xf, yf, zf, r, theta, phi);
    const bool clear = sshot_scaled(a.g, r, theta, phi, raw_r, raw_theta, raw_phi);
    const bool min_clear = sshot_min_clear(r, a.min_radius_f, below_min);
    if (a.log_radius || !min_clear || !clear) {
        const float4 e = sshot_exact(xf, yf, zf, a.radius_d, a.min_radius, a.ln_rmin, a.ln_rmax_rmin, a.log_radius, rb, eb, ab);
        raw_r = e.x; raw_theta = e.y; raw_phi = e.z; below_min = e.w != 0.f;
    }
    if (below_min) return;
    sshot_shape_deposits(hist, dim, rb, eb, ab, raw_r, raw_theta, raw_phi);
}

// 108 VGPRs, no scratch, 20 KiB LDS per workgroup: 4 waves per SIMD (the compiler's resource report; held to 96 it spills 16)
__global__ __launch_bounds__(256, 4) void k_short_shot(ShortShotArgs a) {
    __shared__ ShortShotSmem sm;
    int o, bx;
    if (!xcd_object_block(a.nbx, a.n_obj, o, bx)) return;
    const int wv = threadIdx.x >> 6;
    const int lane = lane_id();
    if (a.kp_off[o] + bx * 4 + wv >= a.kp_off[o + 1]) return;          // wave-uniform; no block-level barrier below
    const uint32_t k = ordered_keypoint(a.kp_perm, a.kp_off[o], (uint32_t)(bx * 4 + wv));
    const int D = a.r_bins * a.e_bins * a.a_bins;                       // 1 .. 256 (checked by the launcher)
    const int copies = SSHOT_MAX_DIM / D;
    float* out = a.desc + (size_t)k * D;
    const float cx = a.kx[k], cy = a.ky[k], cz = a.kz[k];
    const float* f = a.lrf + (size_t)k * 9;
    const float fx[3] = {f[0], f[1], f[2]}, fy[3] = {f[3], f[4], f[5]}, fz[3] = {f[6], f[7], f[8]};
    const GridMeta m = a.meta[o];
    CellRange cr;
    const bool ok = isfinite(fx[0]) && isfinite(fy[0]) && isfinite(fz[0]) && isfinite(cx) && isfinite(cy) && isfinite(cz);
    if (!ok || !ball_cells(m, cx, cy, cz, a.radius, cr)) {
        for (int i = lane; i < D; i += 64) out[i] = __builtin_nanf("");
        if (a.count && lane == 0) a.count[k] = 0;
        return;
    }
    for (int i = lane; i < SSHOT_MAX_DIM; i += 64) sm.hist[wv][i] = 0ull;
    sshot_bin_t* hist = sm.hist[wv] + (lane % copies) * D;              // this lane's copy
    const uint32_t* cs = a.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const uint32_t base = a.pt_off[o];
    uint32_t qn = 0, qh = 0, total = 0;
    ball_for_each<16, true>(m, cs, cr, cx, cy, cz, a.radius, lane, sm.rows[wv],
                  [&](uint32_t i, bool) { return a.sp4[base + i]; },      // invalid lanes carry index 0 (common.h): no branch, no zero fill
                  [&](const float4& p, uint32_t, bool v) {
        bool pass = false; float dx = 0, dy = 0, dz = 0, d2 = 0;
        if (v) {
            const float px = p.x, py = p.y, pz = p.z;
            d2 = sqdist3(px, py, pz, cx, cy, cz);
            dx = px - cx; dy = py - cy; dz = pz - cz;
            pass = d2 < a.r2;
        }
        const unsigned long long mask = __ballot(pass);
        if (pass) {
            const uint32_t pos = (qh + qn + __popcll(mask & ((1ull << lane) - 1ull))) & 127u;      // 128-entry circular queue
            sm.qd[wv][pos] = make_float4(dx, dy, dz, d2);
        }
        const uint32_t c = __popcll(mask);
        qn += c; total += c;
        if (qn >= 64) {
            // a full wave of neighbours (LDS traffic of one wave is ordered; no barrier needed)
            const float4 e = sm.qd[wv][(qh + lane) & 127u];
            sshot_neighbour(a, hist, D, true, e.x, e.y, e.z, e.w, fx, fy, fz);
            qh = (qh + 64) & 127u; qn -= 64;
        }
    });
    if (qn > 0) {
        const float4 e = sm.qd[wv][(qh + lane) & 127u];
        sshot_neighbour(a, hist, D, (uint32_t)lane < qn, e.x, e.y, e.z, e.w, fx, fy, fz);
    }
    if (a.count && lane == 0) a.count[k] = total;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");             // the deposits of the other lanes are read below
    // L2 norm (:143-152): double sum of squares, sqrt, double division, cast to float. No contributing neighbour: 0 / 0, a NaN row.
    double v[SSHOT_MAX_DIM / 64];
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < SSHOT_MAX_DIM / 64; ++j) {
        const int i = lane + 64 * j;
        sshot_bin_t h = 0ull;
        if (i < D) for (int c = 0; c < copies; ++c) h += sm.hist[wv][c * D + i];
        v[j] = (double)h * SSHOT_FIX_INV;
        acc += v[j] * v[j];
    }
    const double norm = sqrt(wave_sum_d(acc));
#pragma unroll
    for (int j = 0; j < SSHOT_MAX_DIM / 64; ++j) {
        const int i = lane + 64 * j;
        if (i < D) out[i] = (float)(v[j] / norm);
    }
}

}  // namespace

extern "C" {

int ismhip_short_shot(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                      const float* kpx, const float* kpy, const float* kpz, const float* lrf9,
                      float radius, float min_radius, int log_radius, int r_bins, int e_bins, int a_bins,
                      float* desc_out, uint32_t* neighbour_count_out) {
    const char* name = "short_shot";
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (r_bins < 1 || e_bins < 1 || a_bins < 1) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_shot: fewer than one bin on an axis");
    if ((long long)r_bins * e_bins * a_bins > ISMHIP_SHORT_SHOT_MAX_DIM)
        return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "short_shot: more than 256 bins");
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !lrf9 || !desc_out || !(radius > 0.f) || !(min_radius >= 0.f) || !std::isfinite(min_radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_shot: bad argument");
    // the reference divides by log(Radius / min_radius): 0 for min_radius == 0 (and NaN -> int); refused, never altered
    if (log_radius && !(min_radius > 0.f && min_radius < radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_shot: logarithmic radius needs 0 < min_radius < radius");
    const int n_obj = cloud->n_obj;
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, name, kp_offsets_h, n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK) return rc;
    const uint32_t maxk = kp.max_run;
    if (maxk == 0) return ISMHIP_OK;
    ShortShotArgs a;
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz; a.lrf = lrf9;
    a.radius = radius; a.r2 = (float)((double)radius * (double)radius);
    a.radius_d = (double)radius; a.min_radius = (double)min_radius;
    a.ln_rmin = min_radius == 0.f ? 0.0 : log((double)min_radius);
    a.ln_rmax_rmin = min_radius == 0.f ? 0.0 : log((double)radius / (double)min_radius);
    a.log_radius = log_radius ? 1 : 0; a.r_bins = r_bins; a.e_bins = e_bins; a.a_bins = a_bins;
    a.g = sshot_scale_of(r_bins, e_bins, a_bins, radius);
    a.min_radius_f = min_radius;
    a.desc = desc_out; a.count = neighbour_count_out;
    a.n_obj = ctx->xcd_map ? n_obj : 0; a.nbx = (int)((maxk + 3) / 4);
    TimerScope ts(ctx, name);
    a.kp_perm = ism_kp_order(ctx, cloud, kp_offsets_h, kp.dev, kpx, kpy, kpz, maxk);
    const dim3 grid(ctx->xcd_map ? xcd_object_grid((unsigned)a.nbx, n_obj) : (unsigned)a.nbx * (unsigned)n_obj);
    hipLaunchKernelGGL(k_short_shot, grid, dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, name);
    return ISMHIP_OK;
}

}  // extern "C"
