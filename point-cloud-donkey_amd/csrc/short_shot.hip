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
// Structure per wave: that of the SHOT family (shot_wave.h: set-up, the ball's candidates in 16 interleaved segments, the queue of
// those inside the ball -- without their index, no array of this kernel is gathered by it -- and the per-neighbour math on full
// waves); deposits into a per-wave LDS histogram in 2^-28 fixed point (ds_add_u64: order-independent, bitwise reproducible).
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
    shot_bin_t hist[4][SSHOT_MAX_DIM];
    float4 qd[4][128];       // dx, dy, dz, d2 of queued neighbours
    WaveRows rows[4];
};

// Per-neighbour update (:125-140, :159-243). All 64 lanes call it; 'act' marks lanes that hold a neighbour. The steps are those of
// short_common.h: estimate, FP64 re-take where the estimate is not clear of a decision, deposits.
__device__ __forceinline__ void sshot_neighbour(const ShortShotArgs& a, shot_bin_t* hist, int dim, bool act,
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

// 104 VGPRs, no scratch, 20 KiB LDS per workgroup: 4 waves per SIMD (the compiler's resource report; held to 96 it spills 16)
__global__ __launch_bounds__(256, 4) void k_short_shot(ShortShotArgs a) {
    __shared__ ShortShotSmem sm;
    const int D = a.r_bins * a.e_bins * a.a_bins;                       // 1 .. 256 (checked by the launcher)
    const int copies = SSHOT_MAX_DIM / D;
    ShotWave w;
    if (!shot_wave_setup(a, D, w)) return;
    const int wv = w.wv, lane = w.lane;
    float* out = w.row;
    for (int i = lane; i < SSHOT_MAX_DIM; i += 64) sm.hist[wv][i] = 0ull;
    shot_bin_t* hist = sm.hist[wv] + (lane % copies) * D;               // this lane's copy
    shot_wave_neighbours<16, false>(a, w, sm.qd[wv], nullptr, sm.rows[wv],
        [&](bool act, uint32_t, float dx, float dy, float dz, float d2) { sshot_neighbour(a, hist, D, act, dx, dy, dz, d2, w.fx, w.fy, w.fz); });
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");             // the deposits of the other lanes are read below
    // L2 norm (:143-152): double sum of squares, sqrt, double division, cast to float. No contributing neighbour: 0 / 0, a NaN row.
    double v[SSHOT_MAX_DIM / 64];
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < SSHOT_MAX_DIM / 64; ++j) {
        const int i = lane + 64 * j;
        shot_bin_t h = 0ull;
        if (i < D) for (int c = 0; c < copies; ++c) h += sm.hist[wv][c * D + i];
        v[j] = (double)h * SHOT_FIX_INV;
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
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (r_bins < 1 || e_bins < 1 || a_bins < 1) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_shot: fewer than one bin on an axis");
    if ((long long)r_bins * e_bins * a_bins > ISMHIP_SHORT_SHOT_MAX_DIM)
        return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "short_shot: more than 256 bins");
    const ShotCall c{ctx, cloud, kp_offsets_h, kpx, kpy, kpz, nullptr, lrf9, radius, desc_out, neighbour_count_out, "short_shot"};
    ShortShotArgs a;
    uint32_t maxk;
    int rc = shot_check_call(c, sshot_min_radius_ok(min_radius), false);
    if (rc == ISMHIP_OK) rc = sshot_radial_args(c, min_radius, log_radius, a);
    if (rc == ISMHIP_OK) rc = shot_common_args(c, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.r_bins = r_bins; a.e_bins = e_bins; a.a_bins = a_bins;
    a.g = sshot_scale_of(r_bins, e_bins, a_bins, radius);
    return shot_launch(c, a, maxk, k_short_shot, 0);
}

}  // extern "C"
