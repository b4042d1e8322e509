// short_cshot.hip — the Short SHOT with its colour histogram (Features type "SHORT_CSHOT"), one 64-lane wavefront per keypoint.
// Reference seam: FeaturesSHORTCSHOT::compute_descriptor / compute_shape_descriptor / compute_color_descriptor / linear_interpolation /
// correct_bin (features/features_short_cshot.cpp:103-507). The row is the SHORT_SHOT histogram of Ds = r e a bins on the shape grid,
// followed by Dc H bins: a histogram of H colour-distance bins in every cell of a SECOND spherical grid of Dc = rc ec ac cells; the
// two parts are L2-normalised together. A neighbour therefore takes two independent sets of hard decisions on its raw r / theta / phi
// values (one per grid) and one on raw_c = colour distance * H.
//
// Gather model: algorithmic bytes per keypoint = M_k * 32 + 12 + 36 + 4 + 4 * D (M_k = radius neighbours, D = Ds + Dc H <= 1344): the
// 16-byte point record of k_short_shot plus the neighbour's 16-byte normalised CIELab record (slab4, gathered by the queued index as
// k_shot<true> does), the keypoint, its frame and colour, the row.
//
// Structure per wave: that of the SHOT family (shot_wave.h: set-up, ball_for_each<16, true> over sp4, the ballot-compacted queue with
// the neighbours' indices, full waves of neighbours); the steps a neighbour takes are those of short_common.h, their deposits 2^-28
// fixed-point ds_add_u64. The geometry is ESTIMATED once in float (r, theta, phi) and scaled per grid; where a raw value of EITHER grid
// comes within eps of a decision the reference's FP64 sequence is taken for both. The colour side needs no estimate: float subtractions, fabsf, one
// multiplication by 0.5, two additions, an IEEE division by 3, the clamp and the product with (float)H are each exactly the
// reference's operation (the product is the reference's double product rounded once: a 24-bit by <= 11-bit product is exact in double).
// Deviation: the colour distance is taken in float as in PCL's cshot.hpp, from which the reference says it copied the
// block, and as in k_shot<true>; the reference's unqualified fabs does not pin float against double.
//
// Increments: every share is a float in [0.5, 1] (a hair below 0.5 only for phi = -180 degrees) and a multiple of 2^-24, so a sum of
// four is exact in float whatever the order, lies in [1, 4], and round(v * 2^28) <= 2^30 fits 32 bits. The secondary COLOUR bin
// receives (1 - f_c) + (1 - f_r) + f_theta + f_phi exactly as the reference writes it (:424) -- with 1 - f_r, not f_r: bug-compatible.
//
// The per-wave histogram lives in dynamic LDS, sized by the launch (D 64-bit slots per wave): 30 KiB per workgroup at the default 512
// bins (5 workgroups per CU by LDS), 56 KiB at the 1344 cap (2 per CU). No histogram copies for short rows: the default row spreads a
// wave's deposits over 15 colour bins per cell already.
#include "short_common.h"

namespace {

struct ShortCshotArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *slab4;
    const uint32_t* kp_off; const float *kx, *ky, *kz; const uint32_t* kp_rgba;
    const float* lrf; float radius, r2;
    double radius_d, min_radius, ln_rmin, ln_rmax_rmin;
    SshotScale gs, gc;                         // the float estimate's scales and eps on the shape grid and on the colour grid
    float min_radius_f, hist_size_f;
    int log_radius, r_bins, e_bins, a_bins, rc_bins, ec_bins, ac_bins, hist_size, same_grid;
    const float *lut_srgb, *lut_sxyz;
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;   // keypoints in cell order (nullptr: as they come)
};

struct ShortCshotSmem {
    float4 qd[4][128];       // dx, dy, dz, d2 of queued neighbours
    uint32_t qi[4][128];     // sorted index of queued neighbours (their Lab record is gathered when they are processed)
    WaveRows rows[4];
};

// compute_color_descriptor (:312-429) from the float raw values on: up to five deposits into hist[ds .. dim)
__device__ __forceinline__ void scshot_color_deposits(shot_bin_t* hist, int dim, int ds, int rb, int eb, int ab, int hs,
                                                      float raw_r, float raw_theta, float raw_phi, float raw_c) {
    const SshotAxis r = sshot_axis<true, false>(raw_r, rb), t = sshot_axis<false, false>(raw_theta, eb), p = sshot_axis<false, true>(raw_phi, ab);
    const SshotAxis c = sshot_axis<false, false>(raw_c, hs);
    const int hr = hs * rb, hre = hr * eb;
    hist += ds; dim -= ds;
    sshot_dep(hist, dim, c.bin + r.bin * hs + t.bin * hr + p.bin * hre, ((c.f + r.f) + t.f) + p.f);
    if (ab > 1 && p.bin2 != p.bin) sshot_dep(hist, dim, c.bin + r.bin * hs + t.bin * hr + p.bin2 * hre, ((c.f + r.f) + t.f) + (1.0f - p.f));
    if (eb > 1 && t.bin2 != t.bin) sshot_dep(hist, dim, c.bin + r.bin * hs + t.bin2 * hr + p.bin * hre, ((c.f + r.f) + (1.0f - t.f)) + p.f);
    if (rb > 1 && r.bin2 != r.bin) sshot_dep(hist, dim, c.bin + r.bin2 * hs + t.bin * hr + p.bin * hre, ((c.f + (1.0f - r.f)) + t.f) + p.f);
    if (hs > 1 && c.bin2 != c.bin) sshot_dep(hist, dim, c.bin2 + r.bin * hs + t.bin * hr + p.bin * hre, (((1.0f - c.f) + (1.0f - r.f)) + t.f) + p.f);   // :424 as written
}

// Per-neighbour update (:167-202). All 64 lanes call it; 'act' marks lanes that hold a neighbour, gi its sorted point index.
__device__ __forceinline__ void scshot_neighbour(const ShortCshotArgs& a, shot_bin_t* hist, int dim, int ds, bool act, uint32_t gi,
                                                 float dx, float dy, float dz, float d2,
                                                 const float fx[3], const float fy[3], const float fz[3], float LRef, float aRef, float bRef) {
    if (!act) return;
    if (d2 <= 1e-15f) return;                                                     // distances[j] > 1E-15 on the SQUARED distance (:169)
    const float4 lab = a.slab4[gi];
    const float xf = (dx * fx[0] + dy * fx[1]) + dz * fx[2];                      // float products, unfused, in this order
    const float yf = (dx * fy[0] + dy * fy[1]) + dz * fy[2];
    const float zf = (dx * fz[0] + dy * fz[1]) + dz * fz[2];
    float r, theta, phi, sr, st, sp, cr, ct, cp;
    bool below_min;
    sshot_polar(xf, yf, zf, r, theta, phi);
    const bool s_clear = sshot_scaled(a.gs, r, theta, phi, sr, st, sp);
    const bool c_clear = sshot_scaled(a.gc, r, theta, phi, cr, ct, cp);
    const bool min_clear = sshot_min_clear(r, a.min_radius_f, below_min);
    if (a.log_radius || !min_clear || !s_clear || !c_clear) {
        const float4 e = sshot_exact(xf, yf, zf, a.radius_d, a.min_radius, a.ln_rmin, a.ln_rmax_rmin, a.log_radius, a.r_bins, a.e_bins, a.a_bins);
        sr = e.x; st = e.y; sp = e.z; below_min = e.w != 0.f;
        cr = sr; ct = st; cp = sp;
        if (!a.same_grid) {
            const float4 g = sshot_exact(xf, yf, zf, a.radius_d, a.min_radius, a.ln_rmin, a.ln_rmax_rmin, a.log_radius, a.rc_bins, a.ec_bins, a.ac_bins);
            cr = g.x; ct = g.y; cp = g.z;
        }
    }
    if (below_min) return;
    sshot_shape_deposits(hist, ds, a.r_bins, a.e_bins, a.a_bins, sr, st, sp);
    float cd = (fabsf(LRef - lab.x) + ((fabsf(aRef - lab.y) + fabsf(bRef - lab.z)) * 0.5f)) / 3.0f;   // feeds a hard bin: exact division (:194)
    cd = fminf(1.0f, fmaxf(0.0f, cd));
    scshot_color_deposits(hist, dim, ds, a.rc_bins, a.ec_bins, a.ac_bins, a.hist_size, cr, ct, cp, cd * a.hist_size_f);
}

// 121 VGPRs (scalar registers kept in vector-register lanes), no scratch, 14 KiB static + 32 D bytes dynamic LDS per workgroup: 4 waves
// per SIMD by registers (the compiler's resource report)
__global__ __launch_bounds__(256, 4) void k_short_cshot(ShortCshotArgs a) {
    __shared__ ShortCshotSmem sm;
    extern __shared__ shot_bin_t scshot_hist[];                        // [4][D]
    const int Ds = a.r_bins * a.e_bins * a.a_bins;                      // 1 .. 256
    const int D = Ds + a.rc_bins * a.ec_bins * a.ac_bins * a.hist_size; // .. 1344 (both checked by the launcher, which sizes the LDS by D)
    ShotWave w;
    if (!shot_wave_setup(a, D, w)) return;
    const int wv = w.wv, lane = w.lane;
    float* out = w.row;
    shot_bin_t* hist = scshot_hist + (size_t)wv * D;
    for (int i = lane; i < D; i += 64) hist[i] = 0ull;
    float LRef, aRef, bRef;
    rgb2lab_norm(a.lut_srgb, a.lut_sxyz, a.kp_rgba[w.k], LRef, aRef, bRef);   // the keypoint's own colour is the reference colour (:148-155)
    shot_wave_neighbours<16, true>(a, w, sm.qd[wv], sm.qi[wv], sm.rows[wv],
        [&](bool act, uint32_t gi, float dx, float dy, float dz, float d2) {
            scshot_neighbour(a, hist, D, Ds, act, gi, dx, dy, dz, d2, w.fx, w.fy, w.fz, LRef, aRef, bRef);
        });
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");             // the deposits of the other lanes are read below
    // L2 norm of the fused row (:204-220): double sum of squares, sqrt, double division, cast to float. No contributing neighbour:
    // 0 / 0, a NaN row. The bins are integers: reading them twice gives the same values.
    double acc = 0.0;
    for (int i = lane; i < D; i += 64) { const double v = (double)hist[i] * SHOT_FIX_INV; acc += v * v; }
    const double norm = sqrt(wave_sum_d(acc));
    for (int i = lane; i < D; i += 64) out[i] = (float)(((double)hist[i] * SHOT_FIX_INV) / norm);
}

}  // namespace

extern "C" {

int ismhip_short_cshot(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                       const float* kpx, const float* kpy, const float* kpz, const uint32_t* kp_rgba, const float* lrf9,
                       float radius, float min_radius, int log_radius, int r_bins, int e_bins, int a_bins,
                       int rc_bins, int ec_bins, int ac_bins, int hist_size, float* desc_out, uint32_t* neighbour_count_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (r_bins < 1 || e_bins < 1 || a_bins < 1 || rc_bins < 1 || ec_bins < 1 || ac_bins < 1)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_cshot: fewer than one bin on an axis");
    if (hist_size < 1) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_cshot: colour histogram of fewer than one bin");
    const long long ds = (long long)r_bins * e_bins * a_bins;
    if (ds > ISMHIP_SHORT_SHOT_MAX_DIM) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "short_cshot: more than 256 shape bins");
    // a factor at a time, stopping above the cap: the product of four ints cannot overflow
    long long dc = (long long)rc_bins * ec_bins;
    if (dc <= ISMHIP_SHORT_CSHOT_MAX_DIM) dc *= ac_bins;
    if (dc <= ISMHIP_SHORT_CSHOT_MAX_DIM) dc *= hist_size;
    if (ds + dc > ISMHIP_SHORT_CSHOT_MAX_DIM) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "short_cshot: row longer than 1344 bins");
    const ShotCall c{ctx, cloud, kp_offsets_h, kpx, kpy, kpz, kp_rgba, lrf9, radius, desc_out, neighbour_count_out, "short_cshot"};
    ShortCshotArgs a;
    uint32_t maxk;
    int rc = shot_check_call(c, sshot_min_radius_ok(min_radius), true);
    if (rc == ISMHIP_OK) rc = sshot_radial_args(c, min_radius, log_radius, a);
    if (rc == ISMHIP_OK) rc = shot_common_args(c, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.slab4 = cloud->slab4; a.kp_rgba = kp_rgba;
    a.r_bins = r_bins; a.e_bins = e_bins; a.a_bins = a_bins;
    a.rc_bins = rc_bins; a.ec_bins = ec_bins; a.ac_bins = ac_bins; a.hist_size = hist_size; a.hist_size_f = (float)hist_size;
    a.same_grid = (r_bins == rc_bins && e_bins == ec_bins && a_bins == ac_bins) ? 1 : 0;
    a.gs = sshot_scale_of(r_bins, e_bins, a_bins, radius);
    a.gc = sshot_scale_of(rc_bins, ec_bins, ac_bins, radius);
    a.lut_srgb = ctx->lut_srgb; a.lut_sxyz = ctx->lut_sxyz;
    const size_t lds = (size_t)4 * (size_t)(ds + dc) * sizeof(shot_bin_t);          // <= 43 008 bytes: with the 14 KiB static part inside the 64 KiB default
    return shot_launch(c, a, maxk, k_short_cshot, lds);
}

}  // extern "C"
