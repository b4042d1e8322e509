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
// first ESTIMATED in float (sshot_estimate: raw values to a few 1e-7 per bin, bound below); only where an estimate comes within eps of
// a value at which a decision changes -- an integer n >= 1, or n + 0.5 -- does the wave re-take that neighbour in FP64 exactly as
// written in the reference (sqrt and division IEEE-exact; acos, atan2, log from the device's libm, a few ulp of double from the
// host's, ~1e-13 in raw units). Away from the decisions the interpolation shares are continuous, and a raw value off by 1e-6 moves a
// share by 1e-6: far inside the 1e-4 parity tolerance. A logarithmic radius always takes the FP64 sequence.
#include "common.h"

namespace {

struct ShortShotArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    const uint32_t* kp_off; const float *kx, *ky, *kz;
    const float* lrf; float radius, r2;
    double radius_d, min_radius, ln_rmin, ln_rmax_rmin;
    float r_scale, t_scale, p_scale, p_off;    // float estimate: raw_r = r * r_scale, raw_theta = theta * t_scale, raw_phi = phi * p_scale + p_off
    float eps_r, eps_t, eps_p, min_radius_f;   // and how close to a decision it may come before the FP64 sequence decides
    int log_radius, r_bins, e_bins, a_bins;
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;   // keypoints in cell order (nullptr: as they come)
};

#define SSHOT_MAX_DIM   256
#define SSHOT_FIX_SCALE 268435456.0f              /* 2^28: an increment is in [0, 3], so round(v * 2^28) fits 32 bits */
#define SSHOT_FIX_INV   3.7252902984619140625e-09 /* 2^-28 */
#define SSHOT_RAD2DEG   57.29578                  /* pcl::rad2deg(double) of PCL 1.10 multiplies by this truncated constant (external) */
typedef unsigned long long sshot_bin_t;

struct ShortShotSmem {
    // A short histogram draws many lanes of one deposit onto the same address, and same-address LDS atomics of a wave instruction
    // serialise. The 256 slots a wave owns therefore hold 256 / D COPIES of the D bins; lane l deposits into copy l % copies and the
    // copies are summed (integers: exactly) before the norm.
    sshot_bin_t hist[4][SSHOT_MAX_DIM];
    float4 qd[4][128];       // dx, dy, dz, d2 of queued neighbours
    WaveRows rows[4];
};

// linear_interpolation (:246-260): decimals from the UNCLAMPED int; share of the primary bin and the side of the secondary one.
// The reference forms decimals + 0.5 in double and rounds to float: both operands are floats whose sum is exact in double, so the
// float addition rounds the same exact value once.
__device__ __forceinline__ void sshot_interp(float raw, float& f, int& step) {
    const float decimals = raw - (float)(int)raw;
    if (decimals <= 0.5f) { f = decimals + 0.5f; step = -1; }
    else { f = (1.0f - decimals) + 0.5f; step = 1; }
}
__device__ __forceinline__ void sshot_dep(sshot_bin_t* hist, int dim, int bin, float v) {
    if ((unsigned)bin < (unsigned)dim) atomicAdd(&hist[bin], (sshot_bin_t)__float2uint_rn(v * SSHOT_FIX_SCALE));   // the guard never fails on finite frames
}

// true when the float estimate `raw` of a raw bin value is at least eps from every value at which int(raw) or `decimals <= 0.5f`
// changes: the integers n >= 1 (int() truncates towards zero: nothing changes across 0, and no raw value is below -1) and n + 0.5.
// A NaN estimate is not clear.
__device__ __forceinline__ bool sshot_clear(float raw, float eps) {
    const float fl = floorf(raw), d = raw - fl;
    const bool below = fl < 1.f || d >= eps;                 // the integer at or below raw
    const bool above = fl < 0.f || (1.f - d) >= eps;         // the integer above it
    return below && above && fabsf(d - 0.5f) >= eps;
}

// Float estimate of the three raw values of a neighbour with local coordinates (x, y, z); returns false when the FP64 sequence has
// to decide. Error of the estimate, in units of the float epsilon u = 6e-8: r^2 3 roundings and v_sqrt_f32 1 ulp -> r to 3.5 u
// relative, raw_r = r * r_scale to 6 u * r_bins. theta = atan2(sqrt(x^2 + y^2), z) (well conditioned at the poles, unlike acos(z / r)):
// 2 u from its first argument, shot_atan2 itself <= 10 u (v_rcp_f32 1 ulp, the polynomial 2e-8, two subtractions from constants near
// pi), so raw_theta = theta * e_bins * 57.29578 / 180 to 5 u * e_bins; raw_phi likewise to 3 u * a_bins. eps = 2e-6 * (bins + 1) per
// axis is four times that or more. With (2, 2, 8) bins one neighbour in ~8000 is re-taken in FP64.
__device__ __forceinline__ bool sshot_estimate(const ShortShotArgs& a, float x, float y, float z, float& raw_r, float& raw_theta, float& raw_phi,
                                               bool& below_min) {
    const float rho2 = x * x + y * y;
    const float r = __builtin_amdgcn_sqrtf(rho2 + z * z);
    raw_r = r * a.r_scale;
    raw_theta = shot_atan2(__builtin_amdgcn_sqrtf(rho2), z) * a.t_scale;
    raw_phi = __builtin_fmaf(shot_atan2(y, x), a.p_scale, a.p_off);          // x == y == 0: NaN, not clear (the reference's atan2 gives 0)
    below_min = r < a.min_radius_f;
    const bool min_clear = a.min_radius_f == 0.f || fabsf(r - a.min_radius_f) >= r * 2e-6f;
    return !a.log_radius && min_clear && sshot_clear(raw_r, a.eps_r) && sshot_clear(raw_theta, a.eps_t) && sshot_clear(raw_phi, a.eps_p);
}

// The reference's own sequence (:130-137, :166-179) for the neighbours whose estimate is not clear of a decision: the three float raw
// values and, in w, whether r < min_radius. A CALL, not inlined: the three FP64 libm expansions would otherwise set the register
// allocation (167 VGPRs: 3 waves per SIMD) of a kernel that runs them for one neighbour in thousands.
__device__ __noinline__ float4 sshot_exact(float xf, float yf, float zf, double radius_d, double min_radius, double ln_rmin, double ln_rmax_rmin,
                                           int log_radius, int rb, int eb, int ab) {
    const double xl = (double)xf, yl = (double)yf, zl = (double)zf;
    const double r = sqrt((xl * xl + yl * yl) + zl * zl);
    const double theta = acos(zl / r) * SSHOT_RAD2DEG;
    const double phi = atan2(yl, xl) * SSHOT_RAD2DEG;
    const float raw_r = log_radius ? (float)(((double)(rb - 1) * (log(r) - ln_rmin)) / ln_rmax_rmin + 1.0)
                                   : (float)(((double)rb * r) / radius_d);
    return make_float4(raw_r, (float)(((double)eb * theta) / 180.0), (float)(((double)ab * (phi + 180.0)) / 360.0), r < min_radius ? 1.f : 0.f);
}

// Per-neighbour update (:125-140, :159-243). All 64 lanes call it; 'act' marks lanes that hold a neighbour.
__device__ __forceinline__ void sshot_neighbour(const ShortShotArgs& a, sshot_bin_t* hist, int dim, bool act,
                                                float dx, float dy, float dz, float d2,
                                                const float fx[3], const float fy[3], const float fz[3]) {
    if (!act) return;
    if (d2 <= 1e-15f) return;                                                     // distances[j] > 1E-15 on the SQUARED distance (:127)
    const float xf = (dx * fx[0] + dy * fx[1]) + dz * fx[2];                      // float products, unfused, in this order
    const float yf = (dx * fy[0] + dy * fy[1]) + dz * fy[2];
    const float zf = (dx * fz[0] + dy * fz[1]) + dz * fz[2];
    const int rb = a.r_bins, eb = a.e_bins, ab = a.a_bins;
    float raw_r, raw_theta, raw_phi;
    bool below_min;
    if (!sshot_estimate(a, xf, yf, zf, raw_r, raw_theta, raw_phi, below_min)) {
        const float4 e = sshot_exact(xf, yf, zf, a.radius_d, a.min_radius, a.ln_rmin, a.ln_rmax_rmin, a.log_radius, rb, eb, ab);
        raw_r = e.x; raw_theta = e.y; raw_phi = e.z; below_min = e.w != 0.f;
    }
    if (below_min) return;
    int bin_r = (int)raw_r, bin_theta = (int)raw_theta, bin_phi = (int)raw_phi;
    bin_r = bin_r >= 0 ? bin_r : 0;
    bin_r = bin_r < rb ? bin_r : rb - 1;
    bin_theta = bin_theta < eb ? bin_theta : eb - 1;                              // theta and phi: clamped from above only, as written
    bin_phi = bin_phi < ab ? bin_phi : ab - 1;
    float f_r, f_t, f_p; int s_r, s_t, s_p;
    sshot_interp(raw_r, f_r, s_r);
    sshot_interp(raw_theta, f_t, s_t);
    sshot_interp(raw_phi, f_p, s_p);
    // correct_bin (:263-283): r and theta clamp, phi wraps (one step past either end)
    int r2b = bin_r + s_r;         r2b = r2b < 0 ? 0 : (r2b >= rb ? rb - 1 : r2b);
    int t2b = bin_theta + s_t;     t2b = t2b < 0 ? 0 : (t2b >= eb ? eb - 1 : t2b);
    int p2b = bin_phi + s_p;       p2b = p2b < 0 ? ab - 1 : (p2b >= ab ? 0 : p2b);
    const int re = rb * eb;
    sshot_dep(hist, dim, bin_r + bin_theta * rb + bin_phi * re, (f_r + f_t) + f_p);
    if (ab > 1 && p2b != bin_phi)   sshot_dep(hist, dim, bin_r + bin_theta * rb + p2b * re, (f_r + f_t) + (1.0f - f_p));
    if (eb > 1 && t2b != bin_theta) sshot_dep(hist, dim, bin_r + t2b * rb + bin_phi * re, (f_r + (1.0f - f_t)) + f_p);
    if (rb > 1 && r2b != bin_r)     sshot_dep(hist, dim, r2b + bin_theta * rb + bin_phi * re, ((1.0f - f_r) + f_t) + f_p);
}

// 114 VGPRs, no scratch, 20 KiB LDS per workgroup: 4 waves per SIMD (the compiler's resource report; held to 96 it spills 16)
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
    a.r_scale = (float)((double)r_bins / (double)radius);
    a.t_scale = (float)((double)e_bins * SSHOT_RAD2DEG / 180.0);
    a.p_scale = (float)((double)a_bins * SSHOT_RAD2DEG / 360.0); a.p_off = (float)((double)a_bins * 0.5);
    a.eps_r = 2e-6f * (float)(r_bins + 1); a.eps_t = 2e-6f * (float)(e_bins + 1); a.eps_p = 2e-6f * (float)(a_bins + 1);
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
