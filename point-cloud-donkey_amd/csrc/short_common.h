// short_common.h — the steps that the reference's two Short SHOT descriptors share (short_shot.hip: SHORT_SHOT; short_cshot.hip:
// SHORT_CSHOT, whose shape part is the same text and whose colour part runs the same steps on a second spherical grid): the
// interpolation share of a raw bin value, the exact fixed-point deposit, the float estimate of a neighbour's raw values with the test
// that decides whether it may stand, the FP64 re-take of the reference's own sequence, and the three-axis deposits of the shape part.
#pragma once
#include "shot_wave.h"

#define SSHOT_RAD2DEG   57.29578                  /* pcl::rad2deg(double) of PCL 1.10 multiplies by this truncated constant (external) */

// One spherical grid as the float estimate sees it: raw_r = r * r_scale, raw_theta = theta * t_scale, raw_phi = phi * p_scale + p_off,
// and how close to a decision each may come before the FP64 sequence decides
struct SshotScale { float r_scale, t_scale, p_scale, p_off, eps_r, eps_t, eps_p; };
static inline SshotScale sshot_scale_of(int r_bins, int e_bins, int a_bins, float radius) {
    SshotScale g;
    g.r_scale = (float)((double)r_bins / (double)radius);
    g.t_scale = (float)((double)e_bins * SSHOT_RAD2DEG / 180.0);
    g.p_scale = (float)((double)a_bins * SSHOT_RAD2DEG / 360.0); g.p_off = (float)((double)a_bins * 0.5);
    g.eps_r = 2e-6f * (float)(r_bins + 1); g.eps_t = 2e-6f * (float)(e_bins + 1); g.eps_p = 2e-6f * (float)(a_bins + 1);
    return g;
}

// The radial parameters of both entry points. A min_radius that is negative or not finite is a bad argument (sshot_min_radius_ok, for
// shot_check_call); with a logarithmic radius the reference divides by log(Radius / min_radius): 0 for min_radius == 0 (and NaN -> int);
// refused, never altered.
static inline bool sshot_min_radius_ok(float min_radius) { return min_radius >= 0.f && std::isfinite(min_radius); }
template <class Args>
int sshot_radial_args(const ShotCall& c, float min_radius, int log_radius, Args& a) {
    if (log_radius && !(min_radius > 0.f && min_radius < c.radius))
        return ism_set_err(c.ctx, ISMHIP_ERR_INVALID, std::string(c.name) + ": logarithmic radius needs 0 < min_radius < radius");
    a.radius_d = (double)c.radius; a.min_radius = (double)min_radius;
    a.ln_rmin = min_radius == 0.f ? 0.0 : log((double)min_radius);
    a.ln_rmax_rmin = min_radius == 0.f ? 0.0 : log((double)c.radius / (double)min_radius);
    a.min_radius_f = min_radius;
    a.log_radius = log_radius ? 1 : 0;
    return ISMHIP_OK;
}

#ifdef __HIPCC__
// linear_interpolation (:246-260): decimals from the UNCLAMPED int; share of the primary bin and the side of the secondary one.
// The reference forms decimals + 0.5 in double and rounds to float: both operands are floats whose sum is exact in double, so the
// float addition rounds the same exact value once.
__device__ __forceinline__ void sshot_interp(float raw, float& f, int& step) {
    const float decimals = raw - (float)(int)raw;
    if (decimals <= 0.5f) { f = decimals + 0.5f; step = -1; }
    else { f = (1.0f - decimals) + 0.5f; step = 1; }
}
__device__ __forceinline__ void sshot_dep(shot_bin_t* hist, int dim, int bin, float v) {
    if ((unsigned)bin < (unsigned)dim) atomicAdd(&hist[bin], (shot_bin_t)__float2uint_rn(v * SHOT_FIX_SCALE));   // the guard never fails on finite frames
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

// Float estimate of a neighbour with local coordinates (x, y, z): r, theta and phi (radians), then the three raw values on one grid.
// Error of the estimate, in units of the float epsilon u = 6e-8: r^2 3 roundings and v_sqrt_f32 1 ulp -> r to 3.5 u
// relative, raw_r = r * r_scale to 6 u * r_bins. theta = atan2(sqrt(x^2 + y^2), z) (well conditioned at the poles, unlike acos(z / r)):
// 2 u from its first argument, shot_atan2 itself <= 10 u (v_rcp_f32 1 ulp, the polynomial 2e-8, two subtractions from constants near
// pi), so raw_theta = theta * e_bins * 57.29578 / 180 to 5 u * e_bins; raw_phi likewise to 3 u * a_bins. eps = 2e-6 * (bins + 1) per
// axis is four times that or more. With (2, 2, 8) bins one neighbour in ~8000 is re-taken in FP64.
__device__ __forceinline__ void sshot_polar(float x, float y, float z, float& r, float& theta, float& phi) {
    const float rho2 = x * x + y * y;
    r = __builtin_amdgcn_sqrtf(rho2 + z * z);
    theta = shot_atan2(__builtin_amdgcn_sqrtf(rho2), z);
    phi = shot_atan2(y, x);                                                    // x == y == 0: NaN, not clear (the reference's atan2 gives 0)
}
// the raw values of (r, theta, phi) on grid g; false when one of them is not clear of a decision
__device__ __forceinline__ bool sshot_scaled(const SshotScale& g, float r, float theta, float phi, float& raw_r, float& raw_theta, float& raw_phi) {
    raw_r = r * g.r_scale;
    raw_theta = theta * g.t_scale;
    raw_phi = __builtin_fmaf(phi, g.p_scale, g.p_off);
    return sshot_clear(raw_r, g.eps_r) && sshot_clear(raw_theta, g.eps_t) && sshot_clear(raw_phi, g.eps_p);
}
// r < min_radius on the estimate, and whether the estimate may decide it
__device__ __forceinline__ bool sshot_min_clear(float r, float min_radius_f, bool& below_min) {
    below_min = r < min_radius_f;
    return min_radius_f == 0.f || fabsf(r - min_radius_f) >= r * 2e-6f;
}

// The reference's own sequence (:130-137, :166-179) for the neighbours whose estimate is not clear of a decision: the three float raw
// values and, in w, whether r < min_radius. A CALL, not inlined: the three FP64 libm expansions would otherwise set the register
// allocation (167 VGPRs: 3 waves per SIMD) of a kernel that runs them for one neighbour in thousands.
static __device__ __noinline__ float4 sshot_exact(float xf, float yf, float zf, double radius_d, double min_radius, double ln_rmin, double ln_rmax_rmin,
                                           int log_radius, int rb, int eb, int ab) {
    const double xl = (double)xf, yl = (double)yf, zl = (double)zf;
    const double r = sqrt((xl * xl + yl * yl) + zl * zl);
    const double theta = acos(zl / r) * SSHOT_RAD2DEG;
    const double phi = atan2(yl, xl) * SSHOT_RAD2DEG;
    const float raw_r = log_radius ? (float)(((double)(rb - 1) * (log(r) - ln_rmin)) / ln_rmax_rmin + 1.0)
                                   : (float)(((double)rb * r) / radius_d);
    return make_float4(raw_r, (float)(((double)eb * theta) / 180.0), (float)(((double)ab * (phi + 180.0)) / 360.0), r < min_radius ? 1.f : 0.f);
}

// One axis of a grid: the primary bin of a raw value (r clamps to both ends, the others from above only, as written), its share,
// and the secondary bin after correct_bin (:263-283: clamps, or wraps one step past either end for phi)
struct SshotAxis { int bin, bin2; float f; };
template <bool CLAMP_LOW, bool CYCLIC>
__device__ __forceinline__ SshotAxis sshot_axis(float raw, int n) {
    SshotAxis x;
    int b = (int)raw, s;
    if (CLAMP_LOW) b = b >= 0 ? b : 0;
    b = b < n ? b : n - 1;
    sshot_interp(raw, x.f, s);
    const int b2 = b + s;
    x.bin = b;
    x.bin2 = CYCLIC ? (b2 < 0 ? n - 1 : (b2 >= n ? 0 : b2)) : (b2 < 0 ? 0 : (b2 >= n ? n - 1 : b2));
    return x;
}

// compute_shape_descriptor (:159-243) from the three float raw values on: up to four deposits into hist[0 .. dim)
__device__ __forceinline__ void sshot_shape_deposits(shot_bin_t* hist, int dim, int rb, int eb, int ab, float raw_r, float raw_theta, float raw_phi) {
    const SshotAxis r = sshot_axis<true, false>(raw_r, rb), t = sshot_axis<false, false>(raw_theta, eb), p = sshot_axis<false, true>(raw_phi, ab);
    const int re = rb * eb;
    sshot_dep(hist, dim, r.bin + t.bin * rb + p.bin * re, (r.f + t.f) + p.f);
    if (ab > 1 && p.bin2 != p.bin) sshot_dep(hist, dim, r.bin + t.bin * rb + p.bin2 * re, (r.f + t.f) + (1.0f - p.f));
    if (eb > 1 && t.bin2 != t.bin) sshot_dep(hist, dim, r.bin + t.bin2 * rb + p.bin * re, (r.f + (1.0f - t.f)) + p.f);
    if (rb > 1 && r.bin2 != r.bin) sshot_dep(hist, dim, r.bin2 + t.bin * rb + p.bin * re, ((1.0f - r.f) + t.f) + p.f);
}
#endif
