// shot_deposit.h — the per-neighbour arithmetic of SHOT-352 / CSHOT-1344 (PCL 1.10 computePointSHOT / interpolateSingleChannel /
// interpolateDoubleChannel): one neighbour's deposits into a 2^-28 fixed-point LDS histogram (shot_wave.h).
// Shared by the kernels that build such a row: k_shot (shot.hip, one wave per keypoint) and k_global (global.hip, one workgroup per
// region), so that both take every hard decision in the same instructions.
#pragma once
#include "shot_wave.h"

#define PST_RAD_45f   0.78539816339744830962f
#define PST_RAD_90f   1.57079632679489661923f
#define PST_RAD_135f  2.35619449019234492885f
#define PST_RAD_PI_7_8f 2.7488935718910690836f

#ifdef __HIPCC__
// The interpolation weights are CONTINUOUS in distance / inclination / azimuth (all hard bin decisions are taken on the
// signs and squares above them), so these three only need ~1e-7 absolute accuracy -- far inside the 1e-4 parity tolerance --
// and not libm's last ulp: the IEEE division / sqrt expansions and OCML's acosf / atan2f were a quarter of the kernel's VALU.
// acos: Abramowitz & Stegun 4.4.46 (|err| <= 2e-8 before rounding); atan: A&S 4.4.49 (|err| <= 2e-8), shot_atan2 in common.h.
__device__ __forceinline__ float shot_acos(float x) {
    const float a = fabsf(x);
    float p = -0.0012624911f;
    p = __builtin_fmaf(p, a, 0.0066700901f); p = __builtin_fmaf(p, a, -0.0170881256f); p = __builtin_fmaf(p, a, 0.0308918810f);
    p = __builtin_fmaf(p, a, -0.0501743046f); p = __builtin_fmaf(p, a, 0.0889789874f); p = __builtin_fmaf(p, a, -0.2145988016f);
    p = __builtin_fmaf(p, a, 1.5707963050f);
    const float r = __builtin_amdgcn_sqrtf(fmaxf(1.0f - a, 0.f)) * p;
    return x < 0.f ? 3.14159265358979323846f - r : r;
}
// step = floor(m*x + c) and off = float((m*x + c0) - step) exactly as the reference's double arithmetic yields them, for a float x
// whose product m*x (m = 5 or 30) is exact in double -- true wherever m*x + c can reach an integer. One fma rounds the exact value
// once; floor of the rounded value differs from the true floor only if the rounding went UP onto an integer, which the sign of a
// second fma (the exact residual, rounded) reveals. c0 = c - 0.5: the offset is measured from the bin centre.
__device__ __forceinline__ void shot_hard_bin(float m, float x, float c, float c0, int& step, float& off) {
    const float t = __builtin_fmaf(m, x, c);
    float k = floorf(t);
    if (t == k && __builtin_fmaf(m, x, c - k) < 0.f) k -= 1.f;
    step = (int)k;
    off = __builtin_fmaf(m, x, c0 - k);
}

__device__ __forceinline__ void shot_dep(shot_bin_t* hist, int bin, float v) {
    atomicAdd(&hist[bin], (shot_bin_t)__float2uint_rn(v * SHOT_FIX_SCALE));
}
// the same for a weight held in double (spin_image.hip): round(v * 2^28), at most 2^-29 off
__device__ __forceinline__ void shot_dep(shot_bin_t* hist, int bin, double v) {
    atomicAdd(&hist[bin], (shot_bin_t)__double2ull_rn(v * (double)SHOT_FIX_SCALE));
}

// Per-neighbour SHOT update. All 64 lanes call it; 'act' marks lanes that hold a neighbour. Args: anything with the cell-sorted
// normals sn4 and, for COLOR, the normalised CIELab slab4.
template <bool COLOR, class Args>
__device__ __forceinline__ void shot_neighbour(const Args& a, shot_bin_t* hist, bool act, uint32_t gi,
                                               float dx, float dy, float dz, float d2,
                                               const float fx[3], const float fy[3], const float fz[3],
                                               float r12, float r14, float r34, float inv_r12, float r12sq_f,
                                               float LRef, float aRef, float bRef) {
    if (!act) return;
    const float4 nrm = a.sn4[gi];
    const float nxv = nrm.x, nyv = nrm.y, nzv = nrm.z;
    if (!(isfinite(nxv) && isfinite(nyv) && isfinite(nzv))) return;              // createBinDistanceShape: NaN normal -> skipped
    float cosd = (nxv * fz[0] + nyv * fz[1]) + nzv * fz[2];
    cosd = fminf(1.0f, fmaxf(-1.0f, cosd));
    // PCL's interpolation is only partly soft: the whole accumulated weight lands in the HARD-assigned (sector, step) bin, so
    // every hard decision must be taken exactly as the reference takes it. The reference computes the cosine bin in double from
    // the float cosine (createBinDistanceShape) and compares the radial shell on squares in double; both are reproduced below
    // without FP64 instructions (shot_hard_bin, r12sq_f).
    const float dist = __builtin_amdgcn_sqrtf(d2);
    if (dist < 1e-15f) return;                                                    // areEquals(distance, 0)
    float xl = (dx * fx[0] + dy * fx[1]) + dz * fx[2];
    float yl = (dx * fy[0] + dy * fy[1]) + dz * fy[2];
    float zl = (dx * fz[0] + dy * fz[1]) + dz * fz[2];
    if (fabsf(yl) < 1e-30f) yl = 0.f;
    if (fabsf(xl) < 1e-30f) xl = 0.f;
    if (fabsf(zl) < 1e-30f) zl = 0.f;
    const int bit4 = ((yl > 0.f) || ((yl == 0.f) && (xl < 0.f))) ? 1 : 0;
    const int bit3 = ((xl > 0.f) || ((xl == 0.f) && (yl > 0.f))) ? !bit4 : bit4;
    int di = ((bit4 << 3) + (bit3 << 2)) << 1;
    const bool same_sign = (xl > 0.f && yl > 0.f) || (xl < 0.f && yl < 0.f);      // x*y > 0 without float underflow
    if (same_sign || xl == 0.f) di += (fabsf(xl) >= fabsf(yl)) ? 0 : 4;
    else di += (fabsf(xl) > fabsf(yl)) ? 4 : 0;
    di += zl > 0.f ? 1 : 0;
    const bool outer = d2 > r12sq_f;                                              // distance > radius1_2: (double)d2 > r^2/4 in double == d2 > largest float <= r^2/4
    di += outer ? 2 : 0;

    int step; float bd;
    shot_hard_bin(5.f, cosd, 5.5f, 5.f, step, bd);                                // bin = floor(((1 + cos) * 10) / 2 + 0.5), bd = offset from its centre
    const int vol = di * 11;
    float w_shape = 1.f - fabsf(bd);
    // Everything below is branch-free: each of the four interpolation directions yields ONE (neighbouring bin, weight) pair
    // chosen by selects -- written as the reference's if/else ladders it compiled into eight divergent deposit sites with
    // partial exec masks and their branch overhead. The float operations (and so the results) are the same: in the "deposit"
    // case of every ladder the reference adds 1 -/+ t with t of the sign that makes it 1 - |t|, and deposits |t|.
    {
        int t = bd > 0.f ? step + 1 : step + 9;                                   // (step + 1) % 10 | (step - 1 + 10) % 10, step in 0..10
        t = t >= 10 ? t - 10 : t;
        shot_dep(hist, vol + t, fabsf(bd));
    }
    int step_c = 0, vol_c = 0; float w_col = 0.f;
    if (COLOR) {
        const float4 lab = a.slab4[gi];
        const float L = lab.x, A = lab.y, B = lab.z;
        float cd = (fabsf(LRef - L) + ((fabsf(aRef - A) + fabsf(bRef - B)) * 0.5f)) / 3.0f;   // feeds a hard bin: exact division
        cd = fminf(1.0f, fmaxf(0.0f, cd));
        float bc;
        shot_hard_bin(30.f, cd, 0.5f, 0.f, step_c, bc);                           // colorDistance (float) * nr_color_bins_, taken in double by the reference
        vol_c = 352 + di * 31;
        w_col = 1.f - fabsf(bc);
        int t = bc > 0.f ? step_c + 1 : step_c + 29;                              // % 30
        t = t >= 30 ? t - 30 : t;
        shot_dep(hist, vol_c + t, fabsf(bc));
    }
    float winc = 0.f;
    // radial: outer shell interpolates towards the inner one below 3r/4, inner shell towards the outer one above r/4
    const float xr = outer ? (dist - r34) * inv_r12 : -((dist - r14) * inv_r12);
    const float wr_ = xr > 0.f ? 0.f : fabsf(xr);
    winc += 1.f - fabsf(xr);
    const int sec_r = outer ? di - 2 : di + 2;
    // elevation
    float ic = zl * __builtin_amdgcn_rcpf(dist);
    ic = fminf(1.0f, fmaxf(-1.0f, ic));
    const float inc = shot_acos(ic);
    const bool lower = !(zl > 0.f);   // inclination > 90 deg, or exactly 90 deg with z <= 0: the same test that picked the sector's elevation bit
    const float ide = (inc - (lower ? PST_RAD_135f : PST_RAD_45f)) * (1.0f / PST_RAD_90f);
    const float xe = lower ? ide : -ide;
    const float we = xe > 0.f ? 0.f : fabsf(xe);
    winc += 1.f - fabsf(xe);
    const int sec_e = lower ? di + 1 : di - 1;
    // azimuth
    float wa = 0.f; int sec_a = di;
    if (yl != 0.f || xl != 0.f) {
        const float az = shot_atan2(yl, xl);
        const int sel = di >> 2;
        float ad = (az - (-PST_RAD_PI_7_8f + PST_RAD_45f * (float)sel)) * (1.0f / PST_RAD_45f);
        ad = fmaxf(-0.5f, fminf(ad, 0.5f));
        wa = fabsf(ad);
        winc += 1.f - wa;
        sec_a = (ad > 0.f ? di + 4 : di - 4) & 31;
    }
    // deposits only where there is a weight: unconditional ones measured SLOWER (4.44 vs 4.06 ms: more lanes in every atomic = more
    // same-address serialisation)
    if (wr_ != 0.f) { shot_dep(hist, sec_r * 11 + step, wr_); if (COLOR) shot_dep(hist, 352 + sec_r * 31 + step_c, wr_); }
    if (we != 0.f) { shot_dep(hist, sec_e * 11 + step, we); if (COLOR) shot_dep(hist, 352 + sec_e * 31 + step_c, we); }
    if (wa != 0.f) { shot_dep(hist, sec_a * 11 + step, wa); if (COLOR) shot_dep(hist, 352 + sec_a * 31 + step_c, wa); }
    shot_dep(hist, vol + step, w_shape + winc);
    if (COLOR) shot_dep(hist, vol_c + step_c, w_col + winc);
}
#endif

// largest float <= (radius / 2)^2 taken in double: the shell test (double)d2 > r12sq of the reference, as a float compare
static __host__ __device__ inline float shot_r12sq_f(float radius) {
    const double t = 0.25 * (double)radius * (double)radius;
    float tf = (float)t;
    if ((double)tf > t) tf = nextafterf(tf, -INFINITY);
    return tf;
}
