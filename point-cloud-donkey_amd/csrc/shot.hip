// shot.hip — SHOT-352 and CSHOT-1344 descriptors, one 64-lane wavefront per keypoint.
// Reference seams: FeaturesSHOT::iComputeDescriptors (features/features_shot.cpp:28-81) ->
// pcl::SHOTEstimationOMP<..., SHOT352>; FeaturesCSHOT::iComputeDescriptors (features/features_cshot.cpp:28-103)
// -> pcl::SHOTColorEstimationOMP<..., SHOT1344>. Arithmetic restated from PCL 1.10 computePointSHOT /
// interpolateSingleChannel / interpolateDoubleChannel / normalizeHistogram.
//
// Roofline: HBM-bound gather. Algorithmic bytes per keypoint = M_k * 24 + 12 + 36 + 352*4 (SHOT) or
// M_k * 28 + 12 + 36 + 4 + 1344*4 (CSHOT), M_k = radius neighbours.
//
// Structure per wave: set-up and the neighbour queue are those of the whole family (shot_wave.h: the candidate x-runs of the query
// ball in 16 interleaved segments, the lanes inside the ball compacted into an LDS queue, the per-neighbour math on full waves);
// here are the per-neighbour math (shot_neighbour), its deposits into a per-wave LDS histogram (64-bit fixed point, ds_add_u64 --
// see shot_wave.h) and the L2 normalisation of the row, written with coalesced stores.
#include "shot_wave.h"

namespace {

#define PST_RAD_45f   0.78539816339744830962f
#define PST_RAD_90f   1.57079632679489661923f
#define PST_RAD_135f  2.35619449019234492885f
#define PST_RAD_PI_7_8f 2.7488935718910690836f

struct ShotArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *sn4, *slab4;
    const uint32_t* kp_off; const float *kx, *ky, *kz; const uint32_t* kp_rgba;
    const float* lrf; float radius, r2, r12sq_f;
    const float *lut_srgb, *lut_sxyz;
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;   // keypoints in cell order (nullptr: as they come)
};

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

template <bool COLOR>
struct ShotSmem {
    static constexpr int D = COLOR ? 1344 : 352;
    shot_bin_t hist[4][D];
    float4 qd[4][128];       // dx, dy, dz, d2 of queued neighbours
    uint32_t qi[4][128];     // sorted index of queued neighbours
    WaveRows rows[4];
};
__device__ __forceinline__ void shot_dep(shot_bin_t* hist, int bin, float v) {
    atomicAdd(&hist[bin], (shot_bin_t)__float2uint_rn(v * SHOT_FIX_SCALE));
}

// Per-neighbour SHOT update. All 64 lanes call it; 'act' marks lanes that hold a neighbour.
template <bool COLOR>
__device__ __forceinline__ void shot_neighbour(const ShotArgs& a, shot_bin_t* hist, bool act, uint32_t gi,
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

// 6 workgroups (24 waves) per CU: the LDS budget (24.5 KB per workgroup) allows it, so the register allocation must too (<= 80)
template <bool COLOR, int VAR>
__global__ __launch_bounds__(256, COLOR ? 2 : 6) void k_shot(ShotArgs a) {
    constexpr int D = COLOR ? 1344 : 352;
    __shared__ ShotSmem<COLOR> sm;
    ShotWave w;
    if (!shot_wave_setup(a, D, w)) return;
    const int lane = w.lane;
    shot_bin_t* hist = sm.hist[w.wv];
    float* out = w.row;
    for (int i = lane; i < D; i += 64) hist[i] = 0ull;
    float LRef = 0.f, aRef = 0.f, bRef = 0.f;
    if (COLOR) rgb2lab_norm(a.lut_srgb, a.lut_sxyz, a.kp_rgba[w.k], LRef, aRef, bRef);
    const float r12 = a.radius * 0.5f, r14 = a.radius * 0.25f, r34 = (a.radius * 3.0f) * 0.25f, inv_r12 = 1.0f / r12;
    const float r12sq_f = a.r12sq_f;
    // 16 interleaved segments: measured 4.18 (contiguous) -> 3.27 (8 segments) -> 2.96 ms (16 interleaved) per 256 objects; 32 lose to coalescing
    const uint32_t total = shot_wave_neighbours<(VAR & 2) ? 1 : 16, true>(a, w, sm.qd[w.wv], sm.qi[w.wv], sm.rows[w.wv],
        [&](bool act, uint32_t gi, float dx, float dy, float dz, float d2) {
            shot_neighbour<COLOR>(a, hist, act, gi, dx, dy, dz, d2, w.fx, w.fy, w.fz, r12, r14, r34, inv_r12, r12sq_f, LRef, aRef, bRef);
        });
    if (total < 5) {                                    // computePointSHOT: fewer than 5 neighbours -> NaN descriptor
        for (int i = lane; i < D; i += 64) out[i] = __builtin_nanf("");
        return;
    }
    // normalizeHistogram: double accumulate of float squares, divide by float(norm)
    double acc = 0.0;
    for (int i = lane; i < D; i += 64) { const float v = (float)((double)hist[i] * SHOT_FIX_INV); acc += (double)(v * v); }
    acc = wave_sum_d(acc);
    const float fn = (float)sqrt(acc);
    for (int i = lane; i < D; i += 64) out[i] = (float)((double)hist[i] * SHOT_FIX_INV) / fn;
}

template <bool COLOR>
int launch_shot(const ShotCall& c) {
    int rc = shot_check_call(c, true, COLOR);
    if (rc != ISMHIP_OK) return rc;
    ShotArgs a;
    uint32_t maxk;
    rc = shot_common_args(c, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.sn4 = c.cloud->sn4; a.slab4 = c.cloud->slab4; a.kp_rgba = c.kp_rgba;
    {   // largest float <= (radius/2)^2 taken in double: the shell test (double)d2 > r12sq of the reference, as a float compare
        const double t = 0.25 * (double)c.radius * (double)c.radius;
        float tf = (float)t;
        if ((double)tf > t) tf = nextafterf(tf, -INFINITY);
        a.r12sq_f = tf;
    }
    a.lut_srgb = c.ctx->lut_srgb; a.lut_sxyz = c.ctx->lut_sxyz;
    // ISMHIP_SHOT_VAR=2: the contiguous sweep (A/B runs)
    return shot_launch(c, a, maxk, (c.ctx->shot_var & 2) ? k_shot<COLOR, 2> : k_shot<COLOR, 0>, 0);
}

}  // namespace

extern "C" {

int ismhip_shot352(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                   const float* kpx, const float* kpy, const float* kpz,
                   const float* lrf9, float radius, float* desc_out, uint32_t* neighbour_count_out) {
    return launch_shot<false>({ctx, cloud, kp_offsets_h, kpx, kpy, kpz, nullptr, lrf9, radius, desc_out, neighbour_count_out, "shot352"});
}

int ismhip_cshot1344(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                     const float* kpx, const float* kpy, const float* kpz, const uint32_t* kp_rgba,
                     const float* lrf9, float radius, float* desc_out, uint32_t* neighbour_count_out) {
    return launch_shot<true>({ctx, cloud, kp_offsets_h, kpx, kpy, kpz, kp_rgba, lrf9, radius, desc_out, neighbour_count_out, "cshot1344"});
}

}  // extern "C"
