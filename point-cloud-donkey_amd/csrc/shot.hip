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
// the per-neighbour math (shot_neighbour) and its deposits into a per-wave LDS histogram (64-bit fixed point, ds_add_u64 --
// see shot_wave.h) are in shot_deposit.h, which global.hip shares; here is the L2 normalisation of the row, written with coalesced stores.
#include "shot_deposit.h"

namespace {

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

template <bool COLOR>
struct ShotSmem {
    static constexpr int D = COLOR ? 1344 : 352;
    shot_bin_t hist[4][D];
    float4 qd[4][128];       // dx, dy, dz, d2 of queued neighbours
    uint32_t qi[4][128];     // sorted index of queued neighbours
    WaveRows rows[4];
};

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
    a.r12sq_f = shot_r12sq_f(c.radius);
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
