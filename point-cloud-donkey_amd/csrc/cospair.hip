// cospair.hip — the CoSPAIR descriptor (Features type "CoSPAIR"), 378 floats: seven concentric shells around the cloud point nearest
// to the keypoint, per shell a 27-bin histogram of the three Darboux pair features (centre, neighbour) and a 27-bin histogram of the
// neighbour's CIELab colour. Reference seam: FeaturesCospair::iComputeDescriptors (features/features_cospair.cpp:28-77) ->
// COSPAIR::ComputeCOSPAIR (third_party/cospair/cospair.cpp:18-294) with num_levels 7, num_bins 9, rgb_type 5, num_rgb_bins 9; the pair
// features are PCL 1.10's computePairFeatures (pair_features.h), the colours PCL's RGB2CIELAB (common.h: rgb2lab). Definition and the
// five named decisions: DESIGN.md 4.10.
//
// Three launches under the timer "cospair":
//   k_cospair_codes : (first call on a cloud only) per point, the three colour histogram indices in the reference's double sequence
//   k_cospair_snap  : per keypoint, the nearest finite cloud point (lowest original index among equals) -> its sorted index and position
//   k_cospair       : per keypoint, one wavefront sweeps the ball of the SNAPPED point and counts into 378 LDS counters
// Gather model: sum_k M_k (16 + 16 + 2) + K (12 + 1512) bytes (M_k = points in the ball: the 16-byte position record of the sweep, the
// 16-byte normal and the 2-byte colour code gathered by the queued index; the centre, the row), plus the snap's few cells of records.
//
// Every deposit is +1 into a uint32 counter (ds_add_u32), so the row does not depend on the order the neighbours arrive in, and the
// level scale (count / pairs) * level is two float operations on exact integers: the row is bit-reproducible from the counts.
#include "shot_wave.h"
#include "pair_features.h"

namespace {

#define COSPAIR_LEVELS ISMHIP_COSPAIR_LEVELS
#define COSPAIR_BINS   ISMHIP_COSPAIR_BINS
#define COSPAIR_BLOCK  (3 * COSPAIR_BINS)            // 27: one histogram of one level
#define COSPAIR_LEVEL  (2 * COSPAIR_BLOCK)           // 54: geometry then colour
#define COSPAIR_DIM    ISMHIP_COSPAIR_DIM
#define COSPAIR_NONE   0xffffffffu
#define COSPAIR_SNAP_STEPS 4                         // boxes of radius 0, half the smallest cell edge, one and two largest cell edges; then the scan

struct CospairArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *sn4;
    const uint16_t* code;                 // colour codes, cell-sorted like sp4
    const uint32_t* kp_off;
    const float *kx, *ky, *kz;            // k_cospair_snap: the caller's keypoints; k_cospair: the snapped centres (scratch)
    float radius, r2;                     // r2 = r2_7, the ball of the sweep
    float r2l[COSPAIR_LEVELS - 1];        // r2_1 .. r2_6: level l owns r2_{l-1} <= d2 < r2_l
    uint32_t* snap;                       // [nkp] sorted object-local index of the snapped point, COSPAIR_NONE: no row
    float *sx, *sy, *sz;                  // [nkp] its position (NaN: no row), written by k_cospair_snap
    float* desc;
    uint32_t* count;                      // always nullptr: the ball population the sweep counts is not what CoSPAIR reports
    uint32_t *pair_count, *level_count, *snap_index;   // the three optional outputs
    int n_obj, nbx;
    const uint32_t* kp_perm;
};

// offset + bin inside the 27-entry array. The reference writes wherever the sum points: a bin 9 of the first or second feature lands on
// bin 0 of the next one (kept: it is inside the array); an index outside [0, 27) is a stack overwrite there and is clamped here
__device__ __forceinline__ int cospair_index(int offset, int bin) {
    const int i = offset + bin;
    return i < 0 ? 0 : (i > COSPAIR_BLOCK - 1 ? COSPAIR_BLOCK - 1 : i);
}

// ---- colour codes -------------------------------------------------------------------------------------------------------------
// cospair.cpp:220-235 for one point: float l = 1.0 * l / 100 etc. (sums and divisions in double, as the literals make them, rounded to
// float), bin = int(floor(double(x) / (1.0 / 9))). The three resolved indices, 5 bits each.
__global__ __launch_bounds__(256) void k_cospair_codes(const uint32_t* __restrict__ pt_off, const GridMeta* __restrict__ meta, const float4* __restrict__ sp4,
                                                       const uint32_t* __restrict__ rgba, const float* __restrict__ lut_srgb,
                                                       const float* __restrict__ lut_sxyz, uint16_t* __restrict__ code) {
    const int o = blockIdx.y;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= meta[o].n_finite) return;                                  // the sorted span holds the object's finite points first
    const uint32_t base = pt_off[o];
    float L, A, B;
    rgb2lab(lut_srgb, lut_sxyz, rgba[base + __float_as_uint(sp4[base + t].w)], L, A, B);
    const float l = (float)(1.0 * (double)L / 100), a = (float)(1.0 * ((double)A + 86.185) / 184.439), b = (float)(1.0 * ((double)B + 107.863) / 202.345);
    const int il = cospair_index(0, (int)floor((double)l / (1.0 / COSPAIR_BINS)));
    const int ia = cospair_index(COSPAIR_BINS, (int)floor((double)a / (1.0 / COSPAIR_BINS)));
    const int ib = cospair_index(2 * COSPAIR_BINS, (int)floor((double)b / (1.0 / COSPAIR_BINS)));
    code[base + t] = (uint16_t)(il | (ia << 5) | (ib << 10));
}

// ---- the snap -----------------------------------------------------------------------------------------------------------------
// nearestKSearch(keypoint, 1) over the finite points of the object, one wave per keypoint: the minimum of the 64-bit key (bits of the
// float d2, original index) -- d2 >= 0, so its bits order as its value, and among equal distances the lowest original index wins.
// The wave reads a box of cells around the keypoint and grows it; invariant and stopping rule are those of k_sor_meandist
// (prefilter.hip): a point outside the box is at least as far as the nearest box face that still has cells behind it, so the search
// stops when the best d2 is <= the square of that distance (taken conservatively), or when the box is the whole grid. Every step
// reads its whole box (a lane's best key only improves). A keypoint still open after COSPAIR_SNAP_STEPS boxes -- far off the grid, or
// in an empty region -- reads the object's n_finite records once. Which path ran never shows: all end with the minimum over the object.
__global__ __launch_bounds__(256) void k_cospair_snap(CospairArgs a) {
    ShotWave w;
    if (!shot_wave_place(a, 0, w)) return;
    const int lane = w.lane;
    const GridMeta& m = w.m;
    const float q[3] = {w.cx, w.cy, w.cz};
    const uint32_t base = a.pt_off[w.o];
    unsigned long long best = ~0ull;
    uint32_t best_i = COSPAIR_NONE;
    auto consider = [&](uint32_t i) {
        const float4 p = a.sp4[base + i];
        const unsigned long long key = ((unsigned long long)__float_as_uint(sqdist3(p.x, p.y, p.z, q[0], q[1], q[2])) << 32) | __float_as_uint(p.w);
        if (key < best) { best = key; best_i = i; }
    };
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && m.n_finite > 0) {
        const uint32_t* cs = a.cell_start + (size_t)w.o * ISM_GRID_STRIDE;
        const float cmax = fmaxf(m.cell[0], fmaxf(m.cell[1], m.cell[2])), cmin = fminf(m.cell[0], fminf(m.cell[1], m.cell[2]));
        bool done = false;
        for (int s = 0; s < COSPAIR_SNAP_STEPS && !done; ++s) {
            const float R = s == 0 ? 0.f : (s == 1 ? 0.5f * cmin : (float)(s - 1) * cmax);
            int lo[3], hi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lo[c] = cell_coord(q[c] - R, m.minv[c], m.inv_cell[c], m.dim[c]);
                hi[c] = cell_coord(q[c] + R, m.minv[c], m.inv_cell[c], m.dim[c]);
            }
            for (int gz = lo[2]; gz <= hi[2]; ++gz)
                for (int gy = lo[1]; gy <= hi[1]; ++gy) {
                    const int rb = (gz * m.dim[1] + gy) * m.dim[0];
                    const uint32_t e = cs[rb + hi[0] + 1];                  // x is the fastest cell axis: a row of cells is one span
                    for (uint32_t i = cs[rb + lo[0]] + lane; i < e; i += 64) consider(i);
                }
            const unsigned long long wb = wave_min_u64(best);
            float face = INFINITY;                                         // nearest face of the box that has unread cells behind it
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float pad = (fabsf(q[c]) + fabsf(m.minv[c]) + m.cell[c] * (float)m.dim[c]) * 4e-6f;
                if (lo[c] > 0) face = fminf(face, q[c] - (m.minv[c] + (float)lo[c] * m.cell[c]) - pad);
                if (hi[c] < m.dim[c] - 1) face = fminf(face, (m.minv[c] + (float)(hi[c] + 1) * m.cell[c]) - q[c] - pad);
            }
            if (face == INFINITY) done = true;                             // the box is the whole grid
            else if (wb != ~0ull && face > 0.f && __uint_as_float((uint32_t)(wb >> 32)) <= face * face * 0.99999f) done = true;
        }
        if (!done)
            for (uint32_t i = lane; i < m.n_finite; i += 64) consider(i);
    }
    const unsigned long long wb = wave_min_u64(best);
    uint32_t si = COSPAIR_NONE;
    float4 c = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0.f);
    if (wb != ~0ull) {                                                     // wave-uniform; the key is unique: exactly one lane holds it
        const unsigned long long who = __ballot(best == wb);
        si = (uint32_t)__shfl((int)best_i, __ffsll((long long)who) - 1, 64);
        c = a.sp4[base + si];
    }
    if (lane == 0) { a.snap[w.k] = si; a.sx[w.k] = c.x; a.sy[w.k] = c.y; a.sz[w.k] = c.z; }
}

// ---- the descriptor -----------------------------------------------------------------------------------------------------------
struct CospairSmem {
    float4 qd[4][128];                    // dx, dy, dz, d2 of queued neighbours
    uint32_t qi[4][128];                  // their sorted indices
    WaveRows rows[4];
    uint32_t hist[4][COSPAIR_DIM + 6];    // the counters of each wave's row
};

// The three geometry indices by the reference's sequence (cospair.cpp:94-102): computePairFeatures (its return value ignored: PCL 1.10
// has zeroed f1..f3 when it returns false), deg_f1 = rad2deg(f1) + 180, deg = rad2deg(SafeAcos(f)) in float (rad2deg(float) multiplies by
// 57.29578f; the reference's unqualified acos is taken as acosf), bin = int(floor(double(deg) / (360.0 / 9))) or / (180.0 / 9).
__device__ __forceinline__ void cospair_bins_exact(float dx, float dy, float dz, const float4& cn, const float4& qn, int& g1, int& g2, int& g3) {
    float f1, f2, f3;
    if (!pair_features(0.f, 0.f, 0.f, cn.x, cn.y, cn.z, dx, dy, dz, qn.x, qn.y, qn.z, f1, f2, f3)) { f1 = 0.f; f2 = 0.f; f3 = 0.f; }
    auto safe_acos = [](float x) { return acosf(x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x)); };
    const float deg1 = f1 * 57.29578f + 180.0f, deg2 = safe_acos(f2) * 57.29578f, deg3 = safe_acos(f3) * 57.29578f;
    g1 = cospair_index(0, (int)floor((double)deg1 / (360.0 / COSPAIR_BINS)));
    g2 = cospair_index(COSPAIR_BINS, (int)floor((double)deg2 / (180.0 / COSPAIR_BINS)));
    g3 = cospair_index(2 * COSPAIR_BINS, (int)floor((double)deg3 / (180.0 / COSPAIR_BINS)));
}

// The same indices from the FAST features (pair_features.h), when they can be trusted. f1: t1 = 9 (f1 + pi) / 2pi must keep
// COSPAIR_GUARD_T from every integer (the fast value differs from the exact one by < 2e-5 in t, as in fpfh.hip), and for x < 0 from
// the +-pi seam, where the sign of y alone decides between bin 0, bin 8 and the spill of f1 = +pi. f2 and f3: their bin is
// floor(acos(f) 9 / pi) = the number of edges cos(j pi / 9), j = 1..8, that f does not exceed -- no acos at all; f must keep
// COSPAIR_GUARD_F from every edge (the fast f differs from the exact one by < 4e-6, and the exact path's acosf and product move the
// edge by < 1e-6 in f) and from -1, whose bin 9 spills. false: the caller takes cospair_bins_exact.
#define COSPAIR_GUARD_T 1e-4f
#define COSPAIR_GUARD_F 2e-5f
__device__ __forceinline__ bool cospair_bins_fast(float dx, float dy, float dz, const float4& cn, const float4& qn, int& g1, int& g2, int& g3) {
    float f1, f2, f3, x;
    if (!pair_features_fast(0.f, 0.f, 0.f, cn.x, cn.y, cn.z, dx, dy, dz, qn.x, qn.y, qn.z, f1, f2, f3, x)) return false;
    const float t1 = (float)COSPAIR_BINS * ((f1 + 3.14159265358979323846f) * 0.15915494309189535f);
    if (x < 0.f && !(t1 > COSPAIR_GUARD_T && t1 < (float)COSPAIR_BINS - COSPAIR_GUARD_T)) return false;
    const float fr = t1 - floorf(t1);
    bool sure = fr > COSPAIR_GUARD_T && fr < 1.0f - COSPAIR_GUARD_T;     // false for NaN
    sure = sure && f2 > -1.0f + COSPAIR_GUARD_F && f3 > -1.0f + COSPAIR_GUARD_F;
    const float edge[COSPAIR_BINS - 1] = {0.93969262078590838f, 0.76604444311897804f, 0.5f, 0.17364817766693035f,
                                          -0.17364817766693035f, -0.5f, -0.76604444311897804f, -0.93969262078590838f};
    int b2 = 0, b3 = 0;
#pragma unroll
    for (int j = 0; j < COSPAIR_BINS - 1; ++j) {
        b2 += f2 <= edge[j] ? 1 : 0; b3 += f3 <= edge[j] ? 1 : 0;
        sure = sure && fabsf(f2 - edge[j]) > COSPAIR_GUARD_F && fabsf(f3 - edge[j]) > COSPAIR_GUARD_F;
    }
    if (!sure) return false;
    g1 = (int)floorf(t1); g2 = COSPAIR_BINS + b2; g3 = 2 * COSPAIR_BINS + b3;   // t1 in (0, 9), b in 0..8: inside their own blocks
    return true;
}

// the outputs of a keypoint without a row, beside the NaN row itself
__device__ __forceinline__ void cospair_no_row(const CospairArgs& a, uint32_t k, int lane) {
    if (a.level_count && lane < COSPAIR_LEVELS) a.level_count[(size_t)k * COSPAIR_LEVELS + lane] = 0u;
    if (lane == 0) {
        if (a.pair_count) a.pair_count[k] = 0u;
        if (a.snap_index) a.snap_index[k] = COSPAIR_NONE;
    }
}

// 106 VGPRs, no scratch, 20 KiB static LDS per workgroup (queue 10 KiB, row tables 4 KiB, counters 6 KiB): 4 waves per SIMD by
// registers (the compiler's resource report); k_cospair_snap 34 VGPRs, k_cospair_codes 18, neither with LDS or scratch
__global__ __launch_bounds__(256) void k_cospair(CospairArgs a) {
    __shared__ CospairSmem sm;
    ShotWave w;
    if (!shot_wave_place(a, COSPAIR_DIM, w)) return;                     // the centre: the snapped point's position
    const int wv = w.wv, lane = w.lane;
    const uint32_t base = a.pt_off[w.o];
    const uint32_t si = a.snap[w.k];                                     // wave-uniform
    float4 cn = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
    if (si != COSPAIR_NONE) cn = a.sn4[base + si];
    // no snapped point (keypoint not finite, object without a finite point) or its normal not finite: the whole row NaN, counts 0
    if (!shot_wave_ball(a, COSPAIR_DIM, w, isfinite(cn.x) && isfinite(cn.y) && isfinite(cn.z))) { cospair_no_row(a, w.k, lane); return; }
    uint32_t* hist = sm.hist[wv];
    for (int i = lane; i < COSPAIR_DIM; i += 64) hist[i] = 0u;
    const uint32_t centre = base + si;
    uint32_t nl[COSPAIR_LEVELS];                                          // pairs per level, wave-uniform
#pragma unroll
    for (int l = 0; l < COSPAIR_LEVELS; ++l) nl[l] = 0u;
    shot_wave_neighbours<16, true>(a, w, sm.qd[wv], sm.qi[wv], sm.rows[wv],
        [&](bool act, uint32_t gi, float dx, float dy, float dz, float d2) {
            int lev = -1;                                                 // -1: no pair (idle lane, the snapped point itself, a normal that is not finite)
            if (act && gi != centre) {                                    // level 1 drops the snapped point by index; its coincident twins are pairs
                const float4 qn = a.sn4[gi];
                if (isfinite(qn.x) && isfinite(qn.y) && isfinite(qn.z)) {
                    const uint32_t code = a.code[gi];
                    lev = 0;
#pragma unroll
                    for (int l = 0; l < COSPAIR_LEVELS - 1; ++l) lev += d2 >= a.r2l[l] ? 1 : 0;
                    int g1, g2, g3;
                    if (!cospair_bins_fast(dx, dy, dz, cn, qn, g1, g2, g3)) cospair_bins_exact(dx, dy, dz, cn, qn, g1, g2, g3);
                    uint32_t* h = hist + lev * COSPAIR_LEVEL;
                    atomicAdd(&h[g1], 1u); atomicAdd(&h[g2], 1u); atomicAdd(&h[g3], 1u);
                    atomicAdd(&h[COSPAIR_BLOCK + (code & 31u)], 1u);
                    atomicAdd(&h[COSPAIR_BLOCK + ((code >> 5) & 31u)], 1u);
                    atomicAdd(&h[COSPAIR_BLOCK + ((code >> 10) & 31u)], 1u);
                }
            }
#pragma unroll
            for (int l = 0; l < COSPAIR_LEVELS; ++l) nl[l] += (uint32_t)__popcll(__ballot(lev == l));
        });
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // the deposits of the other lanes are read below
    // level scale (cospair.cpp:270-288): (count / levelpaircount) * l in float, an empty level stays zero; no final normalisation
    uint32_t total = 0;
    for (int i = lane; i < COSPAIR_DIM; i += 64) {
        const int l = i / COSPAIR_LEVEL;
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < COSPAIR_LEVELS; ++j) n = l == j ? nl[j] : n;
        w.row[i] = n ? ((float)hist[i] / (float)n) * (float)(l + 1) : 0.f;
    }
#pragma unroll
    for (int l = 0; l < COSPAIR_LEVELS; ++l) {
        total += nl[l];
        if (a.level_count && lane == l) a.level_count[(size_t)w.k * COSPAIR_LEVELS + l] = nl[l];
    }
    if (lane == 0) {
        if (a.pair_count) a.pair_count[w.k] = total;
        if (a.snap_index) a.snap_index[w.k] = __float_as_uint(a.sp4[centre].w);
    }
}

}  // namespace

extern "C" int ismhip_cospair(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                              const float* kpx, const float* kpy, const float* kpz, float radius, float* desc_out,
                              uint32_t* neighbour_count_out, uint32_t* level_count_out, uint32_t* snap_index_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !desc_out || !(radius > 0.f))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cospair: bad argument");
    if (!cloud->rgba) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cospair: colour arrays missing");
    const int n_obj = cloud->n_obj;
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, "cospair", kp_offsets_h, n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK || kp.max_run == 0) return rc;
    const size_t nkp = kp.total;
    uint32_t* scr = (uint32_t*)ism_scratch(ctx, SCR_COSPAIR, nkp * 16);
    if (!scr) return ISMHIP_ERR_NOMEM;
    ismhip_cloud* c = const_cast<ismhip_cloud*>(cloud);                 // the colour-code cache, as ism_kp_order keeps the keypoint order
    const size_t np = cloud->n_pts ? cloud->n_pts : 1;
    if (c->cospair_code_cap < np) {
        if (c->cospair_code) { ISM_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(c->cospair_code); c->cospair_code = nullptr; c->cospair_code_cap = 0; }
        c->cospair_code_valid = false;
        if (hipMalloc((void**)&c->cospair_code, (np + np / 8) * sizeof(uint16_t)) != hipSuccess) {
            (void)hipGetLastError();
            return ism_set_err(ctx, ISMHIP_ERR_NOMEM, "cospair: hipMalloc colour codes");
        }
        c->cospair_code_cap = np + np / 8;
    }
    CospairArgs a;
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4; a.sn4 = cloud->sn4;
    a.code = c->cospair_code;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz;
    a.radius = radius; a.r2 = (float)((double)radius * (double)radius);
    for (int l = 1; l < COSPAIR_LEVELS; ++l) {                           // cospair.cpp:65: r = ((l * 1.0) / num_levels) * radius, in double
        const double r = ((double)l / COSPAIR_LEVELS) * (double)radius;
        a.r2l[l - 1] = (float)(r * r);
    }
    a.snap = scr; a.sx = (float*)(scr + nkp); a.sy = (float*)(scr + 2 * nkp); a.sz = (float*)(scr + 3 * nkp);
    a.desc = desc_out; a.count = nullptr;
    a.pair_count = neighbour_count_out; a.level_count = level_count_out; a.snap_index = snap_index_out;
    a.n_obj = ctx->xcd_map ? n_obj : 0; a.nbx = (int)((kp.max_run + 3) / 4);
    TimerScope ts(ctx, "cospair");
    if (!c->cospair_code_valid) {
        hipLaunchKernelGGL(k_cospair_codes, dim3((cloud->max_pts + 255) / 256 ? (cloud->max_pts + 255) / 256 : 1, n_obj), dim3(256), 0, ctx->stream,
                           cloud->pt_off, cloud->meta, cloud->sp4, cloud->rgba, ctx->lut_srgb, ctx->lut_sxyz, c->cospair_code);
        ISM_CHECK_LAUNCH(ctx, "k_cospair_codes");
        c->cospair_code_valid = true;
    }
    a.kp_perm = ism_kp_order(ctx, cloud, kp_offsets_h, a.kp_off, kpx, kpy, kpz, kp.max_run);
    const dim3 grid(ctx->xcd_map ? xcd_object_grid((unsigned)a.nbx, n_obj) : (unsigned)a.nbx * (unsigned)n_obj);
    hipLaunchKernelGGL(k_cospair_snap, grid, dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_cospair_snap");
    a.kx = a.sx; a.ky = a.sy; a.kz = a.sz;                               // the sweep is centred on the snapped points
    hipLaunchKernelGGL(k_cospair, grid, dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_cospair");
    return ISMHIP_OK;
}
