// usc.hip — the Unique Shape Context descriptor (Features type "USC", 1960 floats) and the point density it weighs its deposits by.
// Reference seam: FeaturesUSC::iComputeDescriptors (features/features_usc.cpp) -> pcl::UniqueShapeContext. PCL is external: the
// arithmetic is this library's definition (include/ismhip.h above ismhip_usc), written from knowledge of PCL 1.10's
// usc.hpp, with two named deviations (phi = 0 for a point on the z axis; a value beyond the last edge takes the last bin).
//
// Two entries, one launch each:
//   k_point_density (timer "point_density"): per cloud point one THREAD, in cell-sorted order, counts the object's points inside the
//                     density ball (the sweep of k_ror_count, prefilter.hip); run once per cloud
//   k_usc           (timer "usc"): per keypoint one wavefront sweeps the ball (shot_wave.h) and deposits into its LDS histogram
// Gather model: sum_k M_k * (16 + 16 + 4) + K (24 + 36 + 4 * 1960) bytes (M_k = candidates of the ball: the position record; per ball
// point its record again for the original index and the density).
//
// Layout: 1960 64-bit bins per wave = 15 680 B, four waves per workgroup: 62 720 B dynamic LDS behind 14 336 B static (queue 8 KiB,
// indices 2 KiB, row tables 4 KiB) = 77 056 B per workgroup, two workgroups (eight waves) per CU of 160 KiB. A deposit is the integer
// q_p = (2^32 + n_p / 2) / n_p added with ds_add_u64: no float atomics, and the bin Q does not depend on the order of arrival. The
// per-point decisions (skip, the three bins) are taken in FP64 from float inputs, in the sequence of the definition, so they are those
// of the float64 restatement (tests/usc_ref.py) wherever no value lies within rounding of an edge.
#include "shot_wave.h"
#include <cfloat>
#include <cmath>

namespace {

#define USC_NA ISMHIP_USC_AZIMUTH_BINS
#define USC_NE ISMHIP_USC_ELEVATION_BINS
#define USC_NR ISMHIP_USC_RADIAL_BINS
static_assert(USC_NA * USC_NE * USC_NR == ISMHIP_USC_DIM && ISMHIP_USC_DIM <= ISMHIP_KNN_MAX_DIM, "USC grid");

struct UscArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start; const float4* sp4;
    const uint32_t* kp_off; const float *kx, *ky, *kz, *lrf;
    float radius, r2;
    float* desc; uint32_t* count;
    const uint32_t* density; unsigned long long* q;
    float edge[USC_NR + 1];               // the radial edges, as ismhip_usc_tables rounds them
    double lut[USC_NR * USC_NE];          // lut[j * 14 + k]
    int n_obj, nbx;
    const uint32_t* kp_perm;
};

struct DensityView {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start; const float4* sp4;
    int n_obj, nbx;
};

__global__ __launch_bounds__(256) void k_point_density(DensityView cv, float radius, float r2, uint32_t* __restrict__ density) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q = cv.sp4[base + t];
    uint32_t cnt = 0;
    ball_rows_for_each(m, cs, q.x, q.y, q.z, radius, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            cnt += sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2 ? 1u : 0u;
        }
        return true;
    });
    density[base + __float_as_uint(q.w)] = cnt;
}

struct UscSmem {
    float4 qd[4][128];                    // dx, dy, dz, d2 of queued neighbours
    uint32_t qi[4][128];                  // their cell-sorted indices
    WaveRows rows[4];
};

#define USC_DEG 57.29577951308232          // 180 / pi

__global__ __launch_bounds__(256) void k_usc(UscArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long usc_hist[];
    __shared__ UscSmem sm;
    constexpr int D = ISMHIP_USC_DIM;
    ShotWave w;
    if (!shot_wave_place(a, D, w)) return;
    const int lane = w.lane;
    unsigned long long* qrow = a.q ? a.q + (size_t)w.k * D : nullptr;
    const float* f = a.lrf + (size_t)w.k * 9;
    bool fin = true;
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(f[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.fx[i] = f[i]; w.fy[i] = f[3 + i]; w.fz[i] = f[6 + i]; }
    if (!shot_wave_ball(a, D, w, fin)) {
        if (qrow) for (int i = lane; i < D; i += 64) qrow[i] = 0ull;
        return;
    }
    unsigned long long* hist = usc_hist + (size_t)w.wv * D;
    for (int i = lane; i < D; i += 64) hist[i] = 0ull;
    const double x0 = w.fx[0], x1 = w.fx[1], x2 = w.fx[2], z0 = w.fz[0], z1 = w.fz[1], z2 = w.fz[2];
    const uint32_t base = a.pt_off[w.o];
    const uint32_t total = shot_wave_neighbours<16, true>(a, w, sm.qd[w.wv], sm.qi[w.wv], sm.rows[w.wv],
        [&](bool act, uint32_t gi, float dx, float dy, float dz, float) {
            if (!act) return;
            const double vx = dx, vy = dy, vz = dz;
            const double n2 = (vx * vx + vy * vy) + vz * vz;
            if (n2 <= (double)FLT_EPSILON) return;                        // the keypoint's own point and its close twins
            const double r = sqrt(n2);
            const double zv = (z0 * vx + z1 * vy) + z2 * vz;
            double c = zv / r;
            c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
            const double theta = acos(c) * USC_DEG;
            const double ux = vx - zv * z0, uy = vy - zv * z1, uz = vz - zv * z2;
            double phi = 0.0;
            if (!(ux == 0.0 && uy == 0.0 && uz == 0.0)) {
                const double cx = x1 * uz - x2 * uy, cy = x2 * ux - x0 * uz, cz = x0 * uy - x1 * ux;
                const double cn = sqrt((cx * cx + cy * cy) + cz * cz);
                const double xu = (x0 * ux + x1 * uy) + x2 * uz;
                phi = atan2(cn, xu) * USC_DEG;
                if ((cx * z0 + cy * z1) + cz * z2 < 0.0) phi = 360.0 - phi;
            }
            int j = USC_NR - 1, k = USC_NE - 1, l = USC_NA - 1;
#pragma unroll
            for (int t = USC_NR - 2; t >= 0; --t) if (r <= (double)a.edge[t + 1]) j = t;
#pragma unroll
            for (int t = USC_NE - 2; t >= 0; --t) if (theta <= (double)(t + 1) * (180.0 / USC_NE)) k = t;
#pragma unroll
            for (int t = USC_NA - 2; t >= 0; --t) if (phi <= (double)(t + 1) * (360.0 / USC_NA)) l = t;
            const uint32_t oi = __float_as_uint(a.sp4[gi].w);             // object-local original index: the density's order
            uint32_t np = a.density[base + oi];
            np = np ? np : 1u;
            const unsigned long long dep = ((1ull << 32) + (unsigned long long)(np >> 1)) / (unsigned long long)np;
            atomicAdd(&hist[l * (USC_NE * USC_NR) + k * USC_NR + j], dep);
        });
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // the deposits of the other lanes are read below
    for (int i = lane; i < D; i += 64) {
        const unsigned long long Q = hist[i];
        const int j = i % USC_NR, k = (i / USC_NR) % USC_NE;
        // a ball that holds no point (wave-uniform): the whole row NaN, as when the ball misses the grid
        w.row[i] = total == 0 ? __builtin_nanf("") : (float)((double)Q * 2.3283064365386962890625e-10 * a.lut[j * USC_NE + k]);
        if (qrow) qrow[i] = Q;
    }
}

bool usc_radii_ok(float radius, float min_radius) {
    return radius > 0.f && std::isfinite(radius) && min_radius > 0.f && min_radius < radius;
}
void usc_tables(float radius, float min_radius, double* lut, float* edges) {
    const double R = (double)radius, rmin = (double)min_radius, pi = 3.14159265358979323846;
    double e[USC_NR + 1];
    for (int j = 0; j <= USC_NR; ++j) e[j] = exp(log(rmin) + ((double)j / USC_NR) * log(R / rmin));
    if (edges) for (int j = 0; j <= USC_NR; ++j) edges[j] = (float)e[j];
    if (lut)
        for (int j = 0; j < USC_NR; ++j)
            for (int k = 0; k < USC_NE; ++k) {
                const double th0 = (double)k * pi / USC_NE, th1 = (double)(k + 1) * pi / USC_NE;
                const double vol = (cos(th0) - cos(th1)) * (e[j + 1] * e[j + 1] * e[j + 1] - e[j] * e[j] * e[j]) / 3.0 * (2.0 * pi / USC_NA);
                lut[j * USC_NE + k] = 1.0 / cbrt(vol);
            }
}

}  // namespace

extern "C" {

int ismhip_point_density(ismhip_ctx* ctx, const ismhip_cloud* cloud, float density_radius, uint32_t* density_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !density_out || !(density_radius > 0.f) || !std::isfinite(density_radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "point_density: bad argument");
    if (cloud->n_pts == 0) return ISMHIP_OK;
    TimerScope ts(ctx, "point_density");
    ISM_HIP(ctx, hipMemsetAsync(density_out, 0, (size_t)cloud->n_pts * sizeof(uint32_t), ctx->stream));   // points that are not finite
    DensityView cv;
    cv.pt_off = cloud->pt_off; cv.meta = cloud->meta; cv.cell_start = cloud->cell_start; cv.sp4 = cloud->sp4;
    cv.n_obj = cloud->n_obj; cv.nbx = std::max(1, (int)((cloud->max_pts + 255) / 256));
    const float r2 = (float)((double)density_radius * (double)density_radius);
    hipLaunchKernelGGL(k_point_density, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, density_radius, r2, density_out);
    ISM_CHECK_LAUNCH(ctx, "k_point_density");
    return ISMHIP_OK;
}

int ismhip_usc_tables(float radius, float min_radius, double* lut140_out, float* edges11_out) {
    if (!usc_radii_ok(radius, min_radius)) return ISMHIP_ERR_INVALID;
    usc_tables(radius, min_radius, lut140_out, edges11_out);
    return ISMHIP_OK;
}

int ismhip_usc(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
               const float* kpx, const float* kpy, const float* kpz, const float* lrf9, float radius, float min_radius,
               const uint32_t* density, float* desc_out, uint32_t* neighbour_count_out, unsigned long long* q_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    const ShotCall c = {ctx, cloud, kp_offsets_h, kpx, kpy, kpz, nullptr, lrf9, radius, desc_out, neighbour_count_out, "usc"};
    int rc = shot_check_call(c, density != nullptr && usc_radii_ok(radius, min_radius), false);
    if (rc != ISMHIP_OK) return rc;
    UscArgs a = {};
    uint32_t maxk;
    rc = shot_common_args(c, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.density = density; a.q = q_out;
    usc_tables(radius, min_radius, a.lut, a.edge);
    const size_t lds = (size_t)4 * ISMHIP_USC_DIM * sizeof(unsigned long long);
    rc = ism_lds_cap(ctx, (const void*)k_usc, lds);
    if (rc != ISMHIP_OK) return rc;
    return shot_launch(c, a, maxk, k_usc, lds);
}

}  // extern "C"
