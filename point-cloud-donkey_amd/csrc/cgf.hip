// cgf.hip — the raw half of the CGF descriptor (Features type "CGF"): the 17 x 11 x 12 spherical histogram of a keypoint's ball in the
// keypoint's own frame, 2244 floats, which mlp.hip then embeds into the 32 or 40 floats the codebook sees. Reference seam:
// FeaturesCGF::iComputeDescriptors (features/features_cgf.cpp:31-102) -> compute_intensities (third_party/cgf/cgf.cpp:64-165). The
// reference states the whole arithmetic; definition and named deviations: DESIGN.md 4.20, restated in tests/cgf_ref.py.
//
// Two entries, both one wavefront per keypoint in cell order (shot_wave.h), four per workgroup:
//   ismhip_keypoint_normals_pca (timer "keypoint_normals_pca")
//     k_cgf_normals : the sweep and the arithmetic of k_pca_normals (lrf.hip) with the keypoint as the query instead of a cloud point:
//                     FP64 moments about the query, eigen3.h, at least 3 ball points, flipped towards (0,0,0)
//   ismhip_cgf_raw (timer "cgf_raw")
//     k_cgf_raw     : the frame (identity for an invalid one, negated against the normal), ONE sweep of the R ball, one ds_add_u32 per
//                     neighbour into the wave's 2244 LDS counters. cgf.cpp skips the first entry of a distance-sorted list: every lane
//                     remembers the smallest (d2, original index) it met and the bin it put it in, the wave takes the minimum of the 64
//                     keys and the owner takes its deposit back -- no second sweep, no sort.
//   - bins: COUNTS OF THRESHOLDS PASSED in float (r^2 against the 16 radial edges squared, z / r against the cosines of the 10 polar
//     edges, atan2f against the 11 azimuth edges), taken twice, against either end of a guard band about every edge; where the two
//     counts differ the lane evaluates the defining double formulas (log, acos, atan2). As k_rsd does.
// Counts are uint32, no float atomics: two calls, any cell size and any lane mapping give the same bytes.
#include "shot_wave.h"
#include "eigen3.h"
#include <cfloat>
#include <cmath>

namespace {

#define CGF_NR ISMHIP_CGF_RADIAL_BINS
#define CGF_NT ISMHIP_CGF_POLAR_BINS
#define CGF_NP ISMHIP_CGF_AZIMUTH_BINS
#define CGF_DIM ISMHIP_CGF_RAW_DIM
#define CGF_RAD2DEG 57.29578                          // pcl::rad2deg(double), as cgf.cpp:141-142 calls it
static_assert(CGF_DIM == CGF_NR * CGF_NT * CGF_NP, "CGF layout");

struct CgfArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    const uint32_t* kp_off; const float *kx, *ky, *kz;
    const float* lrf; const float *knx, *kny, *knz;   // k_cgf_raw: the frames and the keypoint normals
    float *nxo, *nyo, *nzo;                           // k_cgf_normals: the outputs
    float radius, r2;                                 // the ball of the launch (k_cgf_normals: the normal radius)
    double R, rmin;                                   // k_cgf_raw: the doubles of the definition
    float r2lo[CGF_NR - 1], r2hi[CGF_NR - 1];         // (rmin (R / rmin)^((k - 1) / 16))^2 (1 -+ guard), k = 1..16
    float clo[CGF_NT - 1], chi[CGF_NT - 1];           // cos((180 k / 11) / 57.29578) -+ guard, k = 1..10
    float plo[CGF_NP - 1], phi[CGF_NP - 1];           // (30 k - 180) / 57.29578 -+ guard, k = 1..11
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;
};

__global__ __launch_bounds__(256) void k_cgf_normals(CgfArgs a) {
    __shared__ WaveRows s_rows[4];
    ShotWave w;
    if (!shot_wave_place(a, 0, w)) return;
    const int lane = w.lane;
    const float qx = w.cx, qy = w.cy, qz = w.cz;
    const uint32_t base = a.pt_off[w.o];
    const uint32_t* cs = a.cell_start + (size_t)w.o * ISM_GRID_STRIDE;
    double sx = 0, sy = 0, sz = 0, xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
    int cnt = 0;
    // (wave-uniform: every lane holds the same keypoint)
    if (isfinite(qx) && isfinite(qy) && isfinite(qz) && w.m.n_finite > 0 && ball_cells(w.m, qx, qy, qz, a.radius, w.cr))
        ball_for_each(w.m, cs, w.cr, qx, qy, qz, a.radius, lane, s_rows[w.wv],
                      [&](uint32_t t, bool) { return a.sp4[base + t]; },
                      [&](const float4& p, uint32_t, bool v) {
            if (!v) return;
            if (sqdist3(p.x, p.y, p.z, qx, qy, qz) < a.r2) {
                const double dx = (double)p.x - (double)qx, dy = (double)p.y - (double)qy, dz = (double)p.z - (double)qz;
                sx += dx; sy += dy; sz += dz;
                xx = fma(dx, dx, xx); xy = fma(dx, dy, xy); xz = fma(dx, dz, xz); yy = fma(dy, dy, yy); yz = fma(dy, dz, yz); zz = fma(dz, dz, zz);
                cnt++;
            }
        });
    sx = wave_sum_d(sx); sy = wave_sum_d(sy); sz = wave_sum_d(sz);
    xx = wave_sum_d(xx); xy = wave_sum_d(xy); xz = wave_sum_d(xz); yy = wave_sum_d(yy); yz = wave_sum_d(yz); zz = wave_sum_d(zz);
    cnt = wave_sum_i(cnt);
    if (lane != 0) return;
    float n0 = __builtin_nanf(""), n1 = n0, n2 = n0;
    if (cnt >= 3) {
        const double inv = 1.0 / (double)cnt, mx = sx * inv, my = sy * inv, mz = sz * inv;
        double A[3][3] = {{xx * inv - mx * mx, xy * inv - mx * my, xz * inv - mx * mz}, {xy * inv - mx * my, yy * inv - my * my, yz * inv - my * mz},
                          {xz * inv - mx * mz, yz * inv - my * mz, zz * inv - mz * mz}};
        double ev[3], V[3][3];
        eigen_sym3(A, ev, V);
        n0 = (float)V[0][0]; n1 = (float)V[1][0]; n2 = (float)V[2][0];
        // flipNormalTowardsViewpoint, viewpoint (0,0,0): flip when (0 - q) . n < 0
        const float vx = 0.f - qx, vy = 0.f - qy, vz = 0.f - qz;
        if (vx * n0 + vy * n1 + vz * n2 < 0) { n0 = -n0; n1 = -n1; n2 = -n2; }
    }
    a.nxo[w.k] = n0; a.nyo[w.k] = n1; a.nzo[w.k] = n2;
}

// the bin of one neighbour by the definition, in double (cgf.cpp:140-151); a NaN lands in bin 0 of its coordinate
__device__ __forceinline__ int cgf_bin_exact(double x, double y, double z, double ln_rmin, double ln_ratio) {
    const double r = sqrt((x * x + y * y) + z * z);
    const double theta = acos(z / r) * CGF_RAD2DEG, phi = atan2(y, x) * CGF_RAD2DEG;
    const double tr = (CGF_NR - 1) * (log(r) - ln_rmin) / ln_ratio + 1.0;
    const double tt = CGF_NT * theta / 180.0, tp = CGF_NP * (phi + 180.0) / 360.0;
    const int br = !(tr > 0.0) ? 0 : (tr >= (double)CGF_NR ? CGF_NR - 1 : (int)tr);
    const int bt = !(tt > 0.0) ? 0 : (tt >= (double)CGF_NT ? CGF_NT - 1 : (int)tt);
    const int bp = !(tp > 0.0) ? 0 : (tp >= (double)CGF_NP ? CGF_NP - 1 : (int)tp);
    return br + CGF_NR * bt + CGF_NR * CGF_NT * bp;
}

// 40 KiB static LDS per workgroup: four histograms of 2244 counters, four row tables
__global__ __launch_bounds__(256) void k_cgf_raw(CgfArgs a) {
    __shared__ uint32_t s_hist[4][CGF_DIM];
    __shared__ WaveRows s_rows[4];
    ShotWave w;
    if (!shot_wave_place(a, CGF_DIM, w)) return;
    const int lane = w.lane;
    if (!(isfinite(w.cx) && isfinite(w.cy) && isfinite(w.cz))) {          // a keypoint that is no point: the whole row NaN
        for (int i = lane; i < CGF_DIM; i += 64) w.row[i] = __builtin_nanf("");
        if (a.count && lane == 0) a.count[w.k] = 0;
        return;
    }
    uint32_t* hist = s_hist[w.wv];
    for (int i = lane; i < CGF_DIM; i += 64) hist[i] = 0u;
    // the frame (cgf.cpp:112-129)
    const float* f = a.lrf + (size_t)w.k * 9;
    float ax[3] = {f[0], f[1], f[2]}, ay[3] = {f[3], f[4], f[5]}, az[3] = {f[6], f[7], f[8]};
    if (ax[0] != ax[0] || ax[1] != ax[1] || ax[2] != ax[2]) {
        ax[0] = 1.f; ax[1] = 0.f; ax[2] = 0.f; ay[0] = 0.f; ay[1] = 1.f; ay[2] = 0.f; az[0] = 0.f; az[1] = 0.f; az[2] = 1.f;
    } else if ((az[0] * a.knx[w.k] + az[1] * a.kny[w.k]) + az[2] * a.knz[w.k] < 0.f) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { ax[i] = -ax[i]; ay[i] = -ay[i]; az[i] = -az[i]; }
    }
    const double ln_rmin = log(a.rmin), ln_ratio = log(a.R / a.rmin);     // cgf.cpp:98-99
    const float cx = w.cx, cy = w.cy, cz = w.cz;
    const uint32_t base = a.pt_off[w.o];
    const uint32_t* cs = a.cell_start + (size_t)w.o * ISM_GRID_STRIDE;
    unsigned long long best = ~0ull;                                      // the smallest (d2, original index) this lane met
    int best_bin = -1, cnt = 0;                                           // and the bin it went to (-1: none)
    if (w.m.n_finite > 0 && ball_cells(w.m, cx, cy, cz, a.radius, w.cr))
        ball_for_each<8, true>(w.m, cs, w.cr, cx, cy, cz, a.radius, lane, s_rows[w.wv],
                      [&](uint32_t t, bool) { return a.sp4[base + t]; },
                      [&](const float4& p, uint32_t, bool v) {
            if (!v) return;
            const float d2 = sqdist3(p.x, p.y, p.z, cx, cy, cz);
            if (!(d2 < a.r2)) return;
            int bin = -1;
            if ((double)d2 > 1e-15) {                                     // cgf.cpp:134
                const float vx = p.x - cx, vy = p.y - cy, vz = p.z - cz;
                const float x = (vx * ax[0] + vy * ax[1]) + vz * ax[2], y = (vx * ay[0] + vy * ay[1]) + vz * ay[2], z = (vx * az[0] + vy * az[1]) + vz * az[2];
                const float rr = (x * x + y * y) + z * z;
                const float c = z / sqrtf(rr), ph = atan2f(y, x);
                int br = 0, br2 = 0, bt = 0, bt2 = 0, bp = 0, bp2 = 0;
#pragma unroll
                for (int k = 0; k < CGF_NR - 1; ++k) { br += rr >= a.r2hi[k] ? 1 : 0; br2 += rr >= a.r2lo[k] ? 1 : 0; }
#pragma unroll
                for (int k = 0; k < CGF_NT - 1; ++k) { bt += c <= a.clo[k] ? 1 : 0; bt2 += c <= a.chi[k] ? 1 : 0; }
#pragma unroll
                for (int k = 0; k < CGF_NP - 1; ++k) { bp += ph >= a.phi[k] ? 1 : 0; bp2 += ph >= a.plo[k] ? 1 : 0; }
                if (br != br2 || bt != bt2 || bp != bp2 || !(rr > 1e-30f) || !(rr < 1e30f))      // inside a guard band, or no float to trust
                    bin = cgf_bin_exact((double)x, (double)y, (double)z, ln_rmin, ln_ratio);
                else bin = br + CGF_NR * bt + CGF_NR * CGF_NT * bp;
                atomicAdd(&hist[bin], 1u);
                cnt++;
            }
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | __float_as_uint(p.w);   // d2 >= 0: its bits order as its value
            if (key < best) { best = key; best_bin = bin; }
        });
    // THE SKIP RULE: the nearest ball point (ties: the lowest original index) is not part of the histogram
    unsigned long long wmin = best;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long o = ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(wmin >> 32), s, 64) << 32) |
                                     (unsigned)__shfl_xor((int)(unsigned)(wmin & 0xffffffffull), s, 64);
        wmin = o < wmin ? o : wmin;
    }
    if (best == wmin && best != ~0ull && best_bin >= 0) { atomicSub(&hist[best_bin], 1u); cnt--; }   // (a key is one point: one owner)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // the deposits of the other lanes are read below
    cnt = wave_sum_i(cnt);
    const double sum = (double)cnt;
    for (int i = lane; i < CGF_DIM; i += 64) w.row[i] = cnt > 0 ? (float)((double)hist[i] / sum) : 0.f;   // cgf.cpp:156-160
    if (a.count && lane == 0) a.count[w.k] = (uint32_t)cnt;
}

int cgf_common(ismhip_ctx* ctx, const char* name, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h, const float* kpx, const float* kpy,
               const float* kpz, CgfArgs& a, uint32_t& maxk) {
    RaggedOffsets kp;
    maxk = 0;
    int rc = ism_ragged_offsets(ctx, name, kp_offsets_h, cloud->n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK) return rc;
    maxk = kp.max_run;
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz;
    a.n_obj = ctx->xcd_map ? cloud->n_obj : 0; a.nbx = (int)((maxk + 3) / 4);
    return ISMHIP_OK;
}

int cgf_launch(ismhip_ctx* ctx, const char* name, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h, CgfArgs& a, uint32_t maxk, void (*kernel)(CgfArgs)) {
    TimerScope ts(ctx, name);
    a.kp_perm = ism_kp_order(ctx, cloud, kp_offsets_h, a.kp_off, a.kx, a.ky, a.kz, maxk);
    const dim3 grid(ctx->xcd_map ? xcd_object_grid((unsigned)a.nbx, cloud->n_obj) : (unsigned)a.nbx * (unsigned)cloud->n_obj);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, name);
    return ISMHIP_OK;
}

}  // namespace

extern "C" {

int ismhip_keypoint_normals_pca(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                                const float* kpx, const float* kpy, const float* kpz, float radius,
                                float* knx_out, float* kny_out, float* knz_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !knx_out || !kny_out || !knz_out || !(radius > 0.f) || !std::isfinite(radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "keypoint_normals_pca: bad argument");
    CgfArgs a = {};
    uint32_t maxk;
    int rc = cgf_common(ctx, "keypoint_normals_pca", cloud, kp_offsets_h, kpx, kpy, kpz, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.nxo = knx_out; a.nyo = kny_out; a.nzo = knz_out;
    a.radius = radius; a.r2 = (float)((double)radius * (double)radius);
    return cgf_launch(ctx, "keypoint_normals_pca", cloud, kp_offsets_h, a, maxk, k_cgf_normals);
}

int ismhip_cgf_raw(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                   const float* kpx, const float* kpy, const float* kpz, const float* lrf9,
                   const float* knx, const float* kny, const float* knz, double radius, double rmin,
                   float* desc_out, uint32_t* neighbour_count_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !lrf9 || !knx || !kny || !knz || !desc_out || !(radius > 0.0) || !std::isfinite(radius) ||
        !(rmin > 0.0) || !(rmin < radius) || !((float)radius > 0.f) || !std::isfinite((float)radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cgf_raw: bad argument");
    CgfArgs a = {};
    uint32_t maxk;
    int rc = cgf_common(ctx, "cgf_raw", cloud, kp_offsets_h, kpx, kpy, kpz, a, maxk);
    if (rc != ISMHIP_OK || maxk == 0) return rc;
    a.lrf = lrf9; a.knx = knx; a.kny = kny; a.knz = knz;
    a.radius = (float)radius; a.r2 = (float)(radius * radius);
    a.R = radius; a.rmin = rmin;
    a.desc = desc_out; a.count = neighbour_count_out;
    // The guard bands. r^2 in float carries 2e-7 relative: 1e-6 either side of an edge squared. z / r carries 3e-7: 2e-6 either side of
    // a cosine (no polar edge lies within 16 degrees of a pole, where the cosine is flat). atan2f carries 1e-6: 1e-5 either side.
    // A radius so small or so large that a radial band does not enclose its edge in float leaves every radial band open (lo = -1,
    // hi = inf): every neighbour then takes the double formulas.
    bool closed = true;
    for (int k = 1; k < CGF_NR; ++k) {
        const double e = rmin * pow(radius / rmin, (double)(k - 1) / (double)(CGF_NR - 1)), e2 = e * e;
        a.r2lo[k - 1] = (float)(e2 * (1.0 - 1e-6)); a.r2hi[k - 1] = (float)(e2 * (1.0 + 1e-6));
        closed = closed && a.r2lo[k - 1] >= 1e-28f && a.r2hi[k - 1] < 1e28f && (double)a.r2lo[k - 1] < e2 * (1.0 - 5e-7) && (double)a.r2hi[k - 1] > e2 * (1.0 + 5e-7);
    }
    if (!closed)
        for (int k = 0; k < CGF_NR - 1; ++k) { a.r2lo[k] = -1.0f; a.r2hi[k] = INFINITY; }
    for (int k = 1; k < CGF_NT; ++k) {
        const double e = cos((180.0 * k / CGF_NT) / CGF_RAD2DEG);
        a.clo[k - 1] = (float)(e - 2e-6); a.chi[k - 1] = (float)(e + 2e-6);
    }
    for (int k = 1; k < CGF_NP; ++k) {
        const double e = (360.0 * k / CGF_NP - 180.0) / CGF_RAD2DEG;
        a.plo[k - 1] = (float)(e - 1e-5); a.phi[k - 1] = (float)(e + 1e-5);
    }
    return cgf_launch(ctx, "cgf_raw", cloud, kp_offsets_h, a, maxk, k_cgf_raw);
}

}  // extern "C"
