// esf.hip — the ESF_LOCAL descriptor (Features type "ESF_LOCAL"), 640 floats: the "ensemble of shape functions" of the Radius ball round
// every keypoint. Reference seam: FeaturesESFLocal::iComputeDescriptors (features/features_esf_local.cpp:28-100) copies each ball into a cloud of
// its own and calls PCL 1.10 ESFEstimation (computeESF, lci, voxelize9, scale_points_unit_sphere), which draws with an unseeded rand(). PCL
// is external: the arithmetic is this library's definition with its named deviations (include/ismhip.h; restated in
// tests/esf_ref.py).
//
// One launch under the timer "esf_local": k_esf_local, ONE WORKGROUP of 256 threads per keypoint, a fixed number of workgroups that walk
// the keypoints with the stride of the launch (each owns one slab of the HBM work list).
//   1 gather   the object's points are scanned IN CLOUD ORDER, 256 at a time; the ordered compaction of common.h (BlockRank) numbers the
//              ball's points 0..n-1 in ascending cloud index without a sort and without the search grid, so the row cannot depend on the
//              grid's cell size. The scan costs (object points / 256) steps per keypoint: about 1 % of the line walks below at 16 384
//              points per object. The centroid's sums are 64-bit fixed point (order free, as rift.hip / iss3d.hip).
//   2 stage    the first `cap` points of the ball (ESF_CAP = 1024; env ISMHIP_ESF_CAP lowers it, for the tests) live in LDS: scaled
//              coordinates and packed voxel. Nothing is truncated: the ball's cloud indices were also written to the workgroup's slab
//              of the work list, and a draw past the staged points reads its point through that list and scales it again with the same
//              device function, hence to the same bits. A ball of n points finds cap / n of its draws in LDS.
//   3 voxels   64 x 64 x 64 occupancy BITS (32 KiB), up to 27 ds_or_b32 per point.
//   4 draws    attempts are handed out in blocks of 256, one per thread; the stream is a counter hash of (seed, t), so a block is
//              evaluated without state and BlockRank gives every accepted attempt its rank in order of t: "the first n_samples accepted
//              attempts" holds for any block size. The sequence runs TWICE: pass 1 finds the two maxima that the D2 and D3 bins are scaled
//              by (no line walk, no arc cosine), pass 2 replays it, walks the three lines of every sample through the bit set (integer Bresenham, one
//              ds_read_b32 per cell) and adds the integer numerators to 640 LDS bins (ds_add_u32).
//   5 row      row[i] = (float)N_i / (float)sum N: one rounding from exact integers.
// LDS per workgroup: 32 768 (bits) + 16 384 (1024 staged points x 16 bytes) + 2 560 (bins) + 64 (scan and reduction slots) = 51 776 bytes
// static, so THREE workgroups share the 160 KiB of a CU (12 waves). 256 threads, not 512 or 1024: the LDS, not the wave count, caps the
// residency either way (three workgroups), the two barriers of every attempt block stall fewer waves, and a smaller block overshoots the
// last accepted sample by fewer attempts. The walks are dependent integer arithmetic and scattered 4-byte LDS reads (bank conflicts of a
// random gather, about 3-way); no HBM traffic after the gather for the draws that fall on staged points.
// Integer counts, float maxima and fixed-point sums only: two calls, any cell size and any staging capacity give the same bytes.
#include "common.h"
#include <cfloat>
#include <cmath>
#include <cstdlib>

namespace {

#define ESF_CAP    1024                              // ball points staged in LDS
#define ESF_NT     256
#define ESF_BINS   64
#define ESF_WORDS  (64 * 64 * 64 / 32)
#define ESF_MAX_WG 768                               // 3 workgroups on each of 256 CUs
static_assert(ISMHIP_ESF_DIM == 10 * ESF_BINS, "ESF layout");

struct EsfArgs {
    const uint32_t* pt_off; const float *x, *y, *z;
    const uint32_t* kp_off; const float *kx, *ky, *kz;
    float r2;
    int e1;                                           // every |p - q| of a ball < 2^e1
    uint32_t n_samples, seed, cap;
    uint32_t k0, k1;                                  // the keypoints of the call
    int n_obj;
    uint32_t* list; size_t list_stride;               // the HBM work list: one slab of list_stride cloud indices per workgroup
    float* desc; uint32_t *count, *bins; float* scale;
};

__device__ __forceinline__ long long esf_on_grid(double v, double magic) { return __double_as_longlong(v + magic) - __double_as_longlong(magic); }
// h(seed, x) as include/ismhip.h writes it out
__device__ __forceinline__ uint32_t esf_hash(uint32_t seed, uint32_t x) {
    uint32_t v = x * 0x9E3779B1u + seed;
    v ^= v >> 16; v *= 0x7FEB352Du;
    v ^= v >> 15; v *= 0x846CA68Bu;
    v ^= v >> 16;
    return v;
}

// step 3 and 4 of the definition for one coordinate / one point
__device__ __forceinline__ float esf_scaled(float p, float c, float s) { return (p - c) * s; }
__device__ __forceinline__ int esf_cell(float g) {
    const float v = g < 0.f ? floorf(g) + 32.f : ceilf(g) + 31.f;
    return v < 0.f ? 0 : (v > 63.f ? 63 : (int)v);   // the clamp (deviation); g is finite
}
__device__ __forceinline__ uint32_t esf_voxel(float gx, float gy, float gz) {
    return ((uint32_t)esf_cell(gx) << 12) | ((uint32_t)esf_cell(gy) << 6) | (uint32_t)esf_cell(gz);
}

// the ball's points 0..n-1: the first ns staged (LDS), the others through the work list
struct EsfPts {
    const float *gx, *gy, *gz; const uint32_t* vox;   // staged: scaled coordinates and packed voxel
    const float *x, *y, *z; const uint32_t* list;     // listed: the object's coordinates and the ball's cloud indices
    float cx, cy, cz, s;
    uint32_t ns;
    __device__ __forceinline__ void get(uint32_t j, float& px, float& py, float& pz, uint32_t& v) const {
        if (j < ns) { px = gx[j]; py = gy[j]; pz = gz[j]; v = vox[j]; return; }
        const uint32_t i = list[j];
        px = esf_scaled(x[i], cx, s); py = esf_scaled(y[i], cy, s); pz = esf_scaled(z[i], cz, s);
        v = esf_voxel(px, py, pz);
    }
};

struct EsfTri { float a, b, c, H; int th[3]; uint32_t v[3]; };

// The angle bin of two normalised sides; false when it is outside 0..63. BIN false (pass 1 wants the verdict only): acosf of a cosine in
// [0, 1] lies in [0, pi/2 (1 + 2^-23)], which the written operations take to a bin 0..63, and a cosine above 1 or a NaN gives a NaN, so
// the verdict is "|dot| <= 1" without the arc cosine.
template <bool BIN>
__device__ __forceinline__ bool esf_angle(float ux, float uy, float uz, float wx, float wy, float wz, int& th) {
    const float dot = (ux * wx + uy * wy) + uz * wz;
    if (!BIN) return fabsf(dot) <= 1.0f;
    const float f = floorf(acosf(fabsf(dot)) / 1.57079632679489661923f * 63.0f + 0.5f);
    th = (int)f;
    return f >= 0.f && f <= 63.f;                     // a NaN fails
}

// attempt t of a ball of n points: false when it is rejected (step 5); BIN: with the three angle bins
template <bool BIN>
__device__ __forceinline__ bool esf_attempt(const EsfPts& P, uint32_t seed, uint32_t t, uint32_t n, EsfTri& T) {
    const uint32_t i1 = __umulhi(esf_hash(seed, 3u * t), n), i2 = __umulhi(esf_hash(seed, 3u * t + 1u), n), i3 = __umulhi(esf_hash(seed, 3u * t + 2u), n);
    if (i1 == i2 || i1 == i3 || i2 == i3) return false;
    float x1, y1, z1, x2, y2, z2, x3, y3, z3;
    P.get(i1, x1, y1, z1, T.v[0]); P.get(i2, x2, y2, z2, T.v[1]); P.get(i3, x3, y3, z3, T.v[2]);
    float ax = x2 - x1, ay = y2 - y1, az = z2 - z1;   // v21
    float bx = x3 - x1, by = y3 - y1, bz = z3 - z1;   // v31
    float cx = x2 - x3, cy = y2 - y3, cz = z2 - z3;   // v23
    T.a = sqrtf((ax * ax + ay * ay) + az * az);
    T.b = sqrtf((bx * bx + by * by) + bz * bz);
    T.c = sqrtf((cx * cx + cy * cy) + cz * cz);
    const float s = ((T.a + T.b) + T.c) * 0.5f;
    T.H = ((s * (s - T.a)) * (s - T.b)) * (s - T.c);
    if (!(T.H > 0.001f) || !isfinite(T.H)) return false;
    ax /= T.a; ay /= T.a; az /= T.a; bx /= T.b; by /= T.b; bz /= T.b; cx /= T.c; cy /= T.c; cz /= T.c;
    const bool k1 = esf_angle<BIN>(ax, ay, az, bx, by, bz, T.th[0]);
    const bool k2 = esf_angle<BIN>(cx, cy, cz, bx, by, bz, T.th[1]);
    const bool k3 = esf_angle<BIN>(cx, cy, cz, ax, ay, az, T.th[2]);
    return k1 && k2 && k3;
}

// PCL's lci: the 3-D Bresenham line from voxel va towards voxel vb over the bit set. The driving axis is the longest (ties x, y, z), L its
// length: the cells at steps 0 .. max(L, 1) - 1 are visited, so the walk ends one step short of vb. Every cell lies in the box of
// the two ends, which are inside the set.
__device__ __forceinline__ void esf_walk(const uint32_t* occ, uint32_t va, uint32_t vb, int& visited, int& inside) {
    const int dx = (int)(vb >> 12) - (int)(va >> 12), dy = (int)((vb >> 6) & 63u) - (int)((va >> 6) & 63u), dz = (int)(vb & 63u) - (int)(va & 63u);
    const int l = abs(dx), m = abs(dy), n = abs(dz);
    const int sx = dx < 0 ? -4096 : 4096, sy = dy < 0 ? -64 : 64, sz = dz < 0 ? -1 : 1;
    int L, d1, d2, sL, s1, s2;
    if (l >= m && l >= n) { L = l; d1 = m; d2 = n; sL = sx; s1 = sy; s2 = sz; }
    else if (m >= l && m >= n) { L = m; d1 = l; d2 = n; sL = sy; s1 = sx; s2 = sz; }
    else { L = n; d1 = m; d2 = l; sL = sz; s1 = sy; s2 = sx; }
    int idx = (int)va, e1 = 2 * d1 - L, e2 = 2 * d2 - L, in = 0;
    for (int i = 1; i < L; ++i) {
        in += (int)((occ[idx >> 5] >> (idx & 31)) & 1u);
        if (e1 > 0) { idx += s1; e1 -= 2 * L; }
        if (e2 > 0) { idx += s2; e2 -= 2 * L; }
        e1 += 2 * d1; e2 += 2 * d2; idx += sL;
    }
    in += (int)((occ[idx >> 5] >> (idx & 31)) & 1u);
    visited = L > 1 ? L : 1;
    inside = in;
}

// 51 776 bytes of static LDS (head of the file)
__global__ __launch_bounds__(ESF_NT) void k_esf_local(EsfArgs a) {
    __shared__ uint32_t s_occ[ESF_WORDS];
    __shared__ float s_g[3][ESF_CAP];
    __shared__ uint32_t s_vox[ESF_CAP];
    __shared__ uint32_t s_bins[ISMHIP_ESF_DIM];
    __shared__ BlockRank<ESF_NT> s_rank;
    __shared__ unsigned long long s_red64[ESF_NT / 64];
    __shared__ uint32_t s_red[ESF_NT / 64];
    const uint32_t tid = threadIdx.x;
    const float nanf_ = __builtin_nanf("");
    uint32_t* list = a.list ? a.list + (size_t)blockIdx.x * a.list_stride : nullptr;
    for (uint32_t k = a.k0 + blockIdx.x; k < a.k1; k += gridDim.x) {
        // the keypoint's object: the last o with kp_off[o] <= k
        int o = 0;
        for (int hi = a.n_obj; hi - o > 1;) { const int mid = (o + hi) >> 1; if (a.kp_off[mid] <= k) o = mid; else hi = mid; }
        const uint32_t base = a.pt_off[o], npts = a.pt_off[o + 1] - base;
        const float* X = a.x + base; const float* Y = a.y + base; const float* Z = a.z + base;
        const float qx = a.kx[k], qy = a.ky[k], qz = a.kz[k];
        float* row = a.desc + (size_t)k * ISMHIP_ESF_DIM;
        uint32_t n = 0;
        float cx = nanf_, cy = nanf_, cz = nanf_, mx = nanf_;
        bool ok = isfinite(qx) && isfinite(qy) && isfinite(qz);
        // ---- 1 gather: the ball in ascending cloud index, the centroid's fixed-point sums ------------------------------------------
        if (ok) {
            int bits = 40;                                               // 2^(62 - bits) terms fit
            while (bits > 24 && ((unsigned long long)npts + 1ull) >= (1ull << (62 - bits))) --bits;
            const double magic = ldexp(1.5, a.e1 - bits + 52), quantum = ldexp(1.0, a.e1 - bits);
            long long sx = 0, sy = 0, sz = 0;
            for (uint32_t i0 = 0; i0 < npts; i0 += ESF_NT) {
                const uint32_t i = i0 + tid;
                float px = 0.f, py = 0.f, pz = 0.f;
                bool in = false;
                if (i < npts) {
                    px = X[i]; py = Y[i]; pz = Z[i];
                    in = isfinite(px) && isfinite(py) && isfinite(pz) && sqdist3(px, py, pz, qx, qy, qz) < a.r2;
                }
                const uint32_t at = s_rank.step(in, n);
                if (in) {
                    if (at < a.cap) { s_g[0][at] = px; s_g[1][at] = py; s_g[2][at] = pz; }
                    if (list) list[at] = i;                              // at < npts <= list_stride
                    sx += esf_on_grid((double)px - (double)qx, magic);
                    sy += esf_on_grid((double)py - (double)qy, magic);
                    sz += esf_on_grid((double)pz - (double)qz, magic);
                }
            }
            const long long tx = (long long)block_sum_u64((unsigned long long)sx, s_red64);
            const long long ty = (long long)block_sum_u64((unsigned long long)sy, s_red64);
            const long long tz = (long long)block_sum_u64((unsigned long long)sz, s_red64);
            if (n >= 3) {
                cx = (float)((double)qx + ((double)tx * quantum) / (double)n);
                cy = (float)((double)qy + ((double)ty * quantum) / (double)n);
                cz = (float)((double)qz + ((double)tz * quantum) / (double)n);
            }
        }
        ok = ok && n >= 3;
        const uint32_t ns = n < a.cap ? n : a.cap;                        // staged; n > cap needs the list: the host made one whenever an object is that large
        // ---- 2 the scale --------------------------------------------------------------------------------------------------------------
        float s = 0.f;
        if (ok) {                                                         // uniform: n and the keypoint are
            uint32_t best = 0u;
            for (uint32_t j = tid; j < n; j += ESF_NT) {
                float px, py, pz;
                if (j < ns) { px = s_g[0][j]; py = s_g[1][j]; pz = s_g[2][j]; }
                else { const uint32_t i = list[j]; px = X[i]; py = Y[i]; pz = Z[i]; }
                const float dx = px - cx, dy = py - cy, dz = pz - cz;
                const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
                best = max(best, __float_as_uint(d));                     // d >= 0 or NaN (above every number): bits order as values
            }
            best = block_max_u32(best, s_red);
            mx = __uint_as_float(best);
            s = 32.0f / mx;
            ok = mx > 0.f && isfinite(mx) && isfinite(s);
        }
        if (a.count && tid == 0) a.count[k] = n;
        if (a.scale && tid == 0) { float* sc = a.scale + (size_t)k * 4; sc[0] = cx; sc[1] = cy; sc[2] = cz; sc[3] = mx; }
        // ---- 3 voxels -----------------------------------------------------------------------------------------------------------------
        uint32_t limit = 0, need = a.n_samples;
        EsfPts P = {s_g[0], s_g[1], s_g[2], s_vox, X, Y, Z, list, cx, cy, cz, s, ns};
        if (ok) {
            for (uint32_t i = tid; i < ESF_WORDS; i += ESF_NT) s_occ[i] = 0u;
            for (uint32_t i = tid; i < ISMHIP_ESF_DIM; i += ESF_NT) s_bins[i] = 0u;
            __syncthreads();
            for (uint32_t j = tid; j < n; j += ESF_NT) {
                float px, py, pz;
                if (j < ns) { px = s_g[0][j]; py = s_g[1][j]; pz = s_g[2][j]; }
                else { const uint32_t i = list[j]; px = X[i]; py = Y[i]; pz = Z[i]; }
                const float gx = esf_scaled(px, cx, s), gy = esf_scaled(py, cy, s), gz = esf_scaled(pz, cz, s);
                const uint32_t v = esf_voxel(gx, gy, gz);
                if (j < ns) { s_g[0][j] = gx; s_g[1][j] = gy; s_g[2][j] = gz; s_vox[j] = v; }   // thread-private slots
                const int vx = (int)(v >> 12), vy = (int)((v >> 6) & 63u), vz = (int)(v & 63u);
                for (int ix = -1; ix <= 1; ++ix)
                    for (int iy = -1; iy <= 1; ++iy)
                        for (int iz = -1; iz <= 1; ++iz) {
                            const int x = vx + ix, y = vy + iy, z = vz + iz;
                            if ((unsigned)x > 63u || (unsigned)y > 63u || (unsigned)z > 63u) continue;
                            const int idx = (x * 64 + y) * 64 + z;
                            atomicOr(&s_occ[idx >> 5], 1u << (idx & 31));
                        }
            }
            __syncthreads();
            limit = 8u * a.n_samples;
        }
        // ---- 4 draws, pass 1: the maxima of the distances and of the fourth roots of H over the samples ------------------------------------
        uint32_t acc = 0, blocks = 0, bd = 0u, bd3 = 0u;
        for (uint32_t t0 = 0; t0 < limit && acc < need; t0 += ESF_NT, ++blocks) {
            const uint32_t t = t0 + tid;
            EsfTri T;
            const bool good = t < limit && esf_attempt<false>(P, a.seed, t, n, T);
            const uint32_t rk = s_rank.step(good, acc);
            if (good && rk < need) {
                bd = max(bd, __float_as_uint(fmaxf(fmaxf(T.a, T.b), T.c)));
                bd3 = max(bd3, __float_as_uint(sqrtf(sqrtf(T.H))));
            }
        }
        ok = ok && acc >= need;                                           // the attempt cap (deviation)
        const float maxd = __uint_as_float(block_max_u32(bd, s_red)), maxd3 = __uint_as_float(block_max_u32(bd3, s_red));
        // ---- pass 2: the same sequence again, the line walks and the deposits -----------------------------------------------------------
        if (!ok) blocks = 0;
        acc = 0;
        for (uint32_t b = 0; b < blocks; ++b) {
            const uint32_t t = b * ESF_NT + tid;
            EsfTri T;
            const bool good = t < limit && esf_attempt<true>(P, a.seed, t, n, T);
            const uint32_t rk = s_rank.step(good, acc);
            if (!(good && rk < need)) continue;                           // no barrier below
            const float dist[3] = {T.a, T.b, T.c};
            const uint32_t from[3] = {T.v[0], T.v[0], T.v[1]}, to[3] = {T.v[1], T.v[2], T.v[2]};
            int sum_in = 0, sum_vis = 0;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                int vis, in;
                esf_walk(s_occ, from[e], to[e], vis, in);
                sum_in += in; sum_vis += vis;
                const int cls = in >= vis - 1 ? 0 : (in <= 7 ? 1 : 2);
                if (cls == 2) {
                    const float ratio = (float)in / (float)vis;
                    atomicAdd(&s_bins[9 * ESF_BINS + (int)floorf(ratio * 63.0f + 0.5f)], 6u);
                }
                const int bin = (int)floorf(dist[e] / maxd * 63.0f + 0.5f);   // dist <= maxd: 0..63
                atomicAdd(&s_bins[(6 + cls) * ESF_BINS + bin], cls == 0 ? 3u : 12u);
            }
            const int tc = sum_in <= 21 ? 1 : (sum_vis - sum_in < 4 ? 0 : 2);
#pragma unroll
            for (int e = 0; e < 3; ++e) atomicAdd(&s_bins[tc * ESF_BINS + T.th[e]], 1u);
            const int bin3 = (int)floorf(sqrtf(sqrtf(T.H)) / maxd3 * 63.0f + 0.5f);
            atomicAdd(&s_bins[(3 + tc) * ESF_BINS + bin3], tc == 2 ? 6u : 3u);
        }
        __syncthreads();
        // ---- 5 the row ------------------------------------------------------------------------------------------------------------------
        uint32_t part = 0;
        if (ok)
            for (uint32_t i = tid; i < ISMHIP_ESF_DIM; i += ESF_NT) part += s_bins[i];
        const uint32_t sum = block_sum_i(part, s_red);
        for (uint32_t i = tid; i < ISMHIP_ESF_DIM; i += ESF_NT) {
            const uint32_t c = ok ? s_bins[i] : 0u;
            row[i] = ok ? (float)c / (float)sum : nanf_;
            if (a.bins) a.bins[(size_t)k * ISMHIP_ESF_DIM + i] = c;
        }
        __syncthreads();                                                  // the LDS and the list serve the next keypoint
    }
}

}  // namespace

extern "C" int ismhip_esf_local(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                                const float* kpx, const float* kpy, const float* kpz, float radius, int n_samples, uint32_t seed,
                                float* desc_out, uint32_t* neighbour_count_out, uint32_t* bin_counts_out, float* scale_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !desc_out || !(radius > 0.f) || !std::isfinite(radius) || n_samples < 1 ||
        n_samples > 65536)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "esf_local: bad argument");
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, "esf_local", kp_offsets_h, cloud->n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK || kp.max_run == 0) return rc;
    EsfArgs a = {};
    a.pt_off = cloud->pt_off; a.x = cloud->x; a.y = cloud->y; a.z = cloud->z;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz;
    a.r2 = (float)((double)radius * (double)radius);
    if (!(a.r2 > 0.f) || !std::isfinite(a.r2)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "esf_local: bad argument");
    (void)std::frexp(radius, &a.e1);
    a.e1 += 1;                                                            // |p - q| <= sqrt(d2) (1 + 2^-22) < R (1 + 2^-21) < 2^e1
    a.n_samples = (uint32_t)n_samples; a.seed = seed;
    a.cap = ESF_CAP;
    if (const char* e = getenv("ISMHIP_ESF_CAP")) {                       // tests: the listed path at small n
        const long v = atol(e);
        if (v > 0) a.cap = (uint32_t)(v > ESF_CAP ? ESF_CAP : v);
    }
    a.k0 = kp_offsets_h[0]; a.k1 = kp_offsets_h[cloud->n_obj];
    a.n_obj = cloud->n_obj;
    a.desc = desc_out; a.count = neighbour_count_out; a.bins = bin_counts_out; a.scale = scale_out;
    uint32_t n_wg = a.k1 - a.k0 < ESF_MAX_WG ? a.k1 - a.k0 : ESF_MAX_WG;
    if (cloud->max_pts > a.cap) {                                         // a ball may outgrow the staging: one slab per workgroup, 256 MiB at most
        const size_t slab = (size_t)cloud->max_pts * sizeof(uint32_t);
        const size_t fit = ((size_t)256 << 20) / slab;
        if (n_wg > fit) n_wg = fit < 1 ? 1u : (uint32_t)fit;
        a.list = (uint32_t*)ism_scratch(ctx, SCR_ESF_LIST, (size_t)n_wg * slab);
        if (!a.list) return ISMHIP_ERR_NOMEM;
        a.list_stride = cloud->max_pts;
    }
    TimerScope ts(ctx, "esf_local");
    hipLaunchKernelGGL(k_esf_local, dim3(n_wg), dim3(ESF_NT), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_esf_local");
    return ISMHIP_OK;
}
