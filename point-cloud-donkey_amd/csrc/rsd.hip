// rsd.hip — the RSD descriptor (Features type "RSD"): over every unordered PAIR of the keypoint's neighbours, the 5 x 5 histogram of
// (angle between the two normals, distance between the two points), 25 floats, or the two principal radii fitted to the angle range of
// every distance bin, 2 floats. Reference seam: FeaturesRSD::iComputeDescriptors (features/features_rsd.cpp:29-103) -> PCL 1.10
// RSDEstimation::computeFeature / computeRSD as :41-56 configure it (5 subdivisions, max_dist = the search radius, plane_radius =
// Radius), then normalizeDescriptors (features/features.cpp:282-297) for the histogram. Definition and the five named deviations:
// DESIGN.md 4.16; the restatement is tests/rsd_ref.py.
//
// One launch under the timer "rsd": k_rsd<FULL>, one wavefront per keypoint in cell order (shot_wave.h), four per workgroup.
//   - the ball sweep hands its neighbours over 64 at a time; the wave reads their position and normal records by the queued index
//     and STAGES them SoA in its LDS, up to `cap` of them (RSD_CAP = 256; env ISMHIP_RSD_CAP lowers it, for the tests);
//   - the pairs INSIDE the staged tile by the circular mapping: lane i keeps neighbour i in registers and, for the offset
//     s = 1 .. n / 2, takes the pair (i, (i + s) mod n) -- for even n the last offset only for i < n / 2 -- so every unordered pair is
//     visited once, all lanes are busy and the 64 LDS reads of one offset are consecutive;
//   - more than `cap` neighbours: the pair triangle is TILED. The sweep hands the neighbours over in an order that is the same every
//     time the same wave repeats it, and `cap` is a multiple of the 64 of one hand-over, so tile t is the hand-overs
//     [t cap / 64, (t + 1) cap / 64). Sweep t stages tile t, and every LATER hand-over of the same sweep finds the tile complete: its
//     lanes keep one neighbour each and walk the whole tile (broadcast LDS reads). ceil(n / cap) sweeps, nothing spilled, nothing
//     truncated; which neighbour lands in which tile never shows, because the row is made of integer counts and float minima/maxima.
//   - per pair: c and d2 in unfused float, a = min(|c|, 1). The two bins are COUNTS OF THRESHOLDS PASSED (a against cos(k pi / 10),
//     d2 against (k R / 5)^2), taken twice, against the lower and the upper end of a guard band about every edge; where the two
//     counts differ the lane evaluates the defining double formulas (acos, sqrt, floor). No acos outside the band.
//   - histogram mode: one ds_add_u32 per pair into the lane's OWN column hist[bin][lane] (bank = lane: no conflict, no two lanes on one
//     address), the 64 columns summed once per keypoint. Radii mode: min and max of the bits of a (a >= 0: its bits order as its
//     value) per distance bin in registers, no LDS at all, a wave reduction per keypoint.
// Counts are uint32 (n (n - 1) / 2 < 2^32: n < 92 682 neighbours), no float atomics: two calls, any cell size and any `cap` give the
// same bytes.
#include "shot_wave.h"
#include <cfloat>

namespace {

#define RSD_CAP   256                                // neighbours of one staged tile; a multiple of 64
#define RSD_SUB   5                                  // PCL's nr_subdiv
#define RSD_BINS  ISMHIP_RSD_DIM
static_assert(RSD_BINS == RSD_SUB * RSD_SUB && RSD_CAP % 64 == 0, "RSD layout");

struct RsdArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *sn4;
    const uint32_t* kp_off; const float *kx, *ky, *kz;
    float radius, r2;
    float alo[RSD_SUB - 1], ahi[RSD_SUB - 1];         // cos(k pi / 10) -+ guard, k = 1..4
    float dlo[RSD_SUB], dhi[RSD_SUB];                 // (k R / 5)^2 (1 -+ guard), k = 1..5; k = 5: beyond it the pair is neglected
    double D;                                         // (double)radius
    uint32_t cap;
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;
};

template <bool FULL>
struct RsdSmem {
    float4 qd[4][128];                                // the sweep's queue (shot_wave.h)
    uint32_t qi[4][128];
    WaveRows rows[4];
    float st[4][6][RSD_CAP];                          // the staged tile: x, y, z, nx, ny, nz
    uint32_t hist[4][FULL ? RSD_BINS * 64 : 1];       // hist[bin][lane]
};
static_assert(sizeof(RsdSmem<true>) <= 65536, "k_rsd: static LDS");

// min and max of the bits of a per distance bin (radii mode)
struct RsdRange { uint32_t lo[RSD_SUB], hi[RSD_SUB]; };

// the bins of one pair by the definition, in double: bd = RSD_SUB says "neglected"
__device__ __forceinline__ void rsd_bins_exact(float av, float d2, double D, int& ba, int& bd) {
    const double theta = acos((double)av), dist = sqrt((double)d2);
    if (dist > D) bd = RSD_SUB;
    else { bd = (int)floor(5.0 * dist / D); bd = bd > RSD_SUB - 1 ? RSD_SUB - 1 : bd; }     // dist == D: the last bin
    ba = (int)floor(5.0 * theta / (3.14159265358979323846 / 2));
    ba = ba > RSD_SUB - 1 ? RSD_SUB - 1 : (ba < 0 ? 0 : ba);
}

// One pair of neighbours, (p, n) and (q, m). col: &hist[0][lane].
template <bool FULL>
__device__ __forceinline__ void rsd_pair(const RsdArgs& a, bool act, float px, float py, float pz, float nx, float ny, float nz,
                                         float qx, float qy, float qz, float mx, float my, float mz, uint32_t* col, RsdRange& rg) {
    const float c = (nx * mx + ny * my) + nz * mz;
    const float d2 = sqdist3(px, py, pz, qx, qy, qz);
    const float av = fminf(fabsf(c), 1.0f);
    if (!(act && isfinite(c) && isfinite(d2))) return;                  // deviation 3: a pair that is no number is no pair
    int ba = 0, ba2 = 0, bd = 0, bd2 = 0;
#pragma unroll
    for (int k = 0; k < RSD_SUB - 1; ++k) { ba += av <= a.alo[k] ? 1 : 0; ba2 += av <= a.ahi[k] ? 1 : 0; }
#pragma unroll
    for (int k = 0; k < RSD_SUB; ++k) { bd += d2 > a.dhi[k] ? 1 : 0; bd2 += d2 > a.dlo[k] ? 1 : 0; }
    if (ba != ba2 || bd != bd2) rsd_bins_exact(av, d2, a.D, ba, bd);   // inside a guard band
    if (bd >= RSD_SUB) return;                                          // farther apart than the radius
    if (FULL) atomicAdd(&col[(ba + RSD_SUB * bd) * 64], 1u);
    else {
        const uint32_t au = __float_as_uint(av);
#pragma unroll
        for (int k = 0; k < RSD_SUB; ++k)
            if (bd == k) { rg.lo[k] = min(rg.lo[k], au); rg.hi[k] = max(rg.hi[k], au); }
    }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return ~wave_max_u32(~v); }

// 64 512 bytes of static LDS per workgroup in histogram mode (queue 10 KiB, row tables 4 KiB, tiles 24 KiB, columns 25 KiB), 38 928 in
// radii mode
template <bool FULL>
__global__ __launch_bounds__(256) void k_rsd(RsdArgs a) {
    __shared__ RsdSmem<FULL> sm;
    ShotWave w;
    const int DIM = FULL ? ISMHIP_RSD_DIM : ISMHIP_RSD_RADII_DIM;
    if (!shot_wave_place(a, DIM, w)) return;
    if (!shot_wave_ball(a, DIM, w, true)) return;
    const int wv = w.wv, lane = w.lane;
    const uint32_t cap = a.cap;
    float* sx = sm.st[wv][0]; float* sy = sm.st[wv][1]; float* sz = sm.st[wv][2];
    float* snx = sm.st[wv][3]; float* sny = sm.st[wv][4]; float* snz = sm.st[wv][5];
    uint32_t* hist = sm.hist[wv];
    uint32_t* col = hist + (FULL ? lane : 0);
    if (FULL)
        for (int i = lane; i < RSD_BINS * 64; i += 64) hist[i] = 0u;
    RsdRange rg;
#pragma unroll
    for (int k = 0; k < RSD_SUB; ++k) { rg.lo[k] = 0xffffffffu; rg.hi[k] = 0u; }
    uint32_t total = 0;
    for (uint32_t t0 = 0; t0 == 0 || t0 < total; t0 += cap) {
        uint32_t seq = 0;                                                 // neighbours handed over so far in this sweep (wave-uniform)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the last tile has been read
        total = shot_wave_neighbours<16, true>(a, w, sm.qd[wv], sm.qi[wv], sm.rows[wv],
            [&](bool act, uint32_t gi, float, float, float, float) {
                const uint32_t s0 = seq;
                seq += 64;
                if (s0 < t0) return;                                      // an earlier tile's: their pairs with this tile are done
                const float4 p = a.sp4[gi], n = a.sn4[gi];               // an idle lane reads record 0
                if (s0 < t0 + cap) {                                      // this tile's: s0 - t0 + lane < cap <= RSD_CAP
                    if (act) {
                        const uint32_t at = s0 - t0 + (uint32_t)lane;
                        sx[at] = p.x; sy[at] = p.y; sz[at] = p.z; snx[at] = n.x; sny[at] = n.y; snz[at] = n.z;
                    }
                    return;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // a later tile's: the staged tile is complete, `cap` long
                for (uint32_t t = 0; t < cap; ++t)
                    rsd_pair<FULL>(a, act, p.x, p.y, p.z, n.x, n.y, n.z, sx[t], sy[t], sz[t], snx[t], sny[t], snz[t], col, rg);
            });
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the tile staged by the other lanes is read below
        const uint32_t n = min(total - t0, cap), half = n >> 1;          // the pairs inside the tile
        for (uint32_t i0 = 0; i0 < n && half > 0; i0 += 64) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool iv = i < n;
            const uint32_t ii = iv ? i : 0u;
            const float px = sx[ii], py = sy[ii], pz = sz[ii], nx = snx[ii], ny = sny[ii], nz = snz[ii];
            for (uint32_t s = 1; s <= half; ++s) {
                uint32_t j = ii + s;
                j = j >= n ? j - n : j;
                const bool act = iv && !((n & 1u) == 0u && s == half && i >= half);
                rsd_pair<FULL>(a, act, px, py, pz, nx, ny, nz, sx[j], sy[j], sz[j], snx[j], sny[j], snz[j], col, rg);
            }
        }
    }
    // No neighbour: the whole row NaN (deviation 1). One neighbour: no pair, a zero row in either mode.
    if (total < 2) {
        if (lane < DIM) w.row[lane] = total == 0 ? __builtin_nanf("") : 0.f;
        return;
    }
    if (FULL) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the counts of the other lanes are read below
        if (lane < RSD_BINS) {
            uint32_t s = 0;
            for (int l = 0; l < 64; ++l) s += hist[lane * 64 + ((l + lane) & 63)];   // rotated: the 25 lanes stay on 25 banks
            w.row[lane] = (float)s / 300.0f;                              // features.cpp:282-297: by the sum of the indices 0..24
        }
        return;
    }
    // The radii. Bin 0 starts at theta_min = theta_max = 0 (a = 1) as PCL initialises it; a bin without pairs is left out.
    const double D = a.D;
    double Amin2 = 0.0, Amind = 0.0, Amax2 = 0.0, Amaxd = 0.0;
#pragma unroll
    for (int k = 0; k < RSD_SUB; ++k) {
        uint32_t lo = wave_min_u32(rg.lo[k]), hi = wave_max_u32(rg.hi[k]);
        const bool any = lo != 0xffffffffu;
        if (k == 0) { const uint32_t one = __float_as_uint(1.0f); lo = min(lo, one); hi = max(hi, one); }
        if (k == 0 || any) {
            const double tmin = acos((double)__uint_as_float(hi)), tmax = acos((double)__uint_as_float(lo));
            const double f = ((double)k + 0.5) * D / 5.0;
            Amin2 += tmin * tmin; Amind += tmin * f;
            Amax2 += tmax * tmax; Amaxd += tmax * f;
        }
    }
    float r0 = Amin2 == 0.0 ? (float)D : (float)fmin(Amind / Amin2, D);
    float r1 = Amax2 == 0.0 ? (float)D : (float)fmin(Amaxd / Amax2, D);
    r0 *= 1.1f; r1 *= 1.1f;
    if (lane == 0) { w.row[0] = fminf(r0, r1); w.row[1] = fmaxf(r0, r1); }
}

}  // namespace

extern "C" int ismhip_rsd(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                          const float* kpx, const float* kpy, const float* kpz, float radius, int full_histogram,
                          float* desc_out, uint32_t* neighbour_count_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !desc_out || !(radius > 0.f) || !std::isfinite(radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rsd: bad argument");
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, "rsd", kp_offsets_h, cloud->n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK || kp.max_run == 0) return rc;
    const uint32_t maxk = kp.max_run;
    RsdArgs a = {};
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4; a.sn4 = cloud->sn4;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz;
    a.radius = radius; a.r2 = (float)((double)radius * (double)radius);
    a.D = (double)radius;
    a.desc = desc_out; a.count = neighbour_count_out;
    a.n_obj = ctx->xcd_map ? cloud->n_obj : 0; a.nbx = (int)((maxk + 3) / 4);
    // The guard bands. An edge in a: the floats are 6e-8 apart there and the double formula moves the edge by 1e-16: 1.5e-6 either side.
    // An edge in d2: relative 2e-6 either side of (k R / 5)^2. A radius so small or so large that a band does not enclose its edge in
    // float leaves every band open (lo = -1, hi = inf): every pair then takes the double formulas.
    for (int k = 1; k < RSD_SUB; ++k) {
        const double e = cos(k * 3.14159265358979323846 / 10.0);
        a.alo[k - 1] = (float)(e - 1.5e-6); a.ahi[k - 1] = (float)(e + 1.5e-6);
    }
    bool closed = true;
    for (int k = 1; k <= RSD_SUB; ++k) {
        const double r = k * a.D / 5.0, e = r * r;
        a.dlo[k - 1] = (float)(e * (1.0 - 2e-6)); a.dhi[k - 1] = (float)(e * (1.0 + 2e-6));
        closed = closed && a.dlo[k - 1] >= FLT_MIN && std::isfinite(a.dhi[k - 1]) && (double)a.dlo[k - 1] < e * (1.0 - 1e-6) &&
                 (double)a.dhi[k - 1] > e * (1.0 + 1e-6);
    }
    if (!closed)
        for (int k = 0; k < RSD_SUB; ++k) { a.dlo[k] = -1.0f; a.dhi[k] = INFINITY; }
    a.cap = RSD_CAP;
    if (const char* e = getenv("ISMHIP_RSD_CAP")) {                       // tests: the tiled path at small n; rounded down to whole hand-overs
        const long v = atol(e);
        if (v > 0) a.cap = (uint32_t)(v < 64 ? 64 : (v > RSD_CAP ? RSD_CAP : v / 64 * 64));
    }
    const ShotCall c = {ctx, cloud, kp_offsets_h, kpx, kpy, kpz, nullptr, nullptr, radius, desc_out, neighbour_count_out, "rsd"};
    return full_histogram ? shot_launch(c, a, maxk, k_rsd<true>, 0) : shot_launch(c, a, maxk, k_rsd<false>, 0);
}
