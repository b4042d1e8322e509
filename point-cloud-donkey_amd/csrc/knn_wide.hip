// knn_wide.hip — the codeword search for rows of 1345 to ISMHIP_KNN_MAX_DIM (2048) floats: USC-1960. An exact scan of
// its own, apart from the three-stage search of knn.hip, so that no kernel serving dim_pad <= 1344 grows by a register or an LDS byte:
// the term buffers of the re-rank and scan kernels (s_terms[4][KNN_TERMS]) decide their occupancy and stay as they are.
//
// k_knn_wide: one WORKGROUP per (query, row range). The query lies zero padded in LDS; each of the four waves takes four codeword
// rows per step, 16 lanes a row with 16-byte loads, and forms the direct sum of (a-b)^2 [/(a+b)] in an order of its own. A row whose
// direct sum cannot exceed the wave's k-th best exact value by more than the two sums' rounding is evaluated with wave_functor -- the
// FLANN functor in its summation order, the value every other route of ismhip_knn reports -- and enters the wave's k best (distance,
// row) keys. k_knn_wide_merge: one wave per query folds the keys of its row ranges and waves; equal distances go to the lowest row.
//
// The filter. Both sums add the same non-negative terms t_i (each the correctly rounded result of the same float operations;
// -ffp-contract=off). With S their exact sum, a sum of n such terms in ANY order is within (n - 1) u S of it, u = 2^-24. The functor value F
// adds dim terms (chi-square) or dim / 4 group sums of four (squared L2): |F - S| <= (dim + 2) u S. The direct sum P adds at most dim_pad / 16
// terms per lane and four tree levels: |P - S| <= (dim_pad / 16 + 4) u S. A row with F <= thr therefore has P <= thr (1 + slack) for
// slack = 1.01 (dim + dim_pad / 16 + 8) u (1.4e-4 at 2048; the 1.01 and the + 2 cover the second order and the rounding of the product
// thr (1 + slack)). NaN compares unordered and counts as a hit, as does a direct sum that overflowed.
#include "knn_internal.h"

namespace {

#define KNN_WIDE_ROWS_MIN 64        // rows of the shortest range a query's scan is cut into
#define KNN_WIDE_UNITS 4096u        // (query, range) units wanted of a launch: four workgroups per CU by LDS, four rounds of the chip

template <int KM>   // KM = capacity of the result lists: 4 (k <= 4) or KNN_MAX_K
__global__ __launch_bounds__(256) void k_knn_wide(const float* __restrict__ words, int dim, int dim_pad, int n_words,
                                                  const float* __restrict__ q, int nq, int metric, int k, uint32_t P, float slack,
                                                  unsigned long long* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_q[ISMHIP_KNN_MAX_DIM];
    __shared__ __attribute__((aligned(16))) float s_terms[4][ISMHIP_KNN_MAX_DIM];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const bool l2 = metric != ISMHIP_METRIC_CHI2;
    const int n4 = dim_pad >> 2;
    const uint32_t n_units = (uint32_t)nq * P;
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const uint32_t qi = u / P, part = u % P;
        __syncthreads();                                                   // the previous unit's readers are done with s_q
        for (int i = threadIdx.x; i < dim_pad; i += 256) s_q[i] = i < dim ? q[(size_t)qi * dim + i] : 0.f;
        __syncthreads();
        const int r_beg = (int)((long long)n_words * part / P), r_end = (int)((long long)n_words * (part + 1) / P);
        unsigned long long best[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j) best[j] = ~0ull;
        float thr = __builtin_inff();
        for (int r0 = r_beg + 4 * wv; r0 < r_end; r0 += 16) {
            const int r = r0 + g;
            const bool live = r < r_end;
            float part_sum = 0.f;
            if (live) {
                const float* wp = words + (size_t)r * dim_pad;
                for (int c = l16; c < n4; c += 16) {
                    const f32x4 a = *(const f32x4*)(s_q + 4 * c), w = *(const f32x4*)(wp + 4 * c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float df = a[e] - w[e];
                        if (l2) part_sum += df * df;
                        else { const float sm = a[e] + w[e]; part_sum += sm > 0.f ? df * df / sm : 0.f; }
                    }
                }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) part_sum += __shfl_xor(part_sum, o, 64);
            const bool hit = live && (!(part_sum > thr * (1.f + slack) + 1e-30f) || part_sum == __builtin_inff());
            unsigned long long hm = __ballot(hit && l16 == 0);
            while (hm) {
                const int src = __ffsll((long long)hm) - 1; hm &= hm - 1;
                const int rr = __shfl(r, src, 64);
                const float d = wave_functor(metric, s_q, words + (size_t)rr * dim_pad, dim, lane, s_terms[wv]);
                unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)rr;
                if (d != d) key = (0x7fc00000ull << 32) | (unsigned)rr;             // NaN sorts after every finite distance and keeps ITS row
#pragma unroll
                for (int j = 0; j < KM; ++j) if (j < k && key < best[j]) { const unsigned long long tmp = best[j]; best[j] = key; key = tmp; }
                unsigned long long kth = ~0ull;
#pragma unroll
                for (int j = 0; j < KM; ++j) if (j == k - 1) kth = best[j];
                if (kth != ~0ull) thr = fminf(thr, __uint_as_float((unsigned)(kth >> 32)));
            }
        }
#pragma unroll
        for (int j = 0; j < KM; ++j) if (lane == j) out[((size_t)u * 4 + wv) * KM + j] = best[j];
    }
}

// one wave per query: every lane folds its share of the 4 P lists into a sorted private list, then k rounds of a wave-wide minimum.
// A row lies in one range and one wave's rows only, so no key comes twice.
template <int KM>
__global__ __launch_bounds__(256) void k_knn_wide_merge(int nq, int k, uint32_t P, const unsigned long long* __restrict__ in,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    unsigned long long fin[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) fin[j] = ~0ull;
    const unsigned long long* src = in + (size_t)qi * P * 4 * KM;
    for (uint32_t i = lane; i < P * 4 * KM; i += 64) {
        unsigned long long key = src[i];
#pragma unroll
        for (int j = 0; j < KM; ++j) if (key < fin[j]) { const unsigned long long tmp = fin[j]; fin[j] = key; key = tmp; }
    }
    for (int j = 0; j < k; ++j) {
        const unsigned long long mn = wave_min_u64(fin[0]);
        if (lane == 0) {
            if (mn == ~0ull) { idx_out[(size_t)qi * k + j] = -1; dist_out[(size_t)qi * k + j] = __builtin_nanf(""); }
            else { idx_out[(size_t)qi * k + j] = (int)(mn & 0xffffffffull); dist_out[(size_t)qi * k + j] = __uint_as_float((unsigned)(mn >> 32)); }
        }
        if (mn != ~0ull && fin[0] == mn) {
#pragma unroll
            for (int x = 0; x < KM; ++x) fin[x] = x + 1 < KM ? fin[x + 1] : ~0ull;
        }
    }
}

// k_km_closest of kmeans.hip (the centre choosers of ismhip_kmeans) with a term buffer for rows of up to ISMHIP_KNN_MAX_DIM floats
#include "km_closest.h"
__global__ __launch_bounds__(256) void k_km_closest_wide(int n, int dim, int metric, const float* __restrict__ desc, const uint32_t* __restrict__ chosen, int step,
                                                         float* __restrict__ closest, unsigned long long* __restrict__ slot) {
    __shared__ __attribute__((aligned(16))) float s_terms[4][ISMHIP_KNN_MAX_DIM];
    __shared__ unsigned long long s_best[4];
    km_closest(n, dim, metric, desc, chosen, step, closest, slot, s_terms[threadIdx.x >> 6], s_best);
}

}  // namespace

void km_closest_wide_launch(hipStream_t st, unsigned grid, int n, int dim, int metric, const float* desc, const uint32_t* chosen, int step, float* closest,
                            unsigned long long* slot) {
    hipLaunchKernelGGL(k_km_closest_wide, dim3(grid), dim3(256), 0, st, n, dim, metric, desc, chosen, step, closest, slot);
}

int run_knn_wide(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k, int32_t* idx_out, float* dist_out) {
    if (cb->dim_pad > ISMHIP_KNN_MAX_DIM) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn: descriptor longer than 2048 not built");
    const int KM = k <= 4 ? 4 : KNN_MAX_K;
    // few queries: every query's rows are cut into P ranges so that the launch fills the chip
    uint32_t P = (KNN_WIDE_UNITS + (uint32_t)nq - 1) / (uint32_t)nq;
    const uint32_t p_max = (uint32_t)std::max(1, cb->n_words / KNN_WIDE_ROWS_MIN);
    P = std::max(1u, std::min(P, p_max));
    const size_t n_units = (size_t)nq * P;
    unsigned long long* keys = (unsigned long long*)ism_scratch(ctx, SCR_KNN_CAND_VAL, n_units * 4 * KM * sizeof(unsigned long long));
    if (!keys) return ISMHIP_ERR_NOMEM;
    const float slack = 1.01f * (float)(cb->dim + cb->dim_pad / 16 + 8) * KNN_U;
    TimerScope ts(ctx, "knn_wide");
    const unsigned grid = (unsigned)std::min<size_t>(n_units, 4 * KNN_WIDE_UNITS);
    const auto scan = KM == 4 ? k_knn_wide<4> : k_knn_wide<KNN_MAX_K>;
    const auto merge = KM == 4 ? k_knn_wide_merge<4> : k_knn_wide_merge<KNN_MAX_K>;
    hipLaunchKernelGGL(scan, dim3(grid), dim3(256), 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words, q, nq, metric, k, P, slack, keys);
    ISM_CHECK_LAUNCH(ctx, "k_knn_wide");
    hipLaunchKernelGGL(merge, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, nq, k, P, keys, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_wide_merge");
    return ISMHIP_OK;
}
