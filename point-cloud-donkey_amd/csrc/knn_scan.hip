// knn_scan.hip — stage 3 of the codeword search (map: knn.hip): the exact scan of what no proof covers, and THE layout of its queue.
#include "knn_internal.h"

namespace {

// Exact scan for the slots that could not be proven. One WAVE per (query, slot) work item; the wave handles 4 codeword rows
// per step (16 lanes each, 64-byte coalesced segments) with the query held in registers; direct (a-b)^2 [/(a+b)] sums pick
// the rows that can still matter, the FLANN functor order ranks them. Each item leaves its k best (distance,row) keys in
// item_out; k_knn_fallback_merge folds them into the query's result.
// Slot -> rows: L2 bit b = split*4 + wr*2 + h owns, in every tile of its split, the rows wr*wr_rows + x (x < wr_rows) with bit 2
// of x equal to h (the C/D layout of the 32x32 MFMA tile, see the candidate kernels); chi2 bit b = split owns all rows of its split.
#define KNN_FB_UNITS 8192u      // work units (item x row range) when items are few
__host__ __device__ inline uint32_t knn_fb_parts(uint32_t n_items) {
    if (n_items == 0 || n_items > KNN_FB_UNITS / 2) return 1u;
    const uint32_t p = KNN_FB_UNITS / n_items;
    return p > 256u ? 256u : p;
}
// (KnnSlotRows under the name the parameter had before the split: it is part of k_knn_fallback's mangled name, which tools and profiles key on)
struct KnnFbDesc : KnnSlotRows {};
// One launch scans the items of up to two searches that shared a queue: bit 8 of an item's slot word picks d1 (KnnQueueTag).
template <int KM>   // KM = capacity of the per-item result lists: 4 (k <= 4, every shipped configuration) or KNN_MAX_K
__global__ __launch_bounds__(256) void k_knn_fallback(const float* __restrict__ words, int dim, int dim_pad, int n_words,
                                                      const float* __restrict__ q, int ldq, int metric, int k, KnnFbDesc d0, KnnFbDesc d1,
                                                      const int* __restrict__ qrange,
                                                      const uint32_t* __restrict__ flag_count, const uint32_t* __restrict__ items,
                                                      const int32_t* __restrict__ idx_in, const float* __restrict__ dist_in,
                                                      unsigned long long* __restrict__ item_out, size_t part_base) {
    __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, l16 = lane & 15;
    const uint32_t n_items = flag_count[KNN_CNT_ITEMS];
    const bool l2 = metric != ISMHIP_METRIC_CHI2;
    const int nj = dim_pad / 16;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    // With few items a wave per item would leave the chip idle behind a handful of long scans: every item is cut into P row
    // ranges (P * n_items <= KNN_FB_UNITS), each range leaves its own k best in part_out and the merge kernel folds them.
    const uint32_t P = knn_fb_parts(n_items);
    unsigned long long* outp = P > 1 ? item_out + KM * part_base : item_out;
    for (uint32_t u = gw; u < n_items * P; u += nw) {
        const uint32_t it = u / P, part_i = u % P;
        const int qi = (int)items[2 * (size_t)it], bt = (int)items[2 * (size_t)it + 1], b = bt & 255;
        const KnnFbDesc d = (bt >> 8) ? d1 : d0;
        const int wr_rows = d.wr_rows, tile_rows = d.tile_rows;
        const bool lay_all = l2 && wr_rows == KNN_FB_ALL;                     // merged splits (k_knn_merge_splits): the one slot owns every row
        const bool lay16 = l2 && wr_rows == KNN_FB_RING;                       // k_knn_l2_ring16: slot b = split*8 + wr*4 + fq owns rows wr*128 + 16 m + 4 fq + j
        const bool lay16h = l2 && wr_rows == KNN_FB_RING_HALF;                      // k_knn_l2_ring16<T, 1>: 128-row tiles, slot b = split*4 + fq owns rows 16 m + 4 fq + j
        const int rows_per_tile = lay_all ? tile_rows : ((lay16 || lay16h) ? 32 : (l2 ? wr_rows / 2 : tile_rows));   // else a lane slot sees half of its wave-row block (bit 2 of the row == h)
        const float* qp = q + (size_t)qi * ldq;
        const int split = lay_all ? 0 : (lay16 ? (b >> 3) : (l2 ? (b >> 2) : b));
        const int wr = lay16h ? 0 : (lay16 ? (b >> 2) & 1 : (b >> 1) & 1), h = b & 1, fq = b & 3;
        int mt0 = split * d.tiles_per_split, mt1 = min(d.n_tiles, mt0 + d.tiles_per_split);
        if (qrange) {                                                          // ranged search: the query's own rows, cut as the candidate kernel cut them
            const int* rg = qrange + 4 * (qi >> 8);
            knn_range_split(rg[0] / tile_rows, rg[1] / tile_rows, split, lay_all ? 1 : d.n_splits, mt0, mt1);
        }
        const int total = (mt1 - mt0) * rows_per_tile;
        unsigned long long best[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j) best[j] = ~0ull;
        float thr = __builtin_inff();
        {
            const int id = idx_in[(size_t)qi * k + (k - 1)];
            if (id >= 0) thr = dist_in[(size_t)qi * k + (k - 1)];
        }
        const int steps = (total + 3) / 4;
        const int e_beg = 4 * (int)((long long)steps * part_i / P), e_end = min(total, 4 * (int)((long long)steps * (part_i + 1) / P));
        for (int e0 = e_beg; e0 < e_end; e0 += 4) {
            const int e = e0 + g;
            int r = n_words;                                  // out of range = idle group
            if (e < e_end) {
                const int tile = mt0 + e / rows_per_tile, y = e % rows_per_tile;
                const int x = lay_all ? y : ((lay16 || lay16h) ? (wr * 128 + ((y >> 2) << 4) + (fq << 2) + (y & 3)) : (l2 ? (wr * wr_rows + (((y >> 2) << 3) | (h << 2) | (y & 3))) : y));
                r = tile * tile_rows + x;
            }
            float part = 0.f;
            if (r < n_words) {
                const float* wp = words + (size_t)r * dim_pad;
                if (!l2) { for (int j = 0; j < nj; ++j) { const int i = l16 + 16 * j; const float a = i < dim ? qp[i] : 0.f, c = wp[i], sm = a + c, df = a - c; part += sm > 0.f ? df * df / sm : 0.f; } }
                else { for (int j = 0; j < nj; ++j) { const int i = l16 + 16 * j; const float df = (i < dim ? qp[i] : 0.f) - wp[i]; part += df * df; } }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            const bool hit = r < n_words && !(part > thr * 1.0001f + 1e-30f);      // NaN-safe: unordered compares count as hits
            unsigned long long hm = __ballot(hit && l16 == 0);
            while (hm) {                                                             // rare
                const int src = __ffsll((long long)hm) - 1; hm &= hm - 1;
                const int rr = __shfl(r, src, 64);
                const float d = wave_functor(metric, qp, words + (size_t)rr * dim_pad, dim, lane, s_terms[threadIdx.x >> 6]);
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
        for (int j = 0; j < KM; ++j) if (lane == j) outp[KM * (size_t)u + j] = best[j];
    }
}

// one wave per unproven query: the lanes fold the per-unit results (and the re-ranked candidates) into private sorted lists, k
// rounds of a wave-wide minimum then pick the result; a row reached through two paths is taken once
template <int KM>
__global__ __launch_bounds__(256) void k_knn_fallback_merge(int k, const uint32_t* __restrict__ flag_count, const uint32_t* __restrict__ qrec,
                                     const unsigned long long* __restrict__ item_out, size_t part_base, int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const uint32_t n_q = flag_count[KNN_CNT_QUERIES];
    const uint32_t P = knn_fb_parts(flag_count[KNN_CNT_ITEMS]);
    const unsigned long long* outp = P > 1 ? item_out + KM * part_base : item_out;
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_q; t += gridDim.x * 4) {
        const int qi = (int)qrec[3 * (size_t)t]; const uint32_t ibase = qrec[3 * (size_t)t + 1], ni = qrec[3 * (size_t)t + 2];
        unsigned long long fin[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j) fin[j] = ~0ull;
        auto ins = [&](unsigned long long key) {
#pragma unroll
            for (int j = 0; j < KM; ++j) if (fin[j] != ~0ull && (fin[j] & 0xffffffffull) == (key & 0xffffffffull)) return;   // same row twice
#pragma unroll
            for (int j = 0; j < KM; ++j) if (key < fin[j]) { const unsigned long long tmp = fin[j]; fin[j] = key; key = tmp; }
        };
        if (lane < k) {
            const int id = idx_out[(size_t)qi * k + lane];
            if (id >= 0) ins(((unsigned long long)__float_as_uint(dist_out[(size_t)qi * k + lane]) << 32) | (unsigned)id);
        }
        for (uint32_t i = lane; i < ni * P; i += 64)
            for (int j = 0; j < k; ++j) { const unsigned long long key = outp[KM * ((size_t)ibase * P + i) + j]; if (key != ~0ull) ins(key); }
        for (int j = 0; j < k; ++j) {
            const unsigned long long mn = wave_min_u64(fin[0]);
            if (lane == 0) {
                if (mn == ~0ull) { idx_out[(size_t)qi * k + j] = -1; dist_out[(size_t)qi * k + j] = __builtin_nanf(""); }
                else { idx_out[(size_t)qi * k + j] = (int)(mn & 0xffffffffull); dist_out[(size_t)qi * k + j] = __uint_as_float((unsigned)(mn >> 32)); }
            }
            if (mn == ~0ull) continue;
            // drop the chosen row from every private list (it can sit in several lanes, with the same key)
            // (a private list is sorted and holds a row at most once: shift the tail down over the hit)
            bool gone = false;
#pragma unroll
            for (int x = 0; x < KM; ++x) {
                if (!gone && fin[x] != ~0ull && (fin[x] & 0xffffffffull) == (mn & 0xffffffffull)) gone = true;
                if (gone) fin[x] = x + 1 < KM ? fin[x + 1] : ~0ull;
            }
        }
    }
}

}  // namespace

// THE layout of a queue: counters | query records [n_queries * 3] | items [q_items * 2] | item results [q_items + KNN_FB_UNITS][KM] u64
// (8-byte aligned; KM as in k_knn_fallback, whose part results lie behind the q_items whole-item results)
size_t knn_queue_bytes(size_t n_queries, size_t q_items, int k) {
    return (KNN_CNT_WORDS + 3 * n_queries + 2 * q_items) * sizeof(uint32_t) + 8 + (q_items + KNN_FB_UNITS) * (k > 4 ? KNN_MAX_K : 4) * sizeof(unsigned long long);
}
KnnQueue knn_queue_carve(void* mem, size_t n_queries, size_t q_items) {
    KnnQueue Q{};
    Q.count = (uint32_t*)mem; Q.qrec = Q.count + KNN_CNT_WORDS; Q.items = Q.qrec + 3 * n_queries; Q.q_items = q_items;
    Q.item_out = (unsigned long long*)(((uintptr_t)(Q.items + 2 * q_items) + 7) & ~(uintptr_t)7);
    return Q;
}
int knn_scan_queue(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int k, const float* q, int ldq, const KnnQueue& Q, const int* qrange, int32_t* idx_out, float* dist_out) {
    TimerScope ts(ctx, "knn_fallback");
    const auto scan = k <= 4 ? k_knn_fallback<4> : k_knn_fallback<KNN_MAX_K>;      // capacity of the per-item result lists
    const auto merge = k <= 4 ? k_knn_fallback_merge<4> : k_knn_fallback_merge<KNN_MAX_K>;
    hipLaunchKernelGGL(scan, dim3(1024), dim3(256), 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words, q, ldq, metric, k,
                       KnnFbDesc{Q.desc[0]}, KnnFbDesc{Q.desc[1]}, qrange, Q.count, Q.items, idx_out, dist_out, Q.item_out, Q.q_items);
    ISM_CHECK_LAUNCH(ctx, "k_knn_fallback");
    hipLaunchKernelGGL(merge, dim3(256), dim3(256), 0, ctx->stream, k, Q.count, Q.qrec, Q.item_out, Q.q_items, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_fallback_merge");
    return ISMHIP_OK;
}
