// rank.hip — training-side feature ranking ("codebook cleaning") on the device.
// Reference: FeatureRanking::operator() (feature_ranking/feature_ranking.cpp:37-118) between feature extraction and clustering in
// ImplicitShapeModel::train() (implicit_shape_model.cpp:437-443): iComputeScores of the subclass, then rankFeaturesWithScores +
// extractSubsetFromRankedList (:121-203). Every subclass is an exact chi-square kNN (flann::ChiSquareDistance is hard-coded, :35)
// followed by float arithmetic that the reference writes out; the searches are ismhip_knn / ismhip_knn_large_k on search-only
// codebooks (train.hip: ism_knn_only_codebook), everything after them is built here from the device-resident neighbour lists:
//   KNNActivation / Incremental (ranking_knn_activation.cpp:53-110, ranking_incremental.cpp:51-84): every query adds a term to the
//       score of each of its neighbours. The reference adds them one query after the other in float, so the sum of a target is
//       taken in that order: k_rank_count / k_rank_scan / k_rank_fill build the reverse lists (target -> (query, term)); a query names
//       a target at most once, so sorting a list by query IS the reference's order, whatever order the fill's integer atomics ran in.
//       k_rank_sum orders a list of up to RANK_LIST_LDS entries in LDS and adds it sequentially; k_rank_sum_big serves longer lists
//       (hub rows, many duplicates) by sweeping the queries in order. No float atomics anywhere: two runs give the same bits.
//   Strangeness / NaiveBayes (ranking_strangeness.cpp:58-93, ranking_naive_bayes.cpp:52-79): one search per class into a table of the
//       k nearest rows of every class for a chunk of queries, then one thread per query.
//   ismhip_rank_select: two order statistics per class by a radix select on the 64-bit key (ordered score bits, index in the class).
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstring>

int ism_knn_only_codebook(ismhip_ctx* ctx, int n_words, int dim, const float* words_d, ismhip_codebook** out, bool light);   // train.hip

namespace {

// The per-class table of a query chunk (idx + dist of n_classes lists of K entries per query) stays below this many bytes, unless
// fewer than RANK_MIN_CHUNK queries would fit: then the chunk is RANK_MIN_CHUNK queries and the table n_classes * K * 8 * RANK_MIN_CHUNK bytes.
#define RANK_TABLE_BYTES ((size_t)256 << 20)
#define RANK_MIN_CHUNK 256
#define RANK_LIST_LDS 1024                 // reverse-list entries k_rank_sum orders in LDS (per wave); longer lists: k_rank_sum_big

// the term query q adds to its j-th neighbour (distance d, next distance dn)
__device__ __forceinline__ float rank_term(int type, int inc, float d, float dn) {
    if (type == ISMHIP_RANK_INCREMENTAL) return d - dn;                          // ranking_incremental.cpp:77-78
    // ranking_knn_activation.cpp:99-104 with score_dist_rate = 1 (UseFeaturePosition false)
    if (inc == 2) return 1.0f / (d + 1.0f);
    if (inc == 3) return expf(d);
    return 1.0f;
}

// activation a = (query a / m1, neighbour a % m1): the first m1 = m - 1 neighbours of every query
__global__ void k_rank_count(uint32_t na, int m1, int K, uint32_t n, const int32_t* __restrict__ idx, uint32_t* __restrict__ cnt) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    const uint32_t t = (uint32_t)idx[(size_t)(a / m1) * K + a % m1];
    if (t < n) atomicAdd(&cnt[t], 1u);
}
// exclusive scan by ONE workgroup; off[n] = total
__global__ __launch_bounds__(1024) void k_rank_scan(uint32_t n, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off) {
    __shared__ BlockScan<1024> scan;
    scan.init();
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t start = scan.step(i < n ? cnt[i] : 0u);
        if (i < n) off[i] = start;
    }
    if (threadIdx.x == 0) off[n] = scan.total();
}
__global__ void k_rank_fill(uint32_t na, int m1, int K, uint32_t n, int type, int inc, const int32_t* __restrict__ idx, const float* __restrict__ dist,
                            const uint32_t* __restrict__ off, uint32_t* __restrict__ cur, uint32_t* __restrict__ list_q, float* __restrict__ list_term) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    const uint32_t q = a / m1, j = a % m1;
    const size_t e = (size_t)q * K + j;
    const uint32_t t = (uint32_t)idx[e];
    if (t >= n) return;
    const uint32_t pos = off[t] + atomicAdd(&cur[t], 1u);
    list_q[pos] = q;
    list_term[pos] = rank_term(type, inc, dist[e], dist[e + 1]);                 // j + 1 <= m - 1 < K: inside the row
}
// one wave per target: its list ordered by query (rank by counting: the queries of a list are distinct), then the float sum in that order
__global__ __launch_bounds__(256) void k_rank_sum(uint32_t n, const uint32_t* __restrict__ off, const uint32_t* __restrict__ list_q,
                                                  const float* __restrict__ list_term, float* __restrict__ score) {
    __shared__ uint32_t s_q[4][RANK_LIST_LDS];
    __shared__ float s_t[4][RANK_LIST_LDS];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x * 4 + wv; t < n; t += gridDim.x * 4) {
        const uint32_t b = off[t], m = off[t + 1] - b;
        if (m > RANK_LIST_LDS) continue;                                         // k_rank_sum_big
        for (uint32_t i = lane; i < m; i += 64) s_q[wv][i] = list_q[b + i];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (uint32_t i = lane; i < m; i += 64) {
            const uint32_t q = s_q[wv][i];
            uint32_t r = 0;
            for (uint32_t x = 0; x < m; ++x) r += s_q[wv][x] < q;
            s_t[wv][r] = list_term[b + i];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        float sum = 0.f;
        for (uint32_t i = 0; i < m; ++i) sum += s_t[wv][i];
        if (lane == 0) score[t] = sum;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}
// lists longer than RANK_LIST_LDS: one workgroup per target sweeps the queries in ascending order, 256 at a time; the hits of a sweep
// are laid out in query order by the block scan and thread 0 adds them
__global__ __launch_bounds__(256) void k_rank_sum_big(uint32_t n, int m1, int K, int type, int inc, const uint32_t* __restrict__ off,
                                                      const int32_t* __restrict__ idx, const float* __restrict__ dist, float* __restrict__ score) {
    __shared__ BlockScan<256> scan;
    __shared__ float s_term[256];
    for (uint32_t t = blockIdx.x; t < n; t += gridDim.x) {
        if (off[t + 1] - off[t] <= RANK_LIST_LDS) continue;                      // uniform across the workgroup
        float sum = 0.f;                                                         // thread 0's
        for (uint32_t base = 0; base < n; base += 256) {
            const uint32_t q = base + threadIdx.x;
            uint32_t hit = 0; float term = 0.f;
            if (q < n)
                for (int j = 0; j < m1; ++j)
                    if ((uint32_t)idx[(size_t)q * K + j] == t) { hit = 1; term = rank_term(type, inc, dist[(size_t)q * K + j], dist[(size_t)q * K + j + 1]); break; }
            scan.init();
            const uint32_t p = scan.step(hit);
            if (hit) s_term[p] = term;
            __syncthreads();
            if (threadIdx.x == 0) { const uint32_t c = scan.total(); for (uint32_t i = 0; i < c; ++i) sum += s_term[i]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) score[t] = sum;
    }
}

// ---- per-class types: tab_idx / tab_dist [n_classes][nqc][K] of the chunk's queries q0 .. q0 + nqc (rows local to the class, -1 = none)
__device__ __forceinline__ int class_of(const uint32_t* __restrict__ coff, int n_classes, uint32_t i) {
    int c = 0;
    while (c + 1 < n_classes && coff[c + 1] <= i) ++c;                            // the last class with coff[c] <= i: skips empty classes
    return c;
}
__global__ void k_rank_strangeness(uint32_t q0, uint32_t nqc, int K, int n_classes, const uint32_t* __restrict__ coff,
                                   const int32_t* __restrict__ tab_idx, const float* __restrict__ tab_dist, float* __restrict__ score) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nqc) return;
    const int own = class_of(coff, n_classes, q0 + qi);
    float own_sum = 0.f, other = 0.f; bool first = true;
    for (int c = 0; c < n_classes; ++c) {
        float sum = 0.f;                                                         // :76-80; an empty class: the empty list's 0
        if (coff[c + 1] > coff[c]) {
            const size_t e = ((size_t)c * nqc + qi) * K;
            for (int j = 0; j < K; ++j) if (tab_idx[e + j] >= 0) sum += tab_dist[e + j];
        }
        if (c == own) own_sum = sum;
        else if (first || sum < other) { other = sum; first = false; }           // :85-87: the smallest of the others
    }
    score[q0 + qi] = own_sum / other;
}
// num_neg: the rows below the threshold among the K nearest of the complement. Those K are the K smallest, in (distance, global row)
// order, of the other classes' lists; the ones below the threshold are a prefix of them, so their number is the number of entries
// below the threshold in all those lists together, capped at K -- whichever way the ties at the K-th place fall.
__global__ void k_rank_bayes(uint32_t q0, uint32_t nqc, int K, int n_classes, uint32_t n, float thr, const uint32_t* __restrict__ coff,
                             const int32_t* __restrict__ tab_idx, const float* __restrict__ tab_dist, float* __restrict__ score) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nqc) return;
    const int own = class_of(coff, n_classes, q0 + qi);
    int pos = 0, neg = 0;
    for (int c = 0; c < n_classes; ++c) {
        if (coff[c + 1] == coff[c]) continue;
        const size_t e = ((size_t)c * nqc + qi) * K;
        int below = 0;
        for (int j = 0; j < K; ++j) below += tab_idx[e + j] >= 0 && tab_dist[e + j] < thr;
        if (c == own) pos = below; else neg += below;
    }
    if (neg > K) neg = K;
    const uint32_t s = coff[own + 1] - coff[own];
    const float num_pos = (float)pos, num_neg = (float)neg, num_current = (float)s, num_other = (float)(n - s);
    const float pos_prob = num_pos / num_current;                                // ranking_naive_bayes.cpp:71-74
    score[q0 + qi] = pos_prob / ((num_pos + num_neg) / (num_current + num_other));
}

// ---- selection ----------------------------------------------------------------------------------------------------------------
// ascending by (score, index in the class), -0 == +0, NaN after +inf
__device__ __forceinline__ unsigned long long rank_key(float s, uint32_t local) {
    uint32_t u;
    if (s != s) u = 0xffffffffu;
    else {
        u = __float_as_uint(s == 0.f ? 0.f : s);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)u << 32) | local;
}
struct RankClass { uint32_t off, size, lo, hi; };       // the kept ranks of the class are [lo, hi)
// blockIdx.y = 0: the key of rank lo, 1: of rank hi (skipped when the rank is outside the class: no bound on that side). MSB-first
// radix select, 8 bits a pass: histogram of the next digit over the keys that share the prefix found so far.
__global__ __launch_bounds__(1024) void k_rank_select_stat(const RankClass* __restrict__ rc, const float* __restrict__ score, unsigned long long* __restrict__ stat) {
    __shared__ uint32_t s_hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ uint32_t s_rank;
    const RankClass c = rc[blockIdx.x];
    const uint32_t want = blockIdx.y == 0 ? c.lo : c.hi;
    if (want >= c.size) return;                                                  // uniform across the workgroup
    if (threadIdx.x == 0) { s_prefix = 0ull; s_rank = want; }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (threadIdx.x < 256) s_hist[threadIdx.x] = 0u;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        for (uint32_t i = threadIdx.x; i < c.size; i += 1024) {
            const unsigned long long k = rank_key(score[c.off + i], i);
            if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&s_hist[(uint32_t)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t r = s_rank; int d = 0;
            while (d < 255 && r >= s_hist[d]) { r -= s_hist[d]; ++d; }
            s_rank = r; s_prefix = (prefix << 8) | (unsigned long long)d;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) stat[blockIdx.x * 2 + blockIdx.y] = s_prefix;
}
__global__ void k_rank_keep(uint32_t n, int n_classes, const uint32_t* __restrict__ coff, const RankClass* __restrict__ rc, const float* __restrict__ score,
                            const unsigned long long* __restrict__ stat, uint8_t* __restrict__ keep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ci = class_of(coff, n_classes, i);
    const RankClass c = rc[ci];
    bool k = c.lo < c.hi;
    if (k) {
        const unsigned long long key = rank_key(score[i], i - c.off);
        if (c.lo > 0) k = key >= stat[ci * 2];                                   // lo < hi <= size: the statistic was computed
        if (k && c.hi < c.size) k = key < stat[ci * 2 + 1];
    }
    keep[i] = k ? 1 : 0;
}

bool offsets_ok(const uint32_t* off, int n_classes, int n) {
    if (off[0] != 0 || off[n_classes] != (uint32_t)n) return false;
    for (int c = 0; c < n_classes; ++c) if (off[c + 1] < off[c]) return false;
    return true;
}

}  // namespace

// chi-square never searches the rotated squared-L2 image: the codebook is built without it (no host eigen-solve), with the chi-square
// shadow ismhip_knn takes its matrix-core candidates from
static int rank_codebook(ismhip_ctx* ctx, int n_words, int dim, const float* words_d, ismhip_codebook** out) {
    const int was = ctx->knn_pca_m;
    ctx->knn_pca_m = 0;
    const int rc = ism_knn_only_codebook(ctx, n_words, dim, words_d, out, false);
    ctx->knn_pca_m = was;
    return rc;
}

extern "C" int ismhip_rank_scores(ismhip_ctx* ctx, int type, int n, int dim, const float* desc, int n_classes, const uint32_t* class_offsets_h,
                                  int k_search, float dist_threshold, int increment_type, float* score_out) {
    if (!ctx || n <= 0 || dim <= 0 || !desc || n_classes <= 0 || !class_offsets_h || !score_out || k_search < 1)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rank_scores: bad argument");
    if (type < ISMHIP_RANK_KNN_ACTIVATION || type > ISMHIP_RANK_NAIVE_BAYES) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rank_scores: unknown ranking type");
    if (type == ISMHIP_RANK_KNN_ACTIVATION && (increment_type < 0 || increment_type > 3))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rank_scores: score increment type outside 0 .. 3");
    if (!offsets_ok(class_offsets_h, n_classes, n)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rank_scores: class offsets must ascend from 0 to n");
    const bool scatter = type == ISMHIP_RANK_KNN_ACTIVATION || type == ISMHIP_RANK_INCREMENTAL;
    const int K = scatter ? k_search + 1 : k_search;
    if (k_search >= ISMHIP_KNN_LARGE_K_MAX) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "rank_scores: KSearch of 1024 or more not built");
    if (dim > ISMHIP_SHORT_CSHOT_MAX_DIM) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "rank_scores: descriptor longer than 1344 not built");
    if (type == ISMHIP_RANK_STRANGENESS) {
        int nonempty = 0;
        for (int c = 0; c < n_classes; ++c) nonempty += class_offsets_h[c + 1] > class_offsets_h[c];
        if (nonempty < 2) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rank_scores: Strangeness needs two non-empty classes");
    }
    if ((size_t)n * K > 0x7fffffff) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "rank_scores: 2^31 or more neighbours not built");
    TimerScope ts(ctx, "rank_scores");
    ++ctx->rank_launches;
    hipStream_t st = ctx->stream;
    const int metric = ISMHIP_METRIC_CHI2;

    if (scatter) {
        const int m = std::min(K, n), m1 = m - 1;                                // valid neighbours per query; the last one is dropped
        const size_t nk = (size_t)n * K, na = (size_t)n * m1;
        char* kb = (char*)ism_scratch(ctx, SCR_RANK_KNN, nk * 8 + 16);
        char* sb = (char*)ism_scratch(ctx, SCR_RANK, ((size_t)n + 1) * 12 + na * 8 + 64);
        if (!kb || !sb) return ISMHIP_ERR_NOMEM;
        int32_t* idx = (int32_t*)kb; float* dist = (float*)(kb + nk * 4);
        uint32_t* cnt = (uint32_t*)sb; uint32_t* cur = cnt + (n + 1); uint32_t* off = cur + (n + 1);
        uint32_t* list_q = off + (n + 1); float* list_term = (float*)(list_q + na);
        ismhip_codebook* cb = nullptr;
        int rc = rank_codebook(ctx, n, dim, desc, &cb);
        if (rc != ISMHIP_OK) return rc;
        rc = ismhip_knn_large_k(ctx, cb, metric, n, desc, K, idx, dist);        // K <= 16: ismhip_knn
        ismhip_codebook_destroy(ctx, cb);
        if (rc != ISMHIP_OK) return rc;
        TimerScope tk(ctx, "rank_score_kernels");                                // everything but the codebook and the search
        ISM_HIP(ctx, hipMemsetAsync(cnt, 0, ((size_t)n + 1) * 8, st));           // cnt and cur
        if (na) {
            const unsigned ga = (unsigned)((na + 255) / 256);
            hipLaunchKernelGGL(k_rank_count, dim3(ga), dim3(256), 0, st, (uint32_t)na, m1, K, (uint32_t)n, idx, cnt);
            hipLaunchKernelGGL(k_rank_scan, dim3(1), dim3(1024), 0, st, (uint32_t)n, cnt, off);
            hipLaunchKernelGGL(k_rank_fill, dim3(ga), dim3(256), 0, st, (uint32_t)na, m1, K, (uint32_t)n, type, increment_type, idx, dist, off, cur, list_q, list_term);
            hipLaunchKernelGGL(k_rank_sum, dim3((unsigned)std::min<size_t>(((size_t)n + 3) / 4, 16384)), dim3(256), 0, st, (uint32_t)n, off, list_q, list_term, score_out);
            hipLaunchKernelGGL(k_rank_sum_big, dim3((unsigned)std::min(n, 1024)), dim3(256), 0, st, (uint32_t)n, m1, K, type, increment_type, off, idx, dist, score_out);
            ISM_CHECK_LAUNCH(ctx, "k_rank_sum");
        } else {
            ISM_HIP(ctx, hipMemsetAsync(score_out, 0, (size_t)n * 4, st));       // a single feature: no neighbour but the dropped one
        }
        ISM_HIP(ctx, hipStreamSynchronize(st));
        return ISMHIP_OK;
    }

    // ---- Strangeness / NaiveBayes: a search-only codebook per non-empty class, the queries in chunks
    std::vector<ismhip_codebook*> cbs((size_t)n_classes, nullptr);
    auto release = [&](int code) { for (ismhip_codebook* cb : cbs) if (cb) ismhip_codebook_destroy(ctx, cb); return code; };
    for (int c = 0; c < n_classes; ++c) {
        const uint32_t b = class_offsets_h[c], s = class_offsets_h[c + 1] - b;
        if (s == 0) continue;
        const int rc = rank_codebook(ctx, (int)s, dim, desc + (size_t)b * dim, &cbs[c]);
        if (rc != ISMHIP_OK) return release(rc);
    }
    const size_t per_query = (size_t)n_classes * K * 8;
    const uint32_t chunk = (uint32_t)std::min<size_t>((size_t)n, std::max<size_t>(RANK_MIN_CHUNK, RANK_TABLE_BYTES / per_query));
    char* tb = (char*)ism_scratch(ctx, SCR_RANK_KNN, per_query * chunk + 16);
    uint32_t* coff = (uint32_t*)ism_scratch(ctx, SCR_RANK, ((size_t)n_classes + 1) * 4);
    if (!tb || !coff) return release(ISMHIP_ERR_NOMEM);
    if (hipMemcpyAsync(coff, class_offsets_h, ((size_t)n_classes + 1) * 4, hipMemcpyHostToDevice, st) != hipSuccess)
        return release(ism_set_err(ctx, ISMHIP_ERR_HIP, "rank_scores: class offsets copy"));
    for (uint32_t q0 = 0; q0 < (uint32_t)n; q0 += chunk) {
        const uint32_t nqc = std::min(chunk, (uint32_t)n - q0);
        int32_t* tab_idx = (int32_t*)tb; float* tab_dist = (float*)(tb + (size_t)n_classes * nqc * K * 4);
        for (int c = 0; c < n_classes; ++c) {
            if (!cbs[c]) continue;
            const int rc = ismhip_knn_large_k(ctx, cbs[c], metric, (int)nqc, desc + (size_t)q0 * dim, K, tab_idx + (size_t)c * nqc * K, tab_dist + (size_t)c * nqc * K);
            if (rc != ISMHIP_OK) return release(rc);
        }
        const unsigned g = (nqc + 255) / 256;
        TimerScope tk(ctx, "rank_score_kernels");
        if (type == ISMHIP_RANK_STRANGENESS)
            hipLaunchKernelGGL(k_rank_strangeness, dim3(g), dim3(256), 0, st, q0, nqc, K, n_classes, coff, tab_idx, tab_dist, score_out);
        else
            hipLaunchKernelGGL(k_rank_bayes, dim3(g), dim3(256), 0, st, q0, nqc, K, n_classes, (uint32_t)n, dist_threshold, coff, tab_idx, tab_dist, score_out);
        if (hipGetLastError() != hipSuccess) return release(ism_set_err(ctx, ISMHIP_ERR_HIP, "launch k_rank_strangeness / k_rank_bayes"));
    }
    if (hipStreamSynchronize(st) != hipSuccess) return release(ism_set_err(ctx, ISMHIP_ERR_HIP, "rank_scores: synchronize"));
    return release(ISMHIP_OK);
}

extern "C" int ismhip_rank_select(ismhip_ctx* ctx, int n, int n_classes, const uint32_t* class_offsets_h, const float* score,
                                  float factor, float extract_offset, uint8_t* keep_out, uint32_t* n_keep_h_out) {
    if (!ctx || n <= 0 || n_classes <= 0 || !class_offsets_h || !score || !keep_out || !n_keep_h_out)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rank_select: bad argument");
    if (!offsets_ok(class_offsets_h, n_classes, n)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rank_select: class offsets must ascend from 0 to n");
    TimerScope ts(ctx, "rank_select");
    ++ctx->rank_launches;
    // the window of every class (feature_ranking.cpp:177-191). (float)j is monotone in j, so the kept ranks are one range [lo, hi):
    // lo = the first rank with (float)j >= min_index, hi = the first with !((float)j < max_index), found by bisection on the
    // reference's own float comparisons
    std::vector<RankClass> rc((size_t)n_classes);
    for (int c = 0; c < n_classes; ++c) {
        const uint32_t s = class_offsets_h[c + 1] - class_offsets_h[c];
        float min_index = (float)s * extract_offset;
        float max_index = (float)s * (factor + extract_offset);
        if (min_index < 0) min_index = 0;
        if (max_index > (float)s) max_index = (float)s;
        auto first_rank = [&](auto&& pred) { uint32_t a = 0, b = s; while (a < b) { const uint32_t mid = a + (b - a) / 2; if (pred((float)mid)) b = mid; else a = mid + 1; } return a; };
        const uint32_t lo = first_rank([&](float j) { return j >= min_index; });
        const uint32_t hi = first_rank([&](float j) { return !(j < max_index); });
        rc[c] = RankClass{class_offsets_h[c], s, lo, hi};
    }
    const size_t rc_bytes = (rc.size() * sizeof(RankClass) + 15) / 16 * 16, st_bytes = (size_t)n_classes * 16;
    char* sb = (char*)ism_scratch(ctx, SCR_RANK, rc_bytes + st_bytes + ((size_t)n_classes + 1) * 4);
    if (!sb) return ISMHIP_ERR_NOMEM;
    RankClass* d_rc = (RankClass*)sb; unsigned long long* d_stat = (unsigned long long*)(sb + rc_bytes); uint32_t* coff = (uint32_t*)(sb + rc_bytes + st_bytes);
    hipStream_t st = ctx->stream;
    ISM_HIP(ctx, hipMemcpyAsync(d_rc, rc.data(), rc.size() * sizeof(RankClass), hipMemcpyHostToDevice, st));
    ISM_HIP(ctx, hipMemcpyAsync(coff, class_offsets_h, ((size_t)n_classes + 1) * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rank_select_stat, dim3(n_classes, 2), dim3(1024), 0, st, d_rc, score, d_stat);
    hipLaunchKernelGGL(k_rank_keep, dim3((n + 255) / 256), dim3(256), 0, st, (uint32_t)n, n_classes, coff, d_rc, score, d_stat, keep_out);
    ISM_CHECK_LAUNCH(ctx, "k_rank_keep");
    ISM_HIP(ctx, hipStreamSynchronize(st));
    for (int c = 0; c < n_classes; ++c) n_keep_h_out[c] = rc[c].hi > rc[c].lo ? rc[c].hi - rc[c].lo : 0u;
    return ISMHIP_OK;
}
