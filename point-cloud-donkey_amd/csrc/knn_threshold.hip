// knn_threshold.hip — ismhip_knn_threshold, the radius search (the map of the kNN units is at the top of knn.hip).
#include "knn_internal.h"

namespace {

#include "functor.h"

// ---- radius search: ActivationStrategyThreshold (activation_strategy_threshold.cpp:27-44) ----------------------------------------
// Every codeword whose functor value is STRICTLY below the threshold, in ascending row order. Large launches: the
// EMIT variant of k_knn_l2_mfma16 lists every row whose 16-bit score is <= tau_q (L2 on the f16 images of q and c, chi-square on the
// Hellinger images of sqrt q and sqrt c), k_thr_eval sorts a query's list, evaluates the functor for every listed row and keeps
// d < threshold, then count -> scan -> compact writes the CSR. A query whose list exceeds THR_EMIT_CAP is answered by the exact
// scan k_thr_exact, which is also the whole search for small or ungated launches. Proof by construction: a row that is not listed
// has functor value >= threshold (k_thr_tau).
#define THR_EMIT_CAP 512

// thr_q (large-K search, nullable): a threshold per query instead of thr
__global__ __launch_bounds__(256) void k_thr_tau(int nq, const float* __restrict__ qv, int ldq, int dim, float thr, VerifyParams vp, float* __restrict__ tau,
                                                 const float* __restrict__ thr_q = nullptr) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nq) return;
    const int lane = lane_id();
    const float qn2 = wave_norm2(qv + (size_t)i * ldq, dim, lane);
    if (lane == 0) tau[i] = thr_tau_of(thr_q ? thr_q[i] : thr, qn2, dim, vp);
}

// the FLANN functors as the reference's sequential loops (k_thr_exact: a row per thread)
__device__ __forceinline__ float flann_l2(const float* a, const float* b, int size) {
    float result = 0.f;
    int i = 0;
    for (; i + 3 < size; i += 4) {
        const float d0 = a[i] - b[i], d1 = a[i + 1] - b[i + 1], d2 = a[i + 2] - b[i + 2], d3 = a[i + 3] - b[i + 3];
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (; i < size; ++i) { const float d0 = a[i] - b[i]; result += d0 * d0; }
    return result;
}
__device__ __forceinline__ float flann_chi2(const float* a, const float* b, int size) {
    float result = 0.f;
    for (int i = 0; i < size; ++i) {
        const float sum = a[i] + b[i];
        if (sum > 0) { const float diff = a[i] - b[i]; result += diff * diff / sum; }
    }
    return result;
}

// one workgroup per query: the listed rows (codebook rows, through perm for the chi-square shadow) are sorted ascending in LDS, a wave
// per row evaluates the functor, and the rows with d < thr are compacted in row order back into the query's list (dists alongside);
// cnt_out[q] = their number. A query with more than THR_EMIT_CAP listed rows is queued in ovf[1..] (count ovf[0]) for the exact scan.
__global__ __launch_bounds__(256) void k_thr_eval(int nq, const uint32_t* __restrict__ emit_cnt, uint32_t* __restrict__ rows, float* __restrict__ dists,
                                                  const uint32_t* __restrict__ perm, const float* __restrict__ q, int dim, const float* __restrict__ words,
                                                  int dim_pad, int metric, float thr, uint32_t* __restrict__ cnt_out, uint32_t* __restrict__ ovf) {
    __shared__ uint32_t s_row[THR_EMIT_CAP];
    __shared__ float s_d[THR_EMIT_CAP];
    __shared__ __attribute__((aligned(16))) float s_q[1344];
    __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
    __shared__ BlockRank<256> s_rank;
    const int qi = blockIdx.x;
    const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    const uint32_t n = emit_cnt[qi];
    if (n > THR_EMIT_CAP) {
        if (t == 0) { cnt_out[qi] = 0u; const uint32_t s = atomicAdd(&ovf[0], 1u); ovf[1 + s] = (uint32_t)qi; }
        return;
    }
    uint32_t* lr = rows + (size_t)qi * THR_EMIT_CAP;
    for (int i = t; i < THR_EMIT_CAP; i += 256) s_row[i] = i < (int)n ? (perm ? perm[lr[i]] : lr[i]) : 0xffffffffu;
    for (int c = t; c < dim; c += 256) s_q[c] = q[(size_t)qi * dim + c];
    __syncthreads();
    for (int k = 2; k <= THR_EMIT_CAP; k <<= 1)                           // bitonic sort, ascending (empty entries sort last)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < THR_EMIT_CAP; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint32_t a = s_row[i], b = s_row[ixj];
                    if ((a > b) == ((i & k) == 0)) { s_row[i] = b; s_row[ixj] = a; }
                }
            }
            __syncthreads();
        }
    for (uint32_t s_ = wv; s_ < n; s_ += 4) {
        const float d = wave_functor(metric, s_q, words + (size_t)s_row[s_] * dim_pad, dim, lane, s_terms[wv]);
        if (lane == 0) s_d[s_] = d;
    }
    __syncthreads();
    uint32_t total = 0;
    for (int base = 0; base < THR_EMIT_CAP; base += 256) {
        const int i = base + t;
        const bool in = i < (int)n && s_d[i] < thr;
        const uint32_t o = s_rank.step(in, total);
        if (in) { lr[o] = s_row[i]; dists[(size_t)qi * THR_EMIT_CAP + o] = s_d[i]; }
    }
    if (t == 0) cnt_out[qi] = total;
}

// exact radius scan: one query per workgroup (qlist[b], or b when qlist is null) over all codebook rows, one row per thread and step,
// with the functor's own sequential summation (flann_l2 / flann_chi2, bit-identical to wave_functor). PASS 0 counts the rows with
// d < thr into cnt_out[q]; PASS 1 writes them, ascending, from off[q] on.
template <int PASS>
__global__ __launch_bounds__(256) void k_thr_exact(const uint32_t* __restrict__ qlist, const float* __restrict__ q, int dim, const float* __restrict__ words,
                                                   int dim_pad, int n_words, int metric, float thr, uint32_t* __restrict__ cnt_out,
                                                   const unsigned long long* __restrict__ off, int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    __shared__ BlockRank<256> s_rank;
    const uint32_t qi = qlist ? qlist[blockIdx.x] : blockIdx.x;
    const float* qp = q + (size_t)qi * dim;
    const int t = threadIdx.x;
    const unsigned long long pos = PASS ? off[qi] : 0ull;
    uint32_t total = 0;
    for (int base = 0; base < n_words; base += 256) {
        const int row = base + t;
        bool in = false; float d = 0.f;
        if (row < n_words) {
            d = metric == ISMHIP_METRIC_CHI2 ? flann_chi2(qp, words + (size_t)row * dim_pad, dim) : flann_l2(qp, words + (size_t)row * dim_pad, dim);
            in = d < thr;
        }
        const uint32_t r = s_rank.step(in, total);
        if (PASS && in) { idx_out[pos + r] = row; dist_out[pos + r] = d; }
    }
    if (!PASS && t == 0) cnt_out[qi] = total;
}

// exclusive scan of n counts by ONE workgroup (a contiguous chunk per thread): off[0..n] in 64 bits (a total of 2^32 or more is
// refused by the host) and the same truncated to 32 bits in off32[0..n] (the caller's CSR)
__global__ __launch_bounds__(1024) void k_thr_scan(int n, const uint32_t* __restrict__ cnt, unsigned long long* __restrict__ off, uint32_t* __restrict__ off32) {
    __shared__ unsigned long long s[1024];
    const int t = threadIdx.x;
    const int chunk = (n + 1023) / 1024;
    const int i0 = min(n, t * chunk), i1 = min(n, i0 + chunk);
    unsigned long long sum = 0ull;
    for (int i = i0; i < i1; ++i) sum += cnt[i];
    s[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                                   // Hillis-Steele inclusive scan of the chunk sums
        const unsigned long long v = t >= o ? s[t - o] : 0ull;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    unsigned long long run = s[t] - sum;
    for (int i = i0; i < i1; ++i) { off[i] = run; off32[i] = (uint32_t)run; run += cnt[i]; }
    if (t == 1023) { off[n] = s[1023]; off32[n] = (uint32_t)s[1023]; }
}

// the evaluated lists of the queries that fitted the cap -> their CSR ranges (a wave per query)
__global__ __launch_bounds__(256) void k_thr_compact(int nq, const uint32_t* __restrict__ emit_cnt, const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ rows, const float* __restrict__ dists,
                                                     const unsigned long long* __restrict__ off, int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq || emit_cnt[qi] > THR_EMIT_CAP) return;                  // overflowed queries: written by k_thr_exact<1>
    const int lane = lane_id();
    const size_t o = (size_t)off[qi];
    for (uint32_t j = lane; j < cnt[qi]; j += 64) {
        idx_out[o + j] = (int32_t)rows[(size_t)qi * THR_EMIT_CAP + j];
        dist_out[o + j] = dists[(size_t)qi * THR_EMIT_CAP + j];
    }
}

// the candidate sweep + evaluation of the large launches; on return cnt[q] holds every query's list length (the overflowed queries'
// from the exact count) and ovf[0] the number of overflowed queries, ovf[1..] their ids
int run_thr_mfma(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, float thr, const float* sq,
                 uint32_t* cnt, uint32_t* ovf, uint32_t* emit_cnt, uint32_t* rows, float* dists, uint32_t& n_ovf) {
    const bool chi = metric == ISMHIP_METRIC_CHI2;
    const ismhip_codebook* xb = chi ? cb->chi_shadow : cb;
    const int dp = cb->dim_pad, nqp = (nq + 127) / 128 * 128;
    char* buf = (char*)ism_scratch(ctx, SCR_KNN_THR2, (size_t)nqp * 4 + 64 + (size_t)nqp * cb->ld16 * 2);
    if (!buf) return ISMHIP_ERR_NOMEM;
    float* tau = (float*)buf; uint32_t* sc = (uint32_t*)(buf + (size_t)nqp * 4); u16* qimg = (u16*)(buf + (size_t)nqp * 4 + 64);
    const float* qv = chi ? sq : q;                                       // the vectors the 16-bit images are made of
    const int ldv = chi ? dp : cb->dim;
    ++ctx->knn_thr_mfma_launches;
    {
        TimerScope t1(ctx, "knn_threshold_sweep");
        ISM_HIP(ctx, hipMemsetAsync(sc, 0, 64, ctx->stream));
        ISM_HIP(ctx, hipMemsetAsync(emit_cnt, 0, (size_t)nqp * 4, ctx->stream));
        int rc = knn_f16_emit_image(ctx, cb, xb, qv, nq, ldv, nqp, sc, qimg);
        if (rc != ISMHIP_OK) return rc;
        hipLaunchKernelGGL(k_thr_tau, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, nq, qv, ldv, cb->dim, thr, knn_verify_params(xb, dp, 0, sc, true), tau);
        ISM_CHECK_LAUNCH(ctx, "k_thr_tau");
        rc = knn_mfma16_emit(ctx, cb, xb, nq, nqp, sc, qimg, tau, emit_cnt, rows, THR_EMIT_CAP);
        if (rc != ISMHIP_OK) return rc;
    }
    {
        TimerScope t2(ctx, "knn_threshold_eval");
        ISM_HIP(ctx, hipMemsetAsync(ovf, 0, 4, ctx->stream));
        hipLaunchKernelGGL(k_thr_eval, dim3(nq), dim3(256), 0, ctx->stream, nq, (const uint32_t*)emit_cnt, rows, dists,
                           chi ? (const uint32_t*)xb->shadow_perm : (const uint32_t*)nullptr, q, cb->dim, (const float*)cb->words, dp, metric, thr, cnt, ovf);
        ISM_CHECK_LAUNCH(ctx, "k_thr_eval");
        ISM_HIP(ctx, hipMemcpyAsync(&n_ovf, ovf, 4, hipMemcpyDeviceToHost, ctx->stream));
        ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n_ovf) {
        TimerScope t3(ctx, "knn_threshold_exact");
        hipLaunchKernelGGL(k_thr_exact<0>, dim3(n_ovf), dim3(256), 0, ctx->stream, (const uint32_t*)(ovf + 1), q, cb->dim, (const float*)cb->words, dp,
                           cb->n_words, metric, thr, cnt, (const unsigned long long*)nullptr, (int32_t*)nullptr, (float*)nullptr);
        ISM_CHECK_LAUNCH(ctx, "k_thr_exact<0>");
    }
    return ISMHIP_OK;
}

}  // namespace

extern "C" {

int ismhip_knn_threshold(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, float threshold, int64_t capacity,
                         uint32_t* act_offsets_out, int32_t* idx_out, float* dist_out, int64_t* n_act_h_out) {
    if (!ctx || !cb || nq < 0 || (nq > 0 && !q) || !act_offsets_out || !n_act_h_out || capacity < 0 || (capacity > 0 && (!idx_out || !dist_out)) ||
        (metric != ISMHIP_METRIC_L2SQ && metric != ISMHIP_METRIC_CHI2))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn_threshold: bad argument");
    *n_act_h_out = 0;
    if (cb->dim_pad / 16 > KNN_FB_MAXJ) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn_threshold: descriptor longer than 1344 not built");
    TimerScope ts(ctx, "knn_threshold");
    if (nq == 0 || !(threshold > 0.f)) {                                  // functor values are >= 0 (or NaN): nothing is below
        ISM_HIP(ctx, hipMemsetAsync(act_offsets_out, 0, ((size_t)nq + 1) * 4, ctx->stream));
        ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ISMHIP_OK;
    }
    const int dp = cb->dim_pad, nqp = (nq + 127) / 128 * 128;
    bool mfma = dp <= 1344 && knn_matrix_gate(ctx, cb, nq) &&
                (metric == ISMHIP_METRIC_L2SQ ? cb->words_f16 != nullptr && cb->dim > 64 : cb->chi_shadow != nullptr && ctx->knn_hellinger);
    const size_t b_base = ((size_t)nq * 4 + ((size_t)nq + 1) * 8 + ((size_t)nq + 1) * 4 + 64 + 255) / 256 * 256;
    const size_t b_mfma = mfma ? (size_t)nqp * 4 + (size_t)nq * THR_EMIT_CAP * 8 + (metric == ISMHIP_METRIC_CHI2 ? (size_t)nq * dp * 4 + 64 : 0) : 0;
    char* buf = (char*)ism_scratch(ctx, SCR_KNN_THR, b_base + b_mfma);
    if (!buf) return ISMHIP_ERR_NOMEM;
    uint32_t* cnt = (uint32_t*)buf;
    unsigned long long* off = (unsigned long long*)(buf + ((size_t)nq * 4 + 7) / 8 * 8);
    uint32_t* ovf = (uint32_t*)(off + nq + 1);                            // [0] = number of queries for the exact scan, [1..] their ids
    char* mb = buf + b_base;
    uint32_t* emit_cnt = (uint32_t*)mb; uint32_t* rows = (uint32_t*)(mb + (size_t)nqp * 4);
    float* dists = (float*)(rows + (size_t)nq * THR_EMIT_CAP); float* sq = dists + (size_t)nq * THR_EMIT_CAP;
    if (mfma && metric == ISMHIP_METRIC_CHI2) {                           // the Hellinger images need non-negative queries
        bool neg = false;
        const int rc = knn_sqrt_queries(ctx, cb, nq, q, sq, neg);
        if (rc != ISMHIP_OK) return rc;
        if (neg) mfma = false;
    }
    uint32_t n_ovf = 0;
    ctx->knn_thr_overflow = 0;
    if (mfma) {
        const int rc = run_thr_mfma(ctx, cb, metric, nq, q, threshold, sq, cnt, ovf, emit_cnt, rows, dists, n_ovf);
        if (rc != ISMHIP_OK) return rc;
        ctx->knn_thr_overflow = n_ovf;
    } else {
        TimerScope t3(ctx, "knn_threshold_exact");
        hipLaunchKernelGGL(k_thr_exact<0>, dim3(nq), dim3(256), 0, ctx->stream, (const uint32_t*)nullptr, q, cb->dim, (const float*)cb->words, dp,
                           cb->n_words, metric, threshold, cnt, (const unsigned long long*)nullptr, (int32_t*)nullptr, (float*)nullptr);
        ISM_CHECK_LAUNCH(ctx, "k_thr_exact<0>");
    }
    unsigned long long total = 0;
    {
        TimerScope t4(ctx, "knn_threshold_compact");
        hipLaunchKernelGGL(k_thr_scan, dim3(1), dim3(1024), 0, ctx->stream, nq, (const uint32_t*)cnt, off, act_offsets_out);
        ISM_CHECK_LAUNCH(ctx, "k_thr_scan");
        ISM_HIP(ctx, hipMemcpyAsync(&total, off + nq, 8, hipMemcpyDeviceToHost, ctx->stream));
        ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (total >= (1ull << 32)) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn_threshold: 2^32 or more activations not built");
        *n_act_h_out = (int64_t)total;
        if (total > 0 && (unsigned long long)capacity >= total) {         // otherwise: count only, the caller grows its buffers
            if (mfma) {
                hipLaunchKernelGGL(k_thr_compact, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, nq, (const uint32_t*)emit_cnt, (const uint32_t*)cnt,
                                   (const uint32_t*)rows, (const float*)dists, (const unsigned long long*)off, idx_out, dist_out);
                ISM_CHECK_LAUNCH(ctx, "k_thr_compact");
            }
            const int n_exact = mfma ? (int)n_ovf : nq;
            if (n_exact) {
                hipLaunchKernelGGL(k_thr_exact<1>, dim3(n_exact), dim3(256), 0, ctx->stream, mfma ? (const uint32_t*)(ovf + 1) : (const uint32_t*)nullptr, q, cb->dim,
                                   (const float*)cb->words, dp, cb->n_words, metric, threshold, cnt, (const unsigned long long*)off, idx_out, dist_out);
                ISM_CHECK_LAUNCH(ctx, "k_thr_exact<1>");
            }
            ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    return ISMHIP_OK;
}

}  // extern "C"
