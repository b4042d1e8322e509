// ransac.hip — the RANSAC vote filter of Voting::findMaxima as a standalone primitive, and the vote keypoints it works on.
// Reference seams: Voting::filterVotesWithRansac (voting/voting.cpp:356-433), Voting::vote (voting.cpp:58-77: Vote::keypoint is the
// query keypoint, Vote::keypoint_training the codeword's getFeaturePosition()). The filter itself is ransac.h (one workgroup per
// cluster); the same device function runs inside the RANSAC variants of k_find_maxima / k_hough3d (maxima.hip).
#include "ransac.h"

namespace {

struct RansacFilterArgs {
    const uint32_t* off; const float* src; const float* tgt; const float* thr;
    int max_iter; unsigned long long seed; const int32_t* only_hyp;
    uint8_t* inl; int32_t* kept; int32_t* n_inl; int32_t* best_i; int32_t* iters; float* tf;
    double* d2; double* tf_d;                       // diagnostic entry only
    unsigned long long* counters;
};

__global__ __launch_bounds__(256) void k_ransac_filter(RansacFilterArgs a) {
    __shared__ RansacLds L;
    const int cl = blockIdx.x, tid = threadIdx.x;
    const uint32_t o0 = a.off[cl], o1 = a.off[cl + 1];
    const int n = (int)(o1 - o0);
    const float* S = a.src + (size_t)o0 * 3; const float* T = a.tgt + (size_t)o0 * 3;
    auto fetch = [&](int j, float* s, float* t) {
        s[0] = S[(size_t)j * 3]; s[1] = S[(size_t)j * 3 + 1]; s[2] = S[(size_t)j * 3 + 2];
        t[0] = T[(size_t)j * 3]; t[1] = T[(size_t)j * 3 + 1]; t[2] = T[(size_t)j * 3 + 2];
    };
    const int only = a.only_hyp ? a.only_hyp[cl] : -1;
    const RansacResult r = ransac_cluster(n, fetch, a.thr[cl], a.max_iter, a.seed, only, a.inl + o0, L);
    if (a.d2 && r.kept)
        for (int j = tid; j < n; j += 256) {
            float s[3], t[3];
            fetch(j, s, t);
            a.d2[o0 + j] = rs_d2(L.M, (double)s[0], (double)s[1], (double)s[2], (double)t[0], (double)t[1], (double)t[2]);
        }
    if (tid == 0) {
        a.kept[cl] = r.kept; a.n_inl[cl] = r.n_inliers;
        if (a.best_i) a.best_i[cl] = r.best_i;
        if (a.iters) a.iters[cl] = r.iterations;
        if (a.tf) {
            float* m = a.tf + (size_t)cl * 16;
            for (int rr = 0; rr < 3; ++rr) { for (int c = 0; c < 3; ++c) m[rr * 4 + c] = r.kept ? (float)L.M[rr * 3 + c] : (rr == c ? 1.f : 0.f); m[rr * 4 + 3] = r.kept ? (float)L.M[9 + rr] : 0.f; }
            m[12] = 0.f; m[13] = 0.f; m[14] = 0.f; m[15] = 1.f;
        }
        if (a.tf_d) for (int e = 0; e < 12; ++e) a.tf_d[(size_t)cl * 12 + e] = r.kept ? L.M[e] : 0.0;
        if (a.counters && only < 0) {
            atomicAdd(&a.counters[0], 1ull); atomicAdd(&a.counters[1], (unsigned long long)r.kept);
            atomicAdd(&a.counters[2], (unsigned long long)r.iterations); atomicAdd(&a.counters[3], (unsigned long long)r.evaluated);
        }
    }
}

// one thread per activation (as k_cast_votes): the keypoint pair of every vote slot; slots without a vote get zeros
template <bool CSR>
__global__ __launch_bounds__(256) void k_vote_keypoints(const uint32_t* __restrict__ vote_off, const float* __restrict__ word_kp, int n_words, int maxv,
                                                        int nq, int k, const float* __restrict__ kx, const float* __restrict__ ky, const float* __restrict__ kz,
                                                        const uint32_t* __restrict__ act_off, int64_t n_act, const int32_t* __restrict__ idx,
                                                        float* __restrict__ kp_out, float* __restrict__ kpt_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int f;
    if constexpr (CSR) {
        if (t >= n_act) return;
        int lo = 0, hi = nq;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)act_off[mid] <= t) lo = mid; else hi = mid; }
        f = lo;
    } else {
        if (t >= (int64_t)nq * k) return;
        f = (int)(t / k);
    }
    const int c = idx[t];
    const bool ok = c >= 0 && c < n_words;
    const uint32_t nv = ok ? vote_off[c + 1] - vote_off[c] : 0u;
    const size_t slot0 = (size_t)t * maxv;
    for (int v = 0; v < maxv; ++v) {
        const size_t s = (slot0 + v) * 3;
        const bool has = (uint32_t)v < nv;
        kp_out[s] = has ? kx[f] : 0.f; kp_out[s + 1] = has ? ky[f] : 0.f; kp_out[s + 2] = has ? kz[f] : 0.f;
        kpt_out[s] = has ? word_kp[(size_t)c * 3] : 0.f; kpt_out[s + 1] = has ? word_kp[(size_t)c * 3 + 1] : 0.f; kpt_out[s + 2] = has ? word_kp[(size_t)c * 3 + 2] : 0.f;
    }
}

}  // namespace

unsigned long long* ism_ransac_counters(ismhip_ctx* ctx) {
    if (!ctx->ransac_counters_d) {
        if (hipMalloc((void**)&ctx->ransac_counters_d, 4 * sizeof(unsigned long long)) != hipSuccess) { ism_set_err(ctx, ISMHIP_ERR_NOMEM, "ransac counters"); return nullptr; }
        if (hipMemsetAsync(ctx->ransac_counters_d, 0, 4 * sizeof(unsigned long long), ctx->stream) != hipSuccess) { ism_set_err(ctx, ISMHIP_ERR_HIP, "ransac counters"); return nullptr; }
    }
    return ctx->ransac_counters_d;
}

static int ransac_launch(ismhip_ctx* ctx, const char* what, int n_clusters, const uint32_t* cluster_offsets_h, const float* src_xyz, const float* tgt_xyz,
                         const float* threshold_h, int max_iterations, unsigned long long seed, const int32_t* hypothesis_h,
                         uint8_t* inlier_out, int32_t* kept_out, int32_t* n_inliers_out, int32_t* best_hypothesis_out, int32_t* iterations_out,
                         float* transform_out, double* d2_out, double* transform_d_out) {
    if (!ctx || n_clusters < 0 || !cluster_offsets_h || !threshold_h || !inlier_out || !kept_out || !n_inliers_out || max_iterations < 0)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, std::string(what) + ": bad argument");
    if (n_clusters == 0) return ISMHIP_OK;
    RaggedOffsets clusters;
    int rc = ism_ragged_offsets(ctx, what, cluster_offsets_h, n_clusters, SCR_SLOT_OFF, RAGGED_EMPTY, &clusters);
    if (rc != ISMHIP_OK) return rc;
    if (clusters.max_run > 0x7fffffffu) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, std::string(what) + ": a cluster of 2^31 votes or more is not built");
    if (clusters.total > 0 && (!src_xyz || !tgt_xyz)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, std::string(what) + ": bad argument");
    const size_t per = hypothesis_h ? 8 : 4;
    unsigned char* scr = (unsigned char*)ism_scratch(ctx, SCR_CLASS_BW, (size_t)n_clusters * per);
    if (!scr) return ISMHIP_ERR_NOMEM;
    ISM_HIP(ctx, hipMemcpyAsync(scr, threshold_h, (size_t)n_clusters * 4, hipMemcpyHostToDevice, ctx->stream));
    if (hypothesis_h) ISM_HIP(ctx, hipMemcpyAsync(scr + (size_t)n_clusters * 4, hypothesis_h, (size_t)n_clusters * 4, hipMemcpyHostToDevice, ctx->stream));
    RansacFilterArgs a;
    a.off = clusters.dev; a.src = src_xyz; a.tgt = tgt_xyz; a.thr = (const float*)scr; a.max_iter = std::min(max_iterations, 1 << 30); a.seed = seed;
    a.only_hyp = hypothesis_h ? (const int32_t*)(scr + (size_t)n_clusters * 4) : nullptr;
    a.inl = inlier_out; a.kept = kept_out; a.n_inl = n_inliers_out; a.best_i = best_hypothesis_out; a.iters = iterations_out; a.tf = transform_out;
    a.d2 = d2_out; a.tf_d = transform_d_out;
    a.counters = ism_ransac_counters(ctx);
    if (!a.counters) return ISMHIP_ERR_NOMEM;
    TimerScope ts(ctx, "ransac_filter");
    hipLaunchKernelGGL(k_ransac_filter, dim3(n_clusters), dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_ransac_filter");
    // the host arrays (offsets, thresholds) were handed to asynchronous copies: they must have been read before the caller reuses them
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ISMHIP_OK;
}

extern "C" {

int ismhip_ransac_filter(ismhip_ctx* ctx, int n_clusters, const uint32_t* cluster_offsets_h, const float* src_xyz, const float* tgt_xyz,
                         const float* threshold_h, int max_iterations, unsigned long long seed,
                         uint8_t* inlier_out, int32_t* kept_out, int32_t* n_inliers_out, int32_t* best_hypothesis_out, int32_t* iterations_out,
                         float* transform_out) {
    return ransac_launch(ctx, "ransac_filter", n_clusters, cluster_offsets_h, src_xyz, tgt_xyz, threshold_h, max_iterations, seed, nullptr,
                         inlier_out, kept_out, n_inliers_out, best_hypothesis_out, iterations_out, transform_out, nullptr, nullptr);
}

int ismhip_ransac_hypothesis(ismhip_ctx* ctx, int n_clusters, const uint32_t* cluster_offsets_h, const float* src_xyz, const float* tgt_xyz,
                             const float* threshold_h, unsigned long long seed, const int32_t* hypothesis_h,
                             uint8_t* inlier_out, int32_t* valid_out, int32_t* n_inliers_out, double* d2_out, double* transform_out) {
    if (!hypothesis_h || !d2_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "ransac_hypothesis: bad argument");
    for (int c = 0; c < n_clusters; ++c) if (hypothesis_h[c] < 0 || hypothesis_h[c] > (1 << 20)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "ransac_hypothesis: hypothesis index");
    return ransac_launch(ctx, "ransac_hypothesis", n_clusters, cluster_offsets_h, src_xyz, tgt_xyz, threshold_h, 1 << 30, seed, hypothesis_h,
                         inlier_out, valid_out, n_inliers_out, nullptr, nullptr, nullptr, d2_out, transform_out);
}

int ismhip_codebook_set_word_keypoint(ismhip_ctx* ctx, ismhip_codebook* cb, const float* word_keypoint_h) {
    if (!ctx || !cb || !word_keypoint_h) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "codebook_set_word_keypoint: bad argument");
    ISM_HIP(ctx, hipSetDevice(ctx->device));
    if (!cb->word_keypoint && hipMalloc((void**)&cb->word_keypoint, (size_t)std::max(cb->n_words, 1) * 12) != hipSuccess)
        return ism_set_err(ctx, ISMHIP_ERR_NOMEM, "codebook_set_word_keypoint: allocation");
    ISM_HIP(ctx, hipMemcpy(cb->word_keypoint, word_keypoint_h, (size_t)cb->n_words * 12, hipMemcpyHostToDevice));
    return ISMHIP_OK;
}

int ismhip_vote_keypoints(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* kpx, const float* kpy, const float* kpz,
                          int k, const int32_t* idx, float* vote_kp_out, float* vote_kp_train_out) {
    if (!ctx || !cb || nq < 0 || k <= 0 || !kpx || !kpy || !kpz || !idx || !vote_kp_out || !vote_kp_train_out)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "vote_keypoints: bad argument");
    if (!cb->word_keypoint) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "vote_keypoints: the codebook has no training keypoints (ismhip_codebook_set_word_keypoint)");
    if (nq == 0 || cb->max_votes == 0) return ISMHIP_OK;
    TimerScope ts(ctx, "vote_keypoints");
    const int64_t n = (int64_t)nq * k;
    hipLaunchKernelGGL(k_vote_keypoints<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, cb->vote_off, cb->word_keypoint, cb->n_words, cb->max_votes,
                       nq, k, kpx, kpy, kpz, (const uint32_t*)nullptr, (int64_t)0, idx, vote_kp_out, vote_kp_train_out);
    ISM_CHECK_LAUNCH(ctx, "k_vote_keypoints");
    return ISMHIP_OK;
}

int ismhip_vote_keypoints_csr(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* kpx, const float* kpy, const float* kpz,
                              const uint32_t* act_offsets, int64_t n_act, const int32_t* idx, float* vote_kp_out, float* vote_kp_train_out) {
    if (!ctx || !cb || nq < 0 || n_act < 0 || !act_offsets || (n_act > 0 && (!kpx || !kpy || !kpz || !idx || !vote_kp_out || !vote_kp_train_out)))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "vote_keypoints_csr: bad argument");
    if (!cb->word_keypoint) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "vote_keypoints_csr: the codebook has no training keypoints (ismhip_codebook_set_word_keypoint)");
    if (nq == 0 || n_act == 0 || cb->max_votes == 0) return ISMHIP_OK;
    TimerScope ts(ctx, "vote_keypoints");
    hipLaunchKernelGGL(k_vote_keypoints<true>, dim3((unsigned)((n_act + 255) / 256)), dim3(256), 0, ctx->stream, cb->vote_off, cb->word_keypoint, cb->n_words, cb->max_votes,
                       nq, 0, kpx, kpy, kpz, act_offsets, n_act, idx, vote_kp_out, vote_kp_train_out);
    ISM_CHECK_LAUNCH(ctx, "k_vote_keypoints<csr>");
    return ISMHIP_OK;
}

}  // extern "C"
