// km_closest.h — the body of k_km_closest (kmeans.hip, term buffer of 1344 floats) and of k_km_closest_wide (knn_wide.hip, rows of
// up to ISMHIP_KNN_MAX_DIM floats), written once. The two kernels live in different units: a second kernel with a term buffer in
// kmeans.hip cost k_km_closest two VGPRs through the unit's LDS layout. Included inside an anonymous namespace, after functor.h.
#pragma once
#define KM_INVALID 0xffffffffu

// closest[i] = min(closest[i], d(point i, centre chosen[step - 1])): one wave per point, the functor's own summation order.
// slot[step] collects max over i of (closest bits << 32 | ~i): the farthest point, lowest index on ties (GONZALES; step 1 also
// gives dmax0 for the k-means++ integers). sT: the wave's term buffer of dim floats, s_best: four words of the workgroup.
__device__ __forceinline__ void km_closest(int n, int dim, int metric, const float* __restrict__ desc, const uint32_t* __restrict__ chosen, int step,
                                           float* __restrict__ closest, unsigned long long* __restrict__ slot, float* sT, unsigned long long* s_best) {
    const uint32_t c = chosen[step - 1];
    if (c == KM_INVALID) return;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    unsigned long long best = 0ull;
    for (int i = blockIdx.x * 4 + wv; i < n; i += gridDim.x * 4) {
        const float d = wave_functor(metric, desc + (size_t)i * dim, desc + (size_t)c * dim, dim, lane, sT);
        float cur = closest[i];
        if (d < cur) { cur = d; if (lane == 0) closest[i] = d; }
        if (cur == cur) {                                             // NaN distances never lead
            const unsigned long long key = ((unsigned long long)__float_as_uint(cur) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
            best = key > best ? key : best;
        }
    }
    best = block_max_u64(best, s_best);
    if (threadIdx.x == 0 && best) atomicMax(&slot[step], best);
}
