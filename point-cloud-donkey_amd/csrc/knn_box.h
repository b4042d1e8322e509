// knn_box.h — the exact k-nearest search of ONE THREAD per query over a cloud's cell grid, by a growing box of cells around the query
// (k_sor_meandist of prefilter.hip, k_sift_extrema of sift3d.hip). The caller owns the candidate list: `span(b, e)` considers the
// cell-sorted records [b, e) of the object, and `kth_d2` is the caller's current k-th squared distance (+inf while the list is being
// filled), read again after every span.
//
// Invariant after step s: every point of the box [lo, hi] has been read OR lies at a squared distance >= the current k-th one (inside
// the box, cells that cannot hold a closer point are clipped away: cell_coord is monotone and is the very function that binned the
// points, so a point with |p_a - q_a| <= rk lies in a cell of [cell_coord(q_a - rk), cell_coord(q_a + rk)]). A point outside the box is
// at least as far as the nearest box face that still has cells behind it. The search is complete when the k-th squared distance is <=
// the square of that face distance (taken conservatively: the padding absorbs the rounding of the cell bounds, and the factor below
// one keeps a point at exactly the k-th distance from waiting outside), or when the box holds the whole grid. Which cells were read
// therefore never shows in the result. The box radius is 0, half the smallest cell edge, then the largest cell edge doubled per step;
// a grid has at most ISM_GRID_MAXDIM cells per axis, so eight steps reach every cell.
// Returns false when `max_steps` steps did not complete the search (the caller's bounded path takes over).
#pragma once
#include "common.h"

template <class Span>
__device__ __forceinline__ bool knn_box_search(const GridMeta& m, const uint32_t* __restrict__ cs, const float (&q)[3], int max_steps,
                                               const float& kth_d2, Span&& span) {
    const float cmax = fmaxf(m.cell[0], fmaxf(m.cell[1], m.cell[2])), cmin = fminf(m.cell[0], fminf(m.cell[1], m.cell[2]));
    int plo[3] = {0, 0, 0}, phi[3] = {-1, -1, -1};          // previous box (empty)
    bool done = false;
    for (int s = 0; s < max_steps && !done; ++s) {
        const float R = s == 0 ? 0.f : (s == 1 ? 0.5f * cmin : ldexpf(cmax, min(s - 2, 30)));
        int lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = cell_coord(q[a] - R, m.minv[a], m.inv_cell[a], m.dim[a]);
            hi[a] = cell_coord(q[a] + R, m.minv[a], m.inv_cell[a], m.dim[a]);
            if (s > 0) { lo[a] = min(lo[a], plo[a]); hi[a] = max(hi[a], phi[a]); }      // boxes are nested whatever the rounding does
        }
        // the cells that can hold a point no farther than the current k-th distance; refreshed whenever that distance has dropped
        int clo[3] = {lo[0], lo[1], lo[2]}, chi[3] = {hi[0], hi[1], hi[2]};
        float kth_seen = INFINITY;
        auto clip = [&]() {
            if (kth_d2 == kth_seen) return;
            kth_seen = kth_d2;
            const float rk = sqrtf(kth_d2) * 1.00001f + 1e-30f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float ra = rk + fabsf(q[a]) * 4e-7f;                              // the rounding of q -+ rk itself
                clo[a] = max(lo[a], cell_coord(q[a] - ra, m.minv[a], m.inv_cell[a], m.dim[a]));
                chi[a] = min(hi[a], cell_coord(q[a] + ra, m.minv[a], m.inv_cell[a], m.dim[a]));
            }
        };
        clip();
        for (int gz = lo[2]; gz <= hi[2]; ++gz)
            for (int gy = lo[1]; gy <= hi[1]; ++gy) {
                if (gz < clo[2] || gz > chi[2] || gy < clo[1] || gy > chi[1]) continue;
                const int rb = (gz * m.dim[1] + gy) * m.dim[0];
                const bool seen = s > 0 && gz >= plo[2] && gz <= phi[2] && gy >= plo[1] && gy <= phi[1];
                if (!seen) span(cs[rb + clo[0]], cs[rb + chi[0] + 1]);                   // x is the fastest cell axis: a row of cells is one span
                else {
                    if (clo[0] < plo[0]) span(cs[rb + clo[0]], cs[rb + min(plo[0], chi[0] + 1)]);
                    if (chi[0] > phi[0]) span(cs[rb + max(phi[0], clo[0] - 1) + 1], cs[rb + chi[0] + 1]);
                }
                clip();
            }
        // nearest face of the box that has unread cells behind it
        float face = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float pad = (fabsf(q[a]) + fabsf(m.minv[a]) + m.cell[a] * (float)m.dim[a]) * 4e-6f;
            if (lo[a] > 0) face = fminf(face, q[a] - (m.minv[a] + (float)lo[a] * m.cell[a]) - pad);
            if (hi[a] < m.dim[a] - 1) face = fminf(face, (m.minv[a] + (float)(hi[a] + 1) * m.cell[a]) - q[a] - pad);
            plo[a] = lo[a]; phi[a] = hi[a];
        }
        if (face == INFINITY) done = true;                                               // the box is the whole grid
        else if (face > 0.f && kth_d2 <= face * face * 0.99999f) done = true;
    }
    return done;
}
