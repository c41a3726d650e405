// box_fit.h -- the minimum-area bird's-eye-view rectangle of one object's points (include/rtk_fused.h, "Oriented boxes"), implemented
// once: track_boxes.hip's two kernels stage an object and call bf_fit_wave; nothing else restates the rule.
//
// One wave fits one object.  The object's (x, y), widened to float64, lie in LDS (2 KiB per wave at the cap); every lane takes the
// candidates c = lane, lane + 64, ... in increasing c and evaluates each with ONE loop over the points in point order -- every lane
// reads the same LDS address, a broadcast -- so a candidate's extremes and area are computed by a single lane with the statement's own
// sequence of operations, whatever the decomposition.  A lane keeps its best (area, c) under a strict <, the wave takes the
// lexicographic minimum of the 64 pairs, and every lane recomputes the winner's extremes for the output words, which lane 0 stores.
// The extremes of z (and of x and y for an object above the cap) come from lane-local running extremes and a butterfly; the rule takes
// a zero extreme as +0, so the order of those comparisons cannot show in a bit.
#pragma once
#include <math.h>

#include "batch_common.h"

#define BF_PI 3.14159265358979323846      // the float64 nearest pi; BF_PI / 2 is exact

// lane-local running extremes of x, y, z over the points a lane has seen, and whether one of their coordinates was not finite
struct bf_range_t {
    double lo[3], hi[3];
    int bad;
};

__device__ __forceinline__ void bf_range_init(bf_range_t &r) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { r.lo[a] = INFINITY; r.hi[a] = -INFINITY; }
    r.bad = 0;
}

__device__ __forceinline__ void bf_range_add(bf_range_t &r, double x, double y, double z) {
    const double v[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!__builtin_isfinite(v[a])) r.bad = 1;
        r.lo[a] = v[a] < r.lo[a] ? v[a] : r.lo[a];
        r.hi[a] = v[a] > r.hi[a] ? v[a] : r.hi[a];
    }
}

// the wave's extremes in every lane (min and max pick one of their arguments: no rounding, any order) with a zero taken as +0
__device__ __forceinline__ void bf_range_reduce(bf_range_t &r) {
#pragma unroll
    for (int o = RTK_WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double l = __shfl_xor(r.lo[a], o), h = __shfl_xor(r.hi[a], o);
            r.lo[a] = l < r.lo[a] ? l : r.lo[a];
            r.hi[a] = h > r.hi[a] ? h : r.hi[a];
        }
        r.bad |= __shfl_xor(r.bad, o);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { r.lo[a] += 0.0; r.hi[a] += 0.0; }
}

// the extremes of s_k = dx x_k + dy y_k and t_k = dx y_k - dy x_k over the staged points, in point order; a zero extreme is +0
struct bf_extent_t { double s0, s1, t0, t1; };

__device__ __forceinline__ bf_extent_t bf_extents(const double2 *xy, int n, double dx, double dy) {
    bf_extent_t e = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int k = 0; k < n; ++k) {
        const double2 p = xy[k];
        const double s = dx * p.x + dy * p.y, t = dx * p.y - dy * p.x;
        e.s0 = s < e.s0 ? s : e.s0;
        e.s1 = s > e.s1 ? s : e.s1;
        e.t0 = t < e.t0 ? t : e.t0;
        e.t1 = t > e.t1 ? t : e.t1;
    }
    e.s0 += 0.0; e.s1 += 0.0; e.t0 += 0.0; e.t1 += 0.0;
    return e;
}

__device__ __forceinline__ double bf_area(const bf_extent_t &e, double q) { return ((e.s1 - e.s0) * (e.t1 - e.t0)) / q; }

// the eight box words from the winning direction, its extremes and the z range ("From the winner")
__device__ __forceinline__ void bf_store(double dx, double dy, double q, const bf_extent_t &e, double zlo, double zhi, double min_extent, double *box) {
    const double S = e.s1 - e.s0, T = e.t1 - e.t0;
    const double area = (S * T) / q;
    const double r = sqrt(q);
    double len_s = S / r, len_t = T / r;
    const double ms = (e.s0 + e.s1) / 2.0, mt = (e.t0 + e.t1) / 2.0;
    const double cx = (ms * dx - mt * dy) / q, cy = (ms * dy + mt * dx) / q;
    double yaw = atan2(dy, dx);
    if (len_t > len_s) {
        const double v = len_s;
        len_s = len_t;
        len_t = v;
        yaw = yaw + BF_PI / 2.0;
    }
    while (yaw >= BF_PI / 2.0) yaw = yaw - BF_PI;
    while (yaw < -(BF_PI / 2.0)) yaw = yaw + BF_PI;
    const double h = zhi - zlo;
    box[0] = cx;
    box[1] = cy;
    box[2] = (zlo + zhi) / 2.0;
    box[3] = len_s > min_extent ? len_s : min_extent;
    box[4] = len_t > min_extent ? len_t : min_extent;
    box[5] = h > min_extent ? h : min_extent;
    box[6] = yaw;
    box[7] = area;
}

__device__ __forceinline__ void bf_store_empty(double *box, int *cand, int *valid, int code, int lane) {
    if (lane < 8) box[lane] = 0.0;
    if (lane == 0) { *cand = -1; *valid = code; }
}

// xy must be visible to the whole wave before the search reads it, and read before the next object overwrites it
__device__ __forceinline__ void bf_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave, all 64 lanes: the object of n >= 0 points whose first min(n, RTK_BOX_MAX_POINTS) BEV coordinates the wave has written to
// xy (none need be written when n is above the cap) and whose coordinates all went through the lanes' `rg`.  Writes the object's eight
// box words, cand and valid; -> whether the object was above the cap (fitted axis-aligned).  n is the same in every lane.
__device__ __forceinline__ bool bf_fit_wave(const double2 *xy, int n, bf_range_t &rg, double min_extent, double *box, int *cand, int *valid, int lane) {
    if (n <= 0) {
        bf_store_empty(box, cand, valid, 0, lane);
        return false;
    }
    bf_range_reduce(rg);
    if (rg.bad) {
        bf_store_empty(box, cand, valid, -1, lane);
        return false;
    }
    if (n > RTK_BOX_MAX_POINTS) {      // candidate 0 alone: s = x, t = y, q = 1
        const bf_extent_t e = {rg.lo[0], rg.hi[0], rg.lo[1], rg.hi[1]};
        if (lane == 0) {
            bf_store(1.0, 0.0, 1.0, e, rg.lo[2], rg.hi[2], min_extent, box);
            *cand = 0;
            *valid = n;
        }
        return true;
    }
    bf_wave_sync();
    // ---- the search: candidate 0 is (1, 0); candidate c >= 1 is the pair of rank c - 1, (0, c) before its row is found ----
    const int total = n * (n - 1) / 2;
    double best = INFINITY;
    int best_c = 0x7fffffff, best_ij = 0;
    int c = lane, i = 0, j = lane;
    if (c == 0) {
        best = bf_area(bf_extents(xy, n, 1.0, 0.0), 1.0);
        best_c = 0;
        c = RTK_WAVE;
        j = RTK_WAVE;
    }
    for (; c <= total; c += RTK_WAVE, j += RTK_WAVE) {
        while (j >= n) {      // past the end of row i (columns i + 1 .. n - 1): on into row i + 1
            j = j - n + i + 2;
            ++i;
        }
        const double2 a = xy[i], b = xy[j];
        const double dx = b.x - a.x, dy = b.y - a.y;
        const double q = dx * dx + dy * dy;
        if (q == 0.0) continue;
        const double area = bf_area(bf_extents(xy, n, dx, dy), q);
        if (area < best) {
            best = area;
            best_c = c;
            best_ij = (i << 8) | j;
        }
    }
#pragma unroll
    for (int o = RTK_WAVE / 2; o > 0; o >>= 1) {
        const double a2 = __shfl_xor(best, o);
        const int c2 = __shfl_xor(best_c, o), ij2 = __shfl_xor(best_ij, o);
        if (a2 < best || (a2 == best && c2 < best_c)) {
            best = a2;
            best_c = c2;
            best_ij = ij2;
        }
    }
    // ---- the winner's words ----
    double dx = 1.0, dy = 0.0, q = 1.0;
    if (best_c > 0) {
        const double2 a = xy[best_ij >> 8], b = xy[best_ij & 255];
        dx = b.x - a.x;
        dy = b.y - a.y;
        q = dx * dx + dy * dy;
    }
    const bf_extent_t e = bf_extents(xy, n, dx, dy);
    if (lane == 0) {
        bf_store(dx, dy, q, e, rg.lo[2], rg.hi[2], min_extent, box);
        *cand = best_c;
        *valid = n;
    }
    bf_wave_sync();
    return false;
}
