// lds_assignment.h -- an exact maximum-weight one-to-one assignment in a sparse bipartite graph, solved by ONE wave with every table in
// LDS (track_identity.hip closes a clip with it; a per-frame optimal match of detections to objects can use it as it stands).
//
// The problem.  R rows, C columns and E edges (row, column, weight > 0), no (row, column) twice.  A matching takes every row and every
// column at most once; la_solve returns the largest sum of weights a matching can have.  That number is unique even where the best
// matching is not, and it is all that comes out: the matching itself stays in the tables (cp, below) and depends on nothing but the
// edge SET, since every choice is broken by the smaller column index.
//
// The method.  Successive shortest augmenting paths with potentials (the Hungarian method in its Dijkstra form), as a minimisation of
// cost = -weight in which every row also owns a private column of cost 0 ("stays unmatched"), so that every row can always be served:
//   u[row] <= 0, v[column] <= 0, u + v <= cost on every edge and = cost on the matched ones; a free column has v = 0;
//   rows enter one at a time.  The new row r starts with u[r] = min(0, min over its edges of cost - v), which makes the reduced costs
//   cost - u - v of its edges >= 0, as all others are already.  A Dijkstra search over the columns then grows a tree from r: the lanes
//   relax the edges of the row just reached, scan the columns for the nearest one not yet in the tree (ties: the smaller index) and
//   agree on it by a wave reduction; a column that is matched leads on to its row.  The search ends at the first free column, or at
//   the private column of a row of the tree as soon as that is no farther (distance of the row - u[row]: that row then gives its
//   column up and stays unmatched for good -- nothing but itself reaches its private column, so no later tree contains it); the
//   potentials of the tree move by the final distance minus their own, the path is flipped, and the matching of the rows entered so
//   far is optimal again.
// Exact: integers only.  With weights <= W every potential stays in [-W, 0] and every distance in [0, 2 W]: W below 2^29 cannot overflow
// an int.  Bounded: a search puts one more column into its tree per round, so it makes at most C + 1 rounds (the loop is counted, not
// open), R searches in all; no input within the sizes can spin it.  Cost: a round is a handful of LDS round trips plus ceil(C / 64)
// reads per lane, and a solve is at worst R * (min(R, C) + 1) rounds -- 32 x 32 with every edge present took 151 where it was counted.
//
// The contract.
//   * called by all 64 lanes of a one-wave workgroup (blockDim.x == RTK_WAVE) with identical arguments, from uniform control flow;
//     it synchronises with __syncthreads() and every lane returns the same value;
//   * ekey[e] = row << LA_COL_BITS | column and ew[e] = weight for e < E, in LDS, only read; 0 <= row < R, 0 <= column < C < 2^LA_COL_BITS,
//     0 < weight < 2^29, E >= 0.  An edge outside these ranges is the caller's error (it would index the tables out of range);
//   * work: la_words(R, C, E) ints of LDS that overlap neither ekey nor ew; what they held is lost.  After the call cp (work +
//     la_cp_offset(R, C, E)) holds the row matched to every column, -1 for none;
//   * no floating point, no scratch, no inline assembly, no global memory.
#pragma once
#include "rtk_common.h"

#define LA_COL_BITS 12
#define LA_INF 0x7fffffff

// row starts [R + 1] | adjacency column, weight [E] each | u [R] | v, dist, way, cp, done [C] each
__host__ __device__ constexpr int la_words(int R, int C, int E) { return (R + 1) + 2 * E + R + 5 * C; }
__host__ __device__ constexpr int la_cp_offset(int R, int C, int E) { return (R + 1) + 2 * E + R + 3 * C; }

// the smallest value of the wave, in every lane
__device__ __forceinline__ unsigned long long la_wave_min(unsigned long long x) {
#pragma unroll
    for (int o = RTK_WAVE / 2; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)x, o), hi = __shfl_xor((unsigned)(x >> 32), o);
        const unsigned long long y = ((unsigned long long)hi << 32) | lo;
        x = y < x ? y : x;
    }
    return x;
}

__device__ __forceinline__ long long la_wave_sum(long long x) {
#pragma unroll
    for (int o = RTK_WAVE / 2; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)x, o), hi = __shfl_xor((unsigned)((unsigned long long)x >> 32), o);
        x += (long long)(((unsigned long long)hi << 32) | lo);
    }
    return x;
}

__device__ __forceinline__ int la_wave_inclusive_scan(int x, int lane) {
#pragma unroll
    for (int o = 1; o < RTK_WAVE; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}

__device__ inline long long la_solve(int R, int C, int E, const int *ekey, const int *ew, int *work) {
    const int t = threadIdx.x;
    int *rs = work, *ac = rs + (R + 1), *aw = ac + E, *u = aw + E;
    int *v = u + R, *dist = v + C, *way = dist + C, *cp = way + C, *done = cp + C;
    constexpr int COL_MASK = (1 << LA_COL_BITS) - 1;

    // ---- the rows' edges side by side: counts, their running sum, then every edge into its row's span (u lends the cursors) ----
    for (int i = t; i <= R; i += RTK_WAVE) rs[i] = 0;
    for (int j = t; j < C; j += RTK_WAVE) { v[j] = 0; cp[j] = -1; }
    __syncthreads();
    for (int e = t; e < E; e += RTK_WAVE) atomicAdd(&rs[(ekey[e] >> LA_COL_BITS) + 1], 1);
    __syncthreads();
    {
        const int chunk = (R + RTK_WAVE - 1) / RTK_WAVE, lo = min(t * chunk, R), hi = min(lo + chunk, R);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += rs[i + 1];
        int run = la_wave_inclusive_scan(sum, t) - sum;      // the edges of the rows before this lane's
        for (int i = lo; i < hi; ++i) { u[i] = run; run += rs[i + 1]; rs[i + 1] = run; }
    }
    __syncthreads();
    for (int e = t; e < E; e += RTK_WAVE) {
        const int key = ekey[e], at = atomicAdd(&u[key >> LA_COL_BITS], 1);
        ac[at] = key & COL_MASK;
        aw[at] = ew[e];
    }
    __syncthreads();

    // ---- one search per row ----
    for (int r = 0; r < R; ++r) {
        const int r0 = rs[r], r1 = rs[r + 1];
        if (r0 == r1) continue;      // a row without an edge stays unmatched
        // u[r] = min(0, min over the row's edges of cost - v) = -(the largest weight + v, at least 0)
        int most = 0;
        for (int e = r0 + t; e < r1; e += RTK_WAVE) most = max(most, aw[e] + v[ac[e]]);
        const int ur = (int)la_wave_min((unsigned long long)(LA_INF - most)) - LA_INF;
        for (int j = t; j < C; j += RTK_WAVE) { dist[j] = LA_INF; done[j] = 0; }
        if (t == 0) u[r] = ur;
        __syncthreads();
        int i = r, base = 0, jin = -1;    // the row just reached, its distance, the column it was reached through
        int dd = LA_INF, jdd = -1;        // the nearest private column of a row of the tree, and the column THAT row was reached through
        int D = 0, jend = -1;             // the search's result: the final distance and the column the flip starts at (-1: nothing flips)
        for (int round = 0; round <= C; ++round) {
            const int e0 = rs[i], e1 = rs[i + 1], ui = u[i];
            if (base - ui < dd) { dd = base - ui; jdd = jin; }      // row i could end the path by staying unmatched
            for (int e = e0 + t; e < e1; e += RTK_WAVE) {
                const int j = ac[e];
                if (done[j]) continue;
                const int nd = base + (-aw[e] - ui - v[j]);
                if (nd < dist[j]) { dist[j] = nd; way[j] = jin; }      // the row's columns are distinct: no two lanes meet
            }
            __syncthreads();
            unsigned long long near = ((unsigned long long)LA_INF << 32) | 0xffffffffu;
            for (int j = t; j < C; j += RTK_WAVE) {
                const int d = dist[j];
                if (!done[j] && d != LA_INF) near = min(near, ((unsigned long long)(unsigned)d << 32) | (unsigned)j);
            }
            near = la_wave_min(near);
            const int d = (int)(near >> 32), j = (int)(unsigned)near;
            if (d == LA_INF || dd <= d) { D = dd; jend = jdd; break; }      // nothing left to reach, or a private column is no farther
            const int owner = cp[j];
            __syncthreads();                        // every lane has read done and cp before lane 0 marks the column
            if (t == 0) done[j] = 1;
            if (owner < 0) { D = d; jend = j; break; }
            i = owner; base = d; jin = j;
            __syncthreads();
        }
        __syncthreads();
        // ---- the tree's potentials move by what the search still had to go from each of them ----
        for (int j = t; j < C; j += RTK_WAVE) {
            if (!done[j]) continue;
            const int gap = D - dist[j], owner = cp[j];
            v[j] -= gap;
            if (owner >= 0) u[owner] += gap;      // one row per column: no two lanes meet
        }
        if (t == 0) u[r] += D;
        __syncthreads();
        // ---- and the path is flipped, from its free end back to r (ending at a private column: from the column its row gives up) ----
        if (t == 0) {
            int j = jend;
            for (int step = 0; step < C && j >= 0; ++step) {
                const int jp = way[j];
                cp[j] = jp < 0 ? r : cp[jp];
                j = jp;
            }
        }
        __syncthreads();
    }
    // ---- the weight of the matching, edge by edge ----
    long long sum = 0;
    for (int e = t; e < E; e += RTK_WAVE) {
        const int key = ekey[e];
        if (cp[key & COL_MASK] == (key >> LA_COL_BITS)) sum += ew[e];
    }
    return la_wave_sum(sum);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// la_solve_dense -- the same problem on a DENSE block of weights (track_assign.hip: the batched tracker's exact association).  An
// R x C block as an edge list costs la_solve 4 E ints of LDS, 256 KiB at 128 x 128; here the block itself is the adjacency:
// w[i * ld + j] is the weight of pair (row i, column j), 0 = no edge.
//
// The method is la_solve's, statement for statement: successive shortest augmenting paths with potentials on cost = -weight, every
// row owning a private "stays unmatched" column of cost 0; rows enter in index order; the nearest column wins, ties go to the smaller
// column index, and a private column that is no farther than the nearest column ends the search.  So the matching is the one la_solve
// leaves for the edge set {(i, j, w[i * ld + j]) : w > 0}, and it depends on nothing but the block.
// What differs is who holds what.  Lane t owns the columns j = t, t + 64, ...: their dist, way and done words are read and written by
// that lane alone, and one pass over a lane's columns both relaxes them from the row just reached and finds the lane's nearest, so a
// search round is one pass (ceil(C / 64) reads of w, v, dist, done per lane), one wave reduction and two broadcast reads (cp of the
// chosen column, u of its row) -- and no barrier: during a search u, v, cp and w are only read.  The three barriers per row stand
// between the search, the move of the potentials (which reads cp), the flip of the path (which writes cp) and the next row.
// Exact and bounded as la_solve is: integers only, potentials in [-W, 0], distances in [0, 2 W]; a search makes at most C + 1 rounds
// (counted), there are R searches, a flip makes at most C steps (counted).
//
// The contract.
//   * called by all 64 lanes of a one-wave workgroup (blockDim.x == RTK_WAVE) with identical arguments, from uniform control flow;
//     it synchronises with __syncthreads() and every lane returns the same value: the weight of the matching;
//   * w: in LDS, only read; rows i < R, columns j < C, row stride ld >= C; every word is 0 or in (0, 2^29); R >= 0, C >= 0;
//   * work: la_dense_words(R, C) ints of LDS that do not overlap w; what they held is lost.  After the call cp (work +
//     la_dense_cp_offset(R, C)) holds the row matched to every column, -1 for none;
//   * no floating point, no scratch, no inline assembly, no global memory.
// ------------------------------------------------------------------------------------------------------------------------------------
// u [R] | v, dist, way, cp, done [C] each
__host__ __device__ constexpr int la_dense_words(int R, int C) { return R + 5 * C; }
__host__ __device__ constexpr int la_dense_cp_offset(int R, int C) { return R + 3 * C; }

__device__ inline long long la_solve_dense(int R, int C, const int *w, int ld, int *work) {
    const int t = threadIdx.x;
    int *u = work, *v = u + R, *dist = v + C, *way = dist + C, *cp = way + C, *done = cp + C;
    for (int j = t; j < C; j += RTK_WAVE) { v[j] = 0; cp[j] = -1; }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        // u[r] = min(0, min over the row's edges of cost - v) = -(the largest weight + v, at least 0); the lane's columns start a search
        const int *wr = w + (size_t)r * ld;
        int most = 0;
        for (int j = t; j < C; j += RTK_WAVE) {
            const int wj = wr[j];
            if (wj > 0) most = max(most, wj + v[j]);
            dist[j] = LA_INF; done[j] = 0;
        }
        const int ur = (int)la_wave_min((unsigned long long)(LA_INF - most)) - LA_INF;
        int i = r, ui = ur, base = 0, jin = -1;      // the row just reached, its potential and distance, the column it was reached through
        int dd = LA_INF, jdd = -1;                   // the nearest private column of a row of the tree, and the column THAT row was reached through
        int D = 0, jend = -1;                        // the search's result: the final distance and the column the flip starts at (-1: nothing flips)
        for (int round = 0; round <= C; ++round) {
            if (base - ui < dd) { dd = base - ui; jdd = jin; }      // row i could end the path by staying unmatched
            const int *wi = w + (size_t)i * ld;
            unsigned long long near = ((unsigned long long)LA_INF << 32) | 0xffffffffu;
            for (int j = t; j < C; j += RTK_WAVE) {
                if (done[j]) continue;
                int d = dist[j];
                const int wj = wi[j];
                if (wj > 0) {
                    const int nd = base + (-wj - ui - v[j]);
                    if (nd < d) { d = nd; dist[j] = nd; way[j] = jin; }
                }
                if (d != LA_INF) near = min(near, ((unsigned long long)(unsigned)d << 32) | (unsigned)j);
            }
            near = la_wave_min(near);
            const int d = (int)(near >> 32), j = (int)(unsigned)near;
            if (d == LA_INF || dd <= d) { D = dd; jend = jdd; break; }      // nothing left to reach, or a private column is no farther
            const int owner = cp[j];
            if ((j & (RTK_WAVE - 1)) == t) done[j] = 1;                     // the column's own lane: no other reads the word
            if (owner < 0) { D = d; jend = j; break; }
            i = owner; ui = u[owner]; base = d; jin = j;
        }
        __syncthreads();
        // ---- the tree's potentials move by what the search still had to go from each of them ----
        for (int j = t; j < C; j += RTK_WAVE) {
            if (!done[j]) continue;
            const int gap = D - dist[j], owner = cp[j];
            v[j] -= gap;
            if (owner >= 0) u[owner] += gap;      // one row per column: no two lanes meet
        }
        if (t == 0) u[r] = ur + D;                // r owns no column yet: no lane above wrote it
        __syncthreads();
        // ---- and the path is flipped, from its free end back to r (ending at a private column: from the column its row gives up) ----
        if (t == 0) {
            int j = jend;
            for (int step = 0; step < C && j >= 0; ++step) {
                const int jp = way[j];
                cp[j] = jp < 0 ? r : cp[jp];
                j = jp;
            }
        }
        __syncthreads();
    }
    // ---- the weight of the matching, column by column ----
    long long sum = 0;
    for (int j = t; j < C; j += RTK_WAVE) {
        const int i = cp[j];
        if (i >= 0) sum += w[(size_t)i * ld + j];
    }
    return la_wave_sum(sum);
}
