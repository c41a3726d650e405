// The association algorithms of the B = 1 kernels (fused_misc.hip: rtk_dbscan, rtk_log_sinkhorn) and of their batched
// counterparts (track_batched.hip), written once: DBSCAN steps 1-4 (dbscan_workgroup) and the log-OT setup, iterations and plan
// (log_ot_lds, log_ot_plan).  The kernels only say where the inputs and the tables live and where the results go,
// so the two paths agree bit for bit by construction.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

// max / sum over the 16 lanes of a DPP row, result in every lane (s_nop 1: a VGPR written by VALU needs 2 wait states
// before a DPP read)
__device__ __forceinline__ float row16_max(float v) {
    asm volatile("s_nop 1\n v_max_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 "v_max_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 "v_max_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 "v_max_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 : "+v"(v));
    return v;
}

__device__ __forceinline__ float row16_sum(float v) {
    asm volatile("s_nop 1\n v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 "v_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 "v_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
                 : "+v"(v));
    return v;
}

// log_optimal_transport (models/utils/track4d_utils.py:405-434) of an m x n score block (row stride score_ld) on the LDS tables
// Z (m+1, n+1; row stride ld), u (m+1), v (n+1) of a workgroup of 256 threads:
//   Z = [[scores, alpha], [alpha, alpha]],  u = v = 0,  norm = -log(m + n),
//   log_mu = (norm, ..., norm, log n + norm),  log_nu = (norm, ..., norm, log m + norm),
//   iters x { u = log_mu - lse_j(Z + v);  v = log_nu - lse_i(Z + u) }.
// Returns norm; plan entry (i, j) is then log_ot_plan(...).  Contains barriers: every thread calls it.  logsumexp is evaluated as
// torch does: max + log(sum(exp(x - max))) (tree-summed across the lanes of a DPP row).  One 16-lane DPP row per matrix row (then
// per column), its lanes across the other axis: max and sum are 4 rotate-and-combine DPP steps (a ds_bpermute shuffle chain costs
// ~60 cycles per step; 500 iterations x 2 phases x 12 steps of it were 3 ms).  16 rows per pass over the workgroup.
__device__ __forceinline__ float log_ot_lds(int m, int n, const float *scores, int score_ld, float alpha, int iters, float *Z, int ld,
                                            float *u, float *v) {
    const int R = m + 1, C = n + 1;
    const int t = threadIdx.x, grp = t >> 4, c = t & 15;
    for (int e = t; e < R * C; e += 256) {
        const int i = e / C, j = e % C;
        Z[i * ld + j] = (i < m && j < n) ? scores[i * score_ld + j] : alpha;
    }
    for (int e = t; e < R; e += 256) u[e] = 0.f;
    for (int e = t; e < C; e += 256) v[e] = 0.f;
    const float norm = -logf((float)m + (float)n);
    __syncthreads();
    const float lmu_last = logf((float)n) + norm, lnu_last = logf((float)m) + norm;
    for (int it = 0; it < iters; ++it) {
        for (int i0 = 0; i0 < R; i0 += 16) {
            const int i = i0 + grp;
            const bool live = i < R;
            float mx = -INFINITY;
            if (live) for (int j = c; j < C; j += 16) mx = fmaxf(mx, Z[i * ld + j] + v[j]);
            mx = row16_max(mx);
            float sum = 0.f;
            if (live) for (int j = c; j < C; j += 16) sum += expf(Z[i * ld + j] + v[j] - mx);
            sum = row16_sum(sum);
            if (live && c == 0) u[i] = (i < m ? norm : lmu_last) - (logf(sum) + mx);
        }
        __syncthreads();
        for (int j0 = 0; j0 < C; j0 += 16) {
            const int j = j0 + grp;
            const bool live = j < C;
            float mx = -INFINITY;
            if (live) for (int i = c; i < R; i += 16) mx = fmaxf(mx, Z[i * ld + j] + u[i]);
            mx = row16_max(mx);
            float sum = 0.f;
            if (live) for (int i = c; i < R; i += 16) sum += expf(Z[i * ld + j] + u[i] - mx);
            sum = row16_sum(sum);
            if (live && c == 0) v[j] = (j < n ? norm : lnu_last) - (logf(sum) + mx);
        }
        __syncthreads();
    }
    return norm;
}

__device__ __forceinline__ float log_ot_plan(const float *Z, int ld, const float *u, const float *v, float norm, int i, int j) {
    return Z[i * ld + j] + u[i] + v[j] - norm;
}

// Ordered compaction over a 256-thread workgroup: the threads with `keep` get consecutive slots in thread order.  Returns the
// thread's slot (meaningful when keep) and the total in *count.  Contains barriers: every thread calls it.
__device__ __forceinline__ int ordered_slot(bool keep, int *s_wave, int *count) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    *count = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return off + __popcll(bal & ((1ull << lane) - 1ull));
}

// DBSCAN's neighbour test on 8 compacted feature channels: float64 distances with numpy's pairwise summation order,
// sqrt(d2) <= eps -- the arithmetic of ratrack_amd/association.dbscan.
#define DB_D 8

__device__ __forceinline__ bool db_adjacent(const float *f, int i, int j, double eps) {
    double q[DB_D];
#pragma unroll
    for (int c = 0; c < DB_D; ++c) {
        const double d = (double)f[i * DB_D + c] - (double)f[j * DB_D + c];
        q[c] = d * d;
    }
    const double d2 = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));      // numpy's 8-wide pairwise sum
    return __dsqrt_rn(d2) <= eps;
}

// DBSCAN of the movers among n columns on one workgroup of 256 threads: sklearn.cluster.DBSCAN(eps, min_samples) of
// models/track4d.py:108-126, which runs on the host behind a device->host copy and a boolean-mask gather.
//   1. ordered compaction of the movers (is_mover(i)) and their 8 distance channels (load(i, fk) writes them to fk);
//   2. core points: closed eps-ball (itself included) holds >= min_samples movers (db_adjacent);
//   3. connected components of the core points under the eps-graph by min-label propagation with pointer jumping;
//   4. sklearn numbers clusters in order of their first core point and fully expands one cluster before starting the next,
//      so: cluster id = rank of the component's smallest core index; a border point (non-core, within eps of a core
//      point; only possible for min_samples > 2) joins the lowest-numbered cluster among its core neighbours; the rest is
//      noise (-1).  emit(k, src[k], cluster) is called once per mover k.
// Tables of n entries each, in LDS or in global memory: f (n, 8) compacted channels, then int src (mover -> column), lab
// (component label: smallest core index, or INT_MAX), aux (core flag, then cluster number + 2 of a representative).
// Returns the mover and cluster counts.  Contains barriers: every thread calls it; a caller that reuses the tables or reads what
// emit wrote from another thread synchronises first.
struct DbCounts { int movers, clusters; };

template <class IsMover, class Load, class Emit>
__device__ __forceinline__ DbCounts dbscan_workgroup(int n, float *f, int *src, int *lab, int *aux, double eps, int min_samples,
                                                     IsMover is_mover, Load load, Emit emit) {
    __shared__ int s_changed, s_C, s_wave[4];
    const int t = threadIdx.x;
    if (t == 0) s_C = 0;
    // ---- 1. ordered compaction ----------------------------------------------------------------------------------------
    int m = 0;                                                     // the same in every thread: ordered_slot returns the total
    for (int base = 0; base < n; base += 256) {
        const int i = base + t;
        const bool mv = i < n && is_mover(i);
        int cnt;
        const int k = m + ordered_slot(mv, s_wave, &cnt);
        if (mv) {
            src[k] = i;
            load(i, f + (size_t)k * DB_D);
        }
        m += cnt;
    }
    __syncthreads();
    // ---- 2. core points -----------------------------------------------------------------------------------------------
    for (int i = t; i < m; i += 256) {
        int cnt = 0;
        for (int j = 0; j < m; ++j) cnt += db_adjacent(f, i, j, eps) ? 1 : 0;
        aux[i] = cnt >= min_samples;
        lab[i] = cnt >= min_samples ? i : 0x7fffffff;
    }
    __syncthreads();
    // ---- 3. components of the core graph ----------------------------------------------------------------------------------
    for (;;) {
        if (t == 0) s_changed = 0;
        __syncthreads();
        for (int i = t; i < m; i += 256) {
            if (!aux[i]) continue;
            int best = lab[i];
            for (int j = 0; j < m; ++j)
                if (aux[j] && lab[j] < best && db_adjacent(f, i, j, eps)) best = lab[j];
            if (best < lab[i]) { lab[i] = best; s_changed = 1; }       // racy reads of lab[j] only ever see smaller, valid labels
        }
        __syncthreads();
        for (int i = t; i < m; i += 256)                               // pointer jumping: label of my label
            if (aux[i]) { const int l = lab[lab[i]]; if (l < lab[i]) lab[i] = l; }
        __syncthreads();
        if (!s_changed) break;
        __syncthreads();
    }
    // ---- 4. cluster numbers, border points, output -------------------------------------------------------------------------
    for (int i = t; i < m; i += 256) {           // representative i (lab[i] == i): its number = representatives before it
        if (aux[i] && lab[i] == i) {
            int r = 0;
            for (int j = 0; j < i; ++j) r += (aux[j] && lab[j] == j) ? 1 : 0;
            aux[i] = 2 + r;                      // >= 2 marks "core + number"; plain core points keep 1
            atomicAdd(&s_C, 1);
        }
    }
    __syncthreads();
    for (int i = t; i < m; i += 256) {
        int out = -1;
        if (aux[i]) {
            out = aux[lab[i]] - 2;
        } else if (min_samples > 2) {
            for (int j = 0; j < m; ++j)
                if (aux[j] && db_adjacent(f, i, j, eps)) {
                    const int c = aux[lab[j]] - 2;
                    out = (out < 0 || c < out) ? c : out;
                }
        }
        emit(i, src[i], out);
    }
    return {m, s_C};
}
