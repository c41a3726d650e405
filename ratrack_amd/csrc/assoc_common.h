// Device helpers shared by the B = 1 association kernels (fused_misc.hip: rtk_dbscan, rtk_log_sinkhorn) and their batched
// counterparts (track_batched.hip): one definition of the arithmetic, so the two paths agree bit for bit by construction.
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

// The log-Sinkhorn iterations on an LDS table of a workgroup of 256 threads:
//   iters x { u = log_mu - lse_j(Z + v);  v = log_nu - lse_i(Z + u) }
// Z (m+1, n+1) with row stride ld, u (m+1) and v (n+1) zero on entry; norm = -log(m + n).  logsumexp is evaluated as torch does:
// max + log(sum(exp(x - max))) (tree-summed across the lanes of a DPP row).  One 16-lane DPP row per matrix row (then per
// column), its lanes across the other axis: max and sum are 4 rotate-and-combine DPP steps (a ds_bpermute shuffle chain costs
// ~60 cycles per step; 500 iterations x 2 phases x 12 steps of it were 3 ms).  16 rows per pass over the workgroup.
__device__ __forceinline__ void log_sinkhorn_lds(int m, int n, const float *Z, int ld, float *u, float *v, float norm, int iters) {
    const int R = m + 1, C = n + 1;
    const int t = threadIdx.x, grp = t >> 4, c = t & 15;
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
