// batch_common.h -- device helpers shared by the kernels that work on B streams at once (gt_eval.hip, track_score.hip,
// track_batched.hip): one definition of each, so that the contract they carry is stated once.
#pragma once

#include "rtk_common.h"
#include "rtk_fused.h"

// element (b, c, p) of a (B,C,N) or (B,N) fp32 tensor read in place through its strides
__device__ __forceinline__ float bcn_at(const rtk_bcn_view_t &v, int b, int c, int p) {
    return v.ptr[(long long)b * v.sb + (long long)c * v.sc + (long long)p * v.sp];
}

// a count read from the device, brought into [0, hi]
__device__ __forceinline__ int count_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the sum of x over the lanes up to and including this one (an ordered prefix: lane order is the order of the sum)
__device__ __forceinline__ int wave_inclusive_scan(int x, int lane) {
#pragma unroll
    for (int o = 1; o < RTK_WAVE; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}

// one frame of the batched tracker (rtk_track_frame_t): does stream b take part, and how many of its N columns are points
__device__ __forceinline__ bool stream_active(const rtk_track_frame_t &fr, int b) { return !fr.active || fr.active[b]; }

__device__ __forceinline__ int stream_points(const rtk_track_frame_t &fr, int b) {
    if (!fr.n_valid) return fr.N;
    const int n = fr.n_valid[b];
    return n < 0 ? 0 : (n > fr.N ? fr.N : n);
}

// |(p - c) . R[:,k]| <= half_k on the three axes, closed; the operation order is part of the contract (rtk_gt.h).
__device__ __forceinline__ bool box_inside(const double *bx, double x, double y, double z) {
    const double d0 = x - bx[0], d1 = y - bx[1], d2 = z - bx[2];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double pr = (d0 * bx[3 + k] + d1 * bx[6 + k]) + d2 * bx[9 + k];
        in = in && (fabs(pr) <= bx[12 + k]);
    }
    return in;
}
