// box_filter.h -- the arithmetic of the track box filter (include/rtk_fused.h, "Filtered boxes"), stated once: the chain of one segment,
// a member at a time.  Everything is float64, every sum, product and quotient an operation of its own (the build passes
// -ffp-contract=off), nothing transcendental; floor is exact.  csrc/track_box_filter.hip holds the walks and calls these in the order
// the header names.  A state is 15 doubles and lives in the registers of the one lane that walks its segment.
#pragma once
#include <math.h>

#include "box_fit.h"      // BF_PI
#include "rtk_common.h"
#include "rtk_fused.h"

struct bxf_state_t {
    double m[7];                        // x, y, z, yaw, l, w, h
    double v[3];                        // vx, vy, vz
    double P00, P01, P11, Py, Ps;       // the covariance the three (coordinate, velocity) pairs share; the yaw's; the three sizes'
};

// the start of a segment: the measurement itself, at rest
__device__ __forceinline__ void bxf_start(bxf_state_t &s, const double *z, const rtk_box_filter_t &p) {
#pragma unroll
    for (int c = 0; c < 7; ++c) s.m[c] = z[c];
    s.v[0] = s.v[1] = s.v[2] = 0.0;
    s.P00 = p.p0; s.P01 = 0.0; s.P11 = p.p0_vel; s.Py = p.p0; s.Ps = p.p0;
}

// one frame passes
__device__ __forceinline__ void bxf_predict(bxf_state_t &s, const rtk_box_filter_t &p) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s.m[c] = s.m[c] + s.v[c];
    const double a = s.P00 + s.P01, b = s.P01 + s.P11;
    s.P00 = (a + b) + p.q_pos;
    s.P01 = b;
    s.P11 = s.P11 + p.q_vel;
    s.Py = s.Py + p.q_yaw;
    s.Ps = s.Ps + p.q_size;
}

// the measurement z = (x, y, z, yaw, l, w, h) read against the state's yaw: z[3] the nearest of its symmetric copies, l and w swapped
// where that copy is an odd number of quarter turns away (symmetry 4)
__device__ __forceinline__ void bxf_align(const bxf_state_t &s, double *z, const rtk_box_filter_t &p) {
    const double H = (2.0 * BF_PI) / (double)p.symmetry;
    const double d = z[3] - s.m[3];
    const double t = floor(d / H + 0.5);
    z[3] = s.m[3] + (d - t * H);
    if (p.symmetry == 4 && t - 2.0 * floor(t / 2.0) == 1.0) {
        const double l = z[4];
        z[4] = z[5];
        z[5] = l;
    }
}

// the aligned measurement enters the state
__device__ __forceinline__ void bxf_update(bxf_state_t &s, const double *z, const rtk_box_filter_t &p) {
    const double S = s.P00 + p.r_pos, K0 = s.P00 / S, K1 = s.P01 / S;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double y = z[c] - s.m[c];
        s.m[c] = s.m[c] + K0 * y;
        s.v[c] = s.v[c] + K1 * y;
    }
    s.P11 = s.P11 - K1 * s.P01;
    s.P01 = (1.0 - K0) * s.P01;
    s.P00 = (1.0 - K0) * s.P00;
    const double Ky = s.Py / (s.Py + p.r_yaw);
    s.m[3] = s.m[3] + Ky * (z[3] - s.m[3]);
    s.Py = (1.0 - Ky) * s.Py;
    const double Ks = s.Ps / (s.Ps + p.r_size);
#pragma unroll
    for (int c = 4; c < 7; ++c) s.m[c] = s.m[c] + Ks * (z[c] - s.m[c]);
    s.Ps = (1.0 - Ks) * s.Ps;
}

// the backward step: s, the filtered state of a member, becomes its smoothed mean given its successor's smoothed mean (nm, nv) k frames on
__device__ __forceinline__ void bxf_smooth(bxf_state_t &s, int k, const double *nm, const double *nv, const rtk_box_filter_t &p) {
    bxf_state_t q = s;
    for (int i = 0; i < k; ++i) bxf_predict(q, p);
    const double kk = (double)k;
    const double C00 = s.P00 + kk * s.P01, C01 = s.P01, C10 = s.P01 + kk * s.P11, C11 = s.P11;
    const double det = q.P00 * q.P11 - q.P01 * q.P01;
    const double G00 = (C00 * q.P11 - C01 * q.P01) / det, G01 = (C01 * q.P00 - C00 * q.P01) / det;
    const double G10 = (C10 * q.P11 - C11 * q.P01) / det, G11 = (C11 * q.P00 - C10 * q.P01) / det;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e0 = nm[c] - q.m[c], e1 = nv[c] - q.v[c];
        s.m[c] = s.m[c] + (G00 * e0 + G01 * e1);
        s.v[c] = s.v[c] + (G10 * e0 + G11 * e1);
    }
    const double Gy = s.Py / q.Py, Gs = s.Ps / q.Ps;
    s.m[3] = s.m[3] + Gy * (nm[3] - s.m[3]);
#pragma unroll
    for (int c = 4; c < 7; ++c) s.m[c] = s.m[c] + Gs * (nm[c] - s.m[c]);
}

// a final mean as a row of the ObjectBoxes layout and its velocity row
__device__ __forceinline__ void bxf_output(const double *m, const double *v, double *box, double *vel) {
    double l = m[4], w = m[5], yaw = m[3];
    if (w > l) {
        const double x = l;
        l = w;
        w = x;
        yaw = yaw + BF_PI / 2.0;
    }
    yaw = yaw - floor((yaw + BF_PI / 2.0) / BF_PI) * BF_PI;
    if (yaw >= BF_PI / 2.0) yaw = yaw - BF_PI;
    else if (yaw < -(BF_PI / 2.0)) yaw = yaw + BF_PI;
    box[0] = m[0]; box[1] = m[1]; box[2] = m[2]; box[3] = l; box[4] = w; box[5] = m[6]; box[6] = yaw; box[7] = l * w;
    vel[0] = v[0]; vel[1] = v[1]; vel[2] = v[2]; vel[3] = m[3];
}

// host side: the ranges of rtk_box_filter_t outside which both launches refuse the call (who: the entry point, for the message)
static inline bool bxf_positive(double x) { return isfinite(x) && x > 0.0; }
static inline bool bxf_not_negative(double x) { return isfinite(x) && x >= 0.0; }

static inline int bxf_check_ranges(const char *who, const rtk_box_filter_t *par) {
    RTK_REQUIRE(par, "%s: null parameters", who);
    RTK_REQUIRE(bxf_positive(par->r_pos) && bxf_positive(par->r_yaw) && bxf_positive(par->r_size),
                "%s: r_pos=%g, r_yaw=%g, r_size=%g: finite numbers > 0", who, par->r_pos, par->r_yaw, par->r_size);
    RTK_REQUIRE(bxf_not_negative(par->q_pos) && bxf_not_negative(par->q_vel) && bxf_not_negative(par->q_yaw) && bxf_not_negative(par->q_size),
                "%s: q_pos=%g, q_vel=%g, q_yaw=%g, q_size=%g: finite numbers >= 0", who, par->q_pos, par->q_vel, par->q_yaw, par->q_size);
    RTK_REQUIRE(bxf_positive(par->p0) && bxf_positive(par->p0_vel), "%s: p0=%g, p0_vel=%g: finite numbers > 0", who, par->p0, par->p0_vel);
    RTK_REQUIRE(par->symmetry == 2 || par->symmetry == 4, "%s: symmetry=%d is neither 2 nor 4", who, par->symmetry);
    RTK_REQUIRE(par->max_gap >= 1 && par->max_gap <= RTK_BOX_FILTER_MAX_GAP, "%s: max_gap=%d outside [1, %d]", who, par->max_gap,
                RTK_BOX_FILTER_MAX_GAP);
    RTK_REQUIRE((par->smooth == 0 || par->smooth == 1) && (par->size_rule == 0 || par->size_rule == 1) && par->size_percent >= 0 &&
                    par->size_percent <= 100,
                "%s: smooth=%d, size_rule=%d (0 or 1 each), size_percent=%d (0 ... 100)", who, par->smooth, par->size_rule, par->size_percent);
    return RTK_OK;
}
