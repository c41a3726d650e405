// track_box_step.hip -- Kalman-filtered boxes inside the tracked step (include/rtk_fused.h, "Filtered boxes inside the step";
// ratrack_amd/boxes.py, filter_step_raw; BatchedTracker(box_filter=...)).
//
//   rtk_track_box_filter_step   one workgroup per stream, one lane per row of the tracker's table: the filter state of every row
//                               follows its track id from the previous table to the one this step wrote and takes this frame's box
//
// The arithmetic is box_filter.h's and is stated nowhere else: what the offline launch (csrc/track_box_filter.hip) computes along a
// segment a member at a time, this launch computes a frame at a time, with the 15 doubles of the state kept per row between steps.
// The advance is IN PLACE and a permutation of rows: every lane reads its previous row's 16 words into registers, one
// __syncthreads() follows, and only then does any lane store.  The previous ids go through LDS, where every lane looks its own id up.
// Every output word has one writer and a plain store; the counts are clamped to [0, K], so no table is read or written out of bounds.
#include <math.h>

#include "batch_common.h"
#include "box_filter.h"
#include "rtk_common.h"

#define BXS_THREADS 256
static_assert(RTK_RESULT_MAX_OBJECTS <= BXS_THREADS, "every row of a stream's table has a lane of its own");

struct bxs_io_t {
    const unsigned char *active, *reset;
    const int *ids_prev, *count_prev, *ids_new, *count_new, *num_objects;
    const double *box;
    const int *valid;
    double *state;
    int *since;
    double *out_box;
    int *out_valid;
    double *vel, *aligned;
    int *gap;
};

__global__ __launch_bounds__(BXS_THREADS) void box_filter_step_kernel(int K, const rtk_box_filter_t par, const bxs_io_t io) {
    __shared__ int prev_id[BXS_THREADS];
    const int b = blockIdx.x, r = threadIdx.x;
    const size_t row = (size_t)b * K + r;
    const bool live = !io.active || io.active[b] != 0;
    const bool fresh = io.reset && io.reset[b] != 0;
    const int m = (live && !fresh) ? count_clamp(io.count_prev[b], K) : 0;
    const int c = count_clamp(io.count_new[b], K), n = count_clamp(io.num_objects[b], K);
    prev_id[r] = r < m ? io.ids_prev[(size_t)b * K + r] : -1;
    __syncthreads();

    // ---- read: this row's previous row, its 16 words and its counter ----
    const bool mine = live && r < K && r < c;
    int since_prev = -1;
    double w[16];
    if (mine) {
        const int id = io.ids_new[row];
        int p = -1;
        if (id >= 0)
            for (int i = m - 1; i >= 0; --i) p = prev_id[i] == id ? i : p;      // the smallest i: ids are unique, so at most one
        if (p >= 0) {
            since_prev = io.since[(size_t)b * K + p];
            if (since_prev > RTK_BOX_FILTER_MAX_GAP) since_prev = RTK_BOX_FILTER_MAX_GAP;
            const double *st = io.state + ((size_t)b * K + p) * 16;
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = st[q];
        }
    }
    __syncthreads();      // every row has been read: the stores below may land on any of them
    if (r >= K) return;

    double *ob = io.out_box + row * 8, *ov = io.vel + row * 4, *oa = io.aligned + row * 4;
    int since = -1, gap = -1, ovalid = 0;
    double z[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bxf_state_t s;
    if (mine) {
        const int vin = io.valid[row];
        if (r < n && vin > 0) {
            const double *bx = io.box + row * 8;
            z[0] = bx[0]; z[1] = bx[1]; z[2] = bx[2]; z[3] = bx[6]; z[4] = bx[3]; z[5] = bx[4]; z[6] = bx[5];
            const int k = since_prev + 1;
            if (since_prev >= 0 && k <= par.max_gap) {
#pragma unroll
                for (int q = 0; q < 7; ++q) s.m[q] = w[q];
                s.v[0] = w[7]; s.v[1] = w[8]; s.v[2] = w[9];
                s.P00 = w[10]; s.P01 = w[11]; s.P11 = w[12]; s.Py = w[13]; s.Ps = w[14];
                for (int i = 0; i < k; ++i) bxf_predict(s, par);
                bxf_align(s, z, par);
                bxf_update(s, z, par);
                gap = k;
            } else {
                bxf_start(s, z, par);
            }
            since = 0;
            ovalid = vin;
#pragma unroll
            for (int q = 0; q < 7; ++q) w[q] = s.m[q];
            w[7] = s.v[0]; w[8] = s.v[1]; w[9] = s.v[2];
            w[10] = s.P00; w[11] = s.P01; w[12] = s.P11; w[13] = s.Py; w[14] = s.Ps; w[15] = 0.0;
        } else if (since_prev >= 0) {
            since = since_prev + 1 < RTK_BOX_FILTER_MAX_GAP ? since_prev + 1 : RTK_BOX_FILTER_MAX_GAP;      // carried: w as it was read
        }
    }

    // ---- the outputs: every row of every stream ----
    if (since >= 0) {
        double mm[7], vv[3] = {w[7], w[8], w[9]};
#pragma unroll
        for (int q = 0; q < 7; ++q) mm[q] = w[q];
        for (int i = 0; i < since; ++i) {
#pragma unroll
            for (int q = 0; q < 3; ++q) mm[q] = mm[q] + vv[q];
        }
        bxf_output(mm, vv, ob, ov);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) ob[q] = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) ov[q] = 0.0;
    }
    const bool measured = since == 0;
    oa[0] = measured ? z[3] : 0.0; oa[1] = measured ? z[4] : 0.0; oa[2] = measured ? z[5] : 0.0; oa[3] = measured ? z[6] : 0.0;
    io.out_valid[row] = ovalid;
    io.gap[row] = gap;

    // ---- the state: an inactive stream keeps every bit ----
    if (live) {
        double *st = io.state + row * 16;
#pragma unroll
        for (int q = 0; q < 16; ++q) st[q] = since >= 0 ? w[q] : 0.0;
        io.since[row] = since;
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_track_box_filter_step(int B, int K, const unsigned char *active, const unsigned char *reset, const int *ids_prev,
                                         const int *count_prev, const int *ids_new, const int *count_new, const int *num_objects,
                                         const double *box, const int *valid, const rtk_box_filter_t *par, double *state, int *since,
                                         double *out_box, int *out_valid, double *vel, double *aligned, int *gap, rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535, "track_box_filter_step: B=%d streams", B);
    RTK_REQUIRE(K >= 1 && K <= RTK_RESULT_MAX_OBJECTS, "track_box_filter_step: K=%d outside [1, %d]", K, RTK_RESULT_MAX_OBJECTS);
    if (const int e = bxf_check_ranges("track_box_filter_step", par)) return e;
    RTK_REQUIRE(par->smooth == 0 && par->size_rule == 0,
                "track_box_filter_step: smooth=%d, size_rule=%d: neither is causal (both must be 0; rtk_result_log_filter_boxes has them)",
                par->smooth, par->size_rule);
    RTK_REQUIRE(ids_prev && count_prev && ids_new && count_new && num_objects, "track_box_filter_step: null table");
    RTK_REQUIRE(box && valid, "track_box_filter_step: null input boxes");
    RTK_REQUIRE(state && since && out_box && out_valid && vel && aligned && gap, "track_box_filter_step: null state or output");
    RTK_REQUIRE(out_box != box && out_valid != valid, "track_box_filter_step: the outputs must not alias the input boxes");
    bxs_io_t io;
    io.active = active; io.reset = reset; io.ids_prev = ids_prev; io.count_prev = count_prev; io.ids_new = ids_new; io.count_new = count_new;
    io.num_objects = num_objects; io.box = box; io.valid = valid; io.state = state; io.since = since; io.out_box = out_box;
    io.out_valid = out_valid; io.vel = vel; io.aligned = aligned; io.gap = gap;
    box_filter_step_kernel<<<B, BXS_THREADS, 0, (hipStream_t)stream>>>(K, *par, io);
    RTK_CHECK_LAUNCH("track_box_filter_step");
    return RTK_OK;
}
