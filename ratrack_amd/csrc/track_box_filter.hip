// track_box_filter.hip -- Kalman-filtered, track-consistent boxes over the result log (include/rtk_fused.h, "Filtered boxes";
// ratrack_amd/boxes.py, ResultLog.filter_boxes).
//
//   rtk_result_log_filter_boxes   one workgroup per stream: the records of every (clip, track id) are linked into segments, the filter
//                                 runs along each segment, optionally backwards again (the smoother), and every record below the
//                                 stream's cursor gets its box, velocity, filter state, aligned reading and links
//
// The arithmetic is box_filter.h's and is stated nowhere else; this file holds the walks, in four stages behind __syncthreads():
//   links    clip after clip: the clip's ids enter the track table (score_log_walk.h's, as rtk_result_log_select fills it), then the
//            clip's frames are walked in order, one thread per record of the frame.  Beside its key a slot keeps its track's last member
//            and that member's frame number; the duplicate rule is an integer atomicMin on the record index.  A member's thread writes
//            its prev | gap words and its predecessor's next word; the -1 of a track's last member is written when the clip closes.
//            Every non-member is written as empty here.
//   forward  one lane per segment (the lane that finds a member without a predecessor) walks the chain with the 15 doubles of the
//            state in registers: state, aligned and the link's `first` word.
//   extent   (size_rule 1) every member counts the (value, record) pairs of its segment below its own along the chain; the member
//            of the wanted rank publishes the value in LDS -- the tables' 48 KiB, free by now, hold three doubles for each of 2048
//            record slots, so segments are served in windows of 2048 by their first member's index.
//   finish   the segment's lane again: forwards over the stored filtered means, or to the chain's end and backwards with the smoother;
//            it writes box and vel.
// Every output word has one writer and plain stores; the flags word is gathered with an integer OR in LDS and stored by thread 0.
// Every index read back from `link` is checked against the stream's cursor and every chain walk ends after `records` steps, so a
// foreign log (frames that overlap) can neither be followed out of bounds nor around a cycle.
#include <math.h>

#include "box_filter.h"
#include "score_log_walk.h"

#define BXF_THREADS 256
#define BXF_NONE 0x7fffffff
#define BXF_WINDOW RTK_SCORE_SWEEP_TRACKS      // record slots whose three extent values the pool holds at a time
static_assert(RTK_SCORE_MAX_OBJECTS <= BXF_THREADS, "the frame walk gives every record of a frame a thread of its own");
static_assert(BXF_WINDOW * 3 * sizeof(double) >= 4 * LW_SLOTS * sizeof(int), "the pool holds the four tables of the link stage");

struct bxf_io_t {
    const unsigned char *keep;
    const double *box;
    const int *valid;
    double *out_box;
    int *out_valid;
    double *vel, *state, *aligned;
    int *link, *flags;
};

__device__ __forceinline__ void bxf_store_empty(const bxf_io_t &io, size_t r) {
#pragma unroll
    for (int c = 0; c < 8; ++c) io.out_box[r * 8 + c] = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) { io.vel[r * 4 + c] = 0.0; io.aligned[r * 4 + c] = 0.0; }
#pragma unroll
    for (int c = 0; c < 16; ++c) io.state[r * 16 + c] = 0.0;
    *reinterpret_cast<int4 *>(io.link + r * 4) = make_int4(-1, -1, -1, -1);
    io.out_valid[r] = 0;
}

// a record's box (cx, cy, cz, l, w, h, yaw, area) as the measurement (x, y, z, yaw, l, w, h)
__device__ __forceinline__ void bxf_measurement(const double *box, double *z) {
    z[0] = box[0]; z[1] = box[1]; z[2] = box[2]; z[3] = box[6]; z[4] = box[3]; z[5] = box[4]; z[6] = box[5];
}

__device__ __forceinline__ void bxf_store_state(const bxf_io_t &io, size_t r, const bxf_state_t &s, const double *z) {
    double *st = io.state + r * 16, *al = io.aligned + r * 4;
#pragma unroll
    for (int c = 0; c < 7; ++c) st[c] = s.m[c];
    st[7] = s.v[0]; st[8] = s.v[1]; st[9] = s.v[2];
    st[10] = s.P00; st[11] = s.P01; st[12] = s.P11; st[13] = s.Py; st[14] = s.Ps; st[15] = 0.0;
    al[0] = z[3]; al[1] = z[4]; al[2] = z[5]; al[3] = z[6];
}

__device__ __forceinline__ void bxf_load_state(const bxf_io_t &io, size_t r, bxf_state_t &s) {
    const double *st = io.state + r * 16;
#pragma unroll
    for (int c = 0; c < 7; ++c) s.m[c] = st[c];
    s.v[0] = st[7]; s.v[1] = st[8]; s.v[2] = st[9];
    s.P00 = st[10]; s.P01 = st[11]; s.P11 = st[12]; s.Py = st[13]; s.Ps = st[14];
}

// the link word `w` of record j as a record of the stream, or -1
__device__ __forceinline__ int bxf_link(const bxf_io_t &io, size_t rb, int j, int w, int records) {
    const int v = io.link[(rb + j) * 4 + w];
    return (v >= 0 && v < records) ? v : -1;
}

// forward: the filter along the segment that begins at member `first`
__device__ void bxf_forward(const bxf_io_t &io, const rtk_box_filter_t &par, size_t rb, int first, int records) {
    bxf_state_t s;
    double z[7];
    bxf_measurement(io.box + (rb + first) * 8, z);
    bxf_start(s, z, par);
    bxf_store_state(io, rb + first, s, z);
    io.link[(rb + first) * 4 + 3] = first;
    int j = first;
    for (int steps = 1; steps < records; ++steps) {
        const int nx = bxf_link(io, rb, j, 2, records);
        if (nx < 0) break;
        const int k = count_clamp(io.link[(rb + nx) * 4 + 1], RTK_BOX_FILTER_MAX_GAP);
        for (int i = 0; i < k; ++i) bxf_predict(s, par);
        bxf_measurement(io.box + (rb + nx) * 8, z);
        bxf_align(s, z, par);
        bxf_update(s, z, par);
        bxf_store_state(io, rb + nx, s, z);
        io.link[(rb + nx) * 4 + 3] = first;
        j = nx;
    }
}

// a member's final mean as its box and velocity rows; ext: NULL, or the segment's l, w, h
__device__ __forceinline__ void bxf_store_output(const bxf_io_t &io, size_t r, const bxf_state_t &s, const double *ext) {
    double m[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) m[c] = s.m[c];
    if (ext) { m[4] = ext[0]; m[5] = ext[1]; m[6] = ext[2]; }
    bxf_output(m, s.v, io.out_box + r * 8, io.vel + r * 4);
}

// finish: box and vel of every member of the segment that begins at `first`
__device__ void bxf_finish(const bxf_io_t &io, const rtk_box_filter_t &par, size_t rb, int first, int records, const double *ext) {
    bxf_state_t s;
    int j = first;
    if (!par.smooth) {
        for (int steps = 0; steps < records && j >= 0; ++steps) {
            bxf_load_state(io, rb + j, s);
            bxf_store_output(io, rb + j, s, ext);
            j = bxf_link(io, rb, j, 2, records);
        }
        return;
    }
    int length = 1;
    for (; length < records; ++length) {
        const int nx = bxf_link(io, rb, j, 2, records);
        if (nx < 0) break;
        j = nx;
    }
    bxf_load_state(io, rb + j, s);      // the last member: its smoothed mean is its filtered one
    bxf_store_output(io, rb + j, s, ext);
    for (int steps = 1; steps < length; ++steps) {
        const int p = bxf_link(io, rb, j, 0, records);
        if (p < 0) break;
        const int k = count_clamp(io.link[(rb + j) * 4 + 1], RTK_BOX_FILTER_MAX_GAP);
        double nm[7], nv[3];
#pragma unroll
        for (int c = 0; c < 7; ++c) nm[c] = s.m[c];
        nv[0] = s.v[0]; nv[1] = s.v[1]; nv[2] = s.v[2];
        bxf_load_state(io, rb + p, s);
        bxf_smooth(s, k, nm, nv, par);
        bxf_store_output(io, rb + p, s, ext);
        j = p;
    }
}

__global__ __launch_bounds__(BXF_THREADS) void filter_boxes_kernel(const rtk_result_log_t rl, const rtk_box_filter_t par, const bxf_io_t io) {
    __shared__ double pool[BXF_WINDOW * 3];      // links: key | last | lastn | cur, LW_SLOTS int32 each; extent: three doubles per record slot
    __shared__ int scal[2], raised;              // scal: 0 ids in the table | 1 overflow
    int *key = reinterpret_cast<int *>(pool), *last = key + LW_SLOTS, *lastn = last + LW_SLOTS, *cur = lastn + LW_SLOTS;
    const int b = blockIdx.x, t = threadIdx.x;
    rtk_score_log_t lg = {};      // the part of the scorer's log block the walk reads: the frame words are the scorer's
    lg.F = rl.F; lg.R = rl.R; lg.cursor = rl.cursor; lg.frame = rl.frame;
    const int frames = lw_frames(lg, b), records = count_clamp(rl.cursor[b * 4 + 1], rl.R);
    const size_t rb = (size_t)b * rl.R;
    for (int h = t; h < LW_SLOTS; h += BXF_THREADS) { key[h] = LW_EMPTY; last[h] = -1; lastn[h] = 0; cur[h] = BXF_NONE; }
    if (t < 2) scal[t] = 0;
    if (t == 0) raised = 0;
    __syncthreads();

    // ---- links ----
    int mine = 0;
    bool dead = false;      // a clip overflowed the track table: it and the later clips come out empty
    for (int f0 = 0; f0 < frames;) {
        int f1 = f0 + 1;
        while (f1 < frames && !lw_frame(lg, b, f1).reset) ++f1;
        if (!dead) {
            for (int f = f0; f < f1; ++f) {
                const lw_frame_t fr = lw_frame(lg, b, f);
                const int r = fr.rec + t;
                if (t < fr.P && r < records && lw_track_slot<true>(key, scal, rl.rec_track[rb + r]) < 0) scal[1] = 1;
            }
            __syncthreads();
            dead = scal[1] != 0;
        }
        if (dead) {
            for (int f = f0; f < f1; ++f) {
                const lw_frame_t fr = lw_frame(lg, b, f);
                const int r = fr.rec + t;
                if (t < fr.P && r < records) bxf_store_empty(io, rb + r);
            }
        } else {
            for (int f = f0; f < f1; ++f) {
                const lw_frame_t fr = lw_frame(lg, b, f);
                const int n = rl.tag[((size_t)b * rl.F + f) * 4 + 1];
                const int r = fr.rec + t;
                const bool rec = t < fr.P && r < records;
                int s = -1, vin = 0;
                if (rec) {
                    vin = io.valid[rb + r];
                    const int id = rl.rec_track[rb + r];
                    if (vin > 0 && (!io.keep || io.keep[rb + r]) && id != LW_EMPTY) {
                        s = lw_track_slot<false>(key, scal, id);
                        if (s >= 0) atomicMin(&cur[s], r);
                    }
                }
                __syncthreads();
                const bool member = s >= 0 && cur[s] == r;
                if (rec && !member) {
                    if (s >= 0) mine = RTK_BOX_FLAG_DUPLICATE;
                    bxf_store_empty(io, rb + r);
                } else if (member) {
                    const int prev = last[s];
                    const long long k = (long long)n - (long long)lastn[s];
                    const bool cont = prev >= 0 && k >= 1 && k <= par.max_gap;
                    io.link[(rb + r) * 4 + 0] = cont ? prev : -1;
                    io.link[(rb + r) * 4 + 1] = cont ? (int)k : -1;
                    if (prev >= 0) io.link[(rb + prev) * 4 + 2] = cont ? r : -1;
                    io.out_valid[rb + r] = vin;
                    last[s] = r;
                    lastn[s] = n;
                }
                __syncthreads();
                if (member) cur[s] = BXF_NONE;
                __syncthreads();
            }
            for (int h = t; h < LW_SLOTS; h += BXF_THREADS)
                if (last[h] >= 0) io.link[(rb + last[h]) * 4 + 2] = -1;
        }
        __syncthreads();
        for (int h = t; h < LW_SLOTS; h += BXF_THREADS) { key[h] = LW_EMPTY; last[h] = -1; lastn[h] = 0; cur[h] = BXF_NONE; }
        if (t == 0) scal[0] = 0;
        __syncthreads();
        f0 = f1;
    }
    if (mine) atomicOr(&raised, mine);

    // ---- forward, and with the filter's own sizes the finish at once (the same lane: no barrier between them) ----
    for (int r = t; r < records; r += BXF_THREADS) {
        if (io.out_valid[rb + r] > 0 && io.link[(rb + r) * 4] < 0) {
            bxf_forward(io, par, rb, r, records);
            if (!par.size_rule) bxf_finish(io, par, rb, r, records, nullptr);
        }
    }
    __syncthreads();

    // ---- extent and finish, a window of first members at a time ----
    if (par.size_rule) {
        for (int base = 0; base < records; base += BXF_WINDOW) {
            for (int r = t; r < records; r += BXF_THREADS) {
                if (io.out_valid[rb + r] <= 0) continue;
                const int first = bxf_link(io, rb, r, 3, records);
                if (first < base || first >= base + BXF_WINDOW) continue;
                const double *al = io.aligned + (rb + r) * 4;
                const double me[3] = {al[1], al[2], al[3]};
                int below[3] = {0, 0, 0}, n = 0;
                for (int j = first; j >= 0 && n < records; j = bxf_link(io, rb, j, 2, records), ++n) {
                    const double *o = io.aligned + (rb + j) * 4;
#pragma unroll
                    for (int c = 0; c < 3; ++c) below[c] += (o[1 + c] < me[c] || (o[1 + c] == me[c] && j < r)) ? 1 : 0;
                }
                const int q = (int)(((long long)par.size_percent * (long long)(n - 1)) / 100);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (below[c] == q) pool[(first - base) * 3 + c] = me[c];
            }
            __syncthreads();
            const int end = records - base < BXF_WINDOW ? records : base + BXF_WINDOW;
            for (int r = base + t; r < end; r += BXF_THREADS)
                if (io.out_valid[rb + r] > 0 && io.link[(rb + r) * 4] < 0) bxf_finish(io, par, rb, r, records, pool + (r - base) * 3);
            __syncthreads();
        }
    }
    if (t == 0) io.flags[b] = raised | (dead ? RTK_BOX_FLAG_TRACKS : 0);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_result_log_filter_boxes(int B, const rtk_result_log_t *lg, const unsigned char *keep, const double *box, const int *valid,
                                           const rtk_box_filter_t *par, double *out_box, int *out_valid, double *vel, double *state,
                                           double *aligned, int *link, int *flags, rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535, "result_log_filter_boxes: B=%d streams", B);
    RTK_REQUIRE(lg && lg->F >= 1 && lg->R >= 1 && lg->cursor && lg->frame && lg->tag && lg->rec_track, "result_log_filter_boxes: null or empty log");
    RTK_REQUIRE((long long)B * 4 * lg->F < (1ll << 31) && (long long)B * 16 * lg->R < (1ll << 31),
                "result_log_filter_boxes: a log of B=%d x (F=%d, R=%d): a table of 2^31 words or more", B, lg->F, lg->R);
    if (const int e = bxf_check_ranges("result_log_filter_boxes", par)) return e;
    RTK_REQUIRE(box && valid, "result_log_filter_boxes: null input boxes");
    RTK_REQUIRE(out_box && out_valid && vel && state && aligned && link && flags, "result_log_filter_boxes: null output");
    RTK_REQUIRE(out_box != box && out_valid != valid, "result_log_filter_boxes: the outputs must not alias the input boxes");
    bxf_io_t io;
    io.keep = keep; io.box = box; io.valid = valid; io.out_box = out_box; io.out_valid = out_valid; io.vel = vel; io.state = state;
    io.aligned = aligned; io.link = link; io.flags = flags;
    filter_boxes_kernel<<<B, BXF_THREADS, 0, (hipStream_t)stream>>>(*lg, *par, io);
    RTK_CHECK_LAUNCH("result_log_filter_boxes");
    return RTK_OK;
}
