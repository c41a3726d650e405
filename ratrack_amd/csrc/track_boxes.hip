// track_boxes.hip -- oriented boxes for tracked objects (include/rtk_fused.h, "Oriented boxes"; ratrack_amd/boxes.py).
//
//   rtk_result_log_boxes   one workgroup per stream: the box of every record below the stream's cursors (of the records `keep` marks)
//   rtk_object_boxes       one workgroup per stream: the box of every object of a live step
//
// The rule is box_fit.h's and is stated nowhere else; this file holds the two walks.  In both a workgroup's four waves work on their
// own: a wave takes whole frames of the log (records of one frame follow one another in the points table, so their offsets are a
// running sum the wave keeps itself) or whole objects of the step, stages one object's BEV coordinates in its 2 KiB of LDS and calls
// bf_fit_wave.  Every output word has one writer and plain stores; the one word waves share is the stream's flags word, gathered with
// an integer OR in LDS and stored by thread 0.
#include "box_fit.h"
#include "score_log_walk.h"

#define TB_THREADS 256
#define TB_WAVES (TB_THREADS / RTK_WAVE)
static_assert(RTK_BOX_MAX_POINTS <= 256, "bf_fit_wave packs a pair's two point indices into eight bits each");

// ------------------------------------------------------------------------------------------------
// rtk_result_log_boxes
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB_THREADS) void log_boxes_kernel(const rtk_result_log_t rl, const unsigned char *keep, double min_extent, double *box,
                                                               int *cand, int *valid, int *flags) {
    __shared__ double2 xy[TB_WAVES][RTK_BOX_MAX_POINTS];
    __shared__ int raised;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1), wave = t / RTK_WAVE;
    rtk_score_log_t lg = {};      // the part of the scorer's log block the walk reads: the frame words are the scorer's
    lg.F = rl.F; lg.R = rl.R; lg.cursor = rl.cursor; lg.frame = rl.frame;
    if (t == 0) raised = 0;
    __syncthreads();
    const int frames = lw_frames(lg, b);
    const int records = count_clamp(rl.cursor[b * 4 + 1], rl.R), points = count_clamp(rl.cursor[b * 4 + 2], rl.P);
    const size_t rb = (size_t)b * rl.R;
    const float *pts = rl.points + (size_t)b * rl.P * 3;
    int mine = 0;
    for (int f = wave; f < frames; f += TB_WAVES) {
        const lw_frame_t fr = lw_frame(lg, b, f);
        int at = count_clamp(rl.frame[((size_t)b * rl.F + f) * 4 + 1], points);      // the frame's first point
        for (int i0 = 0; i0 < fr.P; i0 += RTK_WAVE) {
            // lane i: the size of record i0 + i and whether it is fitted; then record after record, the whole wave on each
            const int r_lane = fr.rec + i0 + lane;
            int size_lane = 0, keep_lane = 0;
            if (i0 + lane < fr.P && r_lane < records) {
                size_lane = count_clamp(rl.rec_size[rb + r_lane], points);
                keep_lane = keep ? (keep[rb + r_lane] != 0) : 1;
            }
            const int count = fr.P - i0 < RTK_WAVE ? fr.P - i0 : RTK_WAVE;
            for (int u = 0; u < count; ++u) {
                const int r = fr.rec + i0 + u;
                if (r >= records) break;
                int n = __builtin_amdgcn_readfirstlane(__shfl(size_lane, u));
                const int fit = __builtin_amdgcn_readfirstlane(__shfl(keep_lane, u));
                if (n > points - at) n = points - at;
                double *bx = box + (rb + r) * 8;
                if (!fit) {
                    bf_store_empty(bx, cand + rb + r, valid + rb + r, 0, lane);
                } else {
                    bf_range_t rg;
                    bf_range_init(rg);
                    for (int k = lane; k < n; k += RTK_WAVE) {
                        const float *p = pts + (size_t)(at + k) * 3;
                        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
                        bf_range_add(rg, x, y, z);
                        if (n <= RTK_BOX_MAX_POINTS) xy[wave][k] = make_double2(x, y);
                    }
                    if (bf_fit_wave(xy[wave], n, rg, min_extent, bx, cand + rb + r, valid + rb + r, lane)) mine = RTK_BOX_FLAG_AXIS;
                }
                at += n;
            }
        }
    }
    if (mine && lane == 0) atomicOr(&raised, mine);
    __syncthreads();
    if (t == 0) flags[b] = raised;
}

// ------------------------------------------------------------------------------------------------
// rtk_object_boxes
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB_THREADS) void object_boxes_kernel(int N, int K, const rtk_bcn_view_t pc1, const int *obj, const int *num_objects,
                                                                  const unsigned char *active, double min_extent, double *box, int *cand,
                                                                  int *valid, int *flags) {
    __shared__ double2 xy[TB_WAVES][RTK_BOX_MAX_POINTS];
    __shared__ int raised;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1), wave = t / RTK_WAVE;
    int num = num_objects[b], refused = 0;
    if (active && !active[b]) {
        num = 0;
    } else if (num < 0 || num > K) {      // rtk_result_log_append's refusal: nothing of the stream is fitted
        refused = RTK_BOX_FLAG_OBJECTS;
        num = 0;
    }
    if (t == 0) raised = refused;
    __syncthreads();
    const int *ob = obj + (size_t)b * N;
    int mine = 0;
    for (int j = wave; j < K; j += TB_WAVES) {
        const size_t o = (size_t)b * K + j;
        if (j >= num) {
            bf_store_empty(box + o * 8, cand + o, valid + o, 0, lane);
            continue;
        }
        // the columns of object j in increasing p: a chunk's members are ranked by the ballot's bits below each lane
        bf_range_t rg;
        bf_range_init(rg);
        int n = 0;
        for (int p0 = 0; p0 < N; p0 += RTK_WAVE) {
            const int p = p0 + lane;
            const bool member = p < N && ob[p] == j;
            const unsigned long long mask = __ballot(member);
            if (member) {
                const double x = (double)bcn_at(pc1, b, 0, p), y = (double)bcn_at(pc1, b, 1, p), z = (double)bcn_at(pc1, b, 2, p);
                bf_range_add(rg, x, y, z);
                const int k = n + __popcll(mask & ((1ull << lane) - 1ull));
                if (k < RTK_BOX_MAX_POINTS) xy[wave][k] = make_double2(x, y);
            }
            n += __popcll(mask);
        }
        if (bf_fit_wave(xy[wave], n, rg, min_extent, box + o * 8, cand + o, valid + o, lane)) mine = RTK_BOX_FLAG_AXIS;
    }
    if (mine && lane == 0) atomicOr(&raised, mine);
    __syncthreads();
    if (t == 0) flags[b] = raised;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool tb_extent_ok(double min_extent) { return isfinite(min_extent) && min_extent >= 0.0; }

extern "C" int rtk_result_log_boxes(int B, const rtk_result_log_t *lg, const unsigned char *keep, double min_extent, double *box, int *cand,
                                    int *valid, int *flags, rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535, "result_log_boxes: B=%d streams", B);
    RTK_REQUIRE(lg && lg->F >= 1 && lg->R >= 1 && lg->P >= 1 && lg->cursor && lg->frame && lg->rec_size && lg->points,
                "result_log_boxes: null or empty log");
    RTK_REQUIRE((long long)B * 4 * lg->F < (1ll << 31) && (long long)B * 8 * lg->R < (1ll << 31) && (long long)B * 3 * lg->P < (1ll << 31),
                "result_log_boxes: a log of B=%d x (F=%d, R=%d, P=%d): a table of 2^31 words or more", B, lg->F, lg->R, lg->P);
    RTK_REQUIRE(tb_extent_ok(min_extent), "result_log_boxes: min_extent=%g is not a finite number >= 0", min_extent);
    RTK_REQUIRE(box && cand && valid && flags, "result_log_boxes: null output");
    log_boxes_kernel<<<B, TB_THREADS, 0, (hipStream_t)stream>>>(*lg, keep, min_extent, box, cand, valid, flags);
    RTK_CHECK_LAUNCH("result_log_boxes");
    return RTK_OK;
}

extern "C" int rtk_object_boxes(int B, int N, int K, const rtk_bcn_view_t *pc1, const int *obj, const int *num_objects,
                                const unsigned char *active, double min_extent, double *box, int *cand, int *valid, int *flags,
                                rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && K >= 1 && K <= RTK_RESULT_MAX_OBJECTS, "object_boxes: bad sizes B=%d N=%d K=%d (K <= %d)", B, N, K,
                RTK_RESULT_MAX_OBJECTS);
    RTK_REQUIRE((long long)B * N < (1ll << 31) - RTK_WAVE, "object_boxes: B=%d streams of N=%d columns: 2^31 or more", B, N);
    RTK_REQUIRE(pc1 && pc1->ptr && obj && num_objects, "object_boxes: null argument");
    RTK_REQUIRE(tb_extent_ok(min_extent), "object_boxes: min_extent=%g is not a finite number >= 0", min_extent);
    RTK_REQUIRE(box && cand && valid && flags, "object_boxes: null output");
    object_boxes_kernel<<<B, TB_THREADS, 0, (hipStream_t)stream>>>(N, K, *pc1, obj, num_objects, active, min_extent, box, cand, valid, flags);
    RTK_CHECK_LAUNCH("object_boxes");
    return RTK_OK;
}
