// track_assign.hip -- the batched tracker's association with the decision made by an exact assignment (include/rtk_fused.h,
// rtk_associate_optimal; ratrack_amd/tracker.py, BatchedTracker(assign="optimal")).
//
//   rtk_associate_optimal   one wave per stream, in place of rtk_associate_batched: the live (m_b, n_b) block of aff is gated and
//                           quantised into integer weights in LDS, la_solve_dense (lds_assignment.h) finds the maximum-weight
//                           one-to-one matching of previous rows and current objects, and the tail writes what
//                           rtk_associate_batched's tail writes: track IDs, confidences, indices1, the next ids / count,
//                           point_track_id
//
// No Sinkhorn, no floating point after the quantisation.  The kernel is latency bound like every one-workgroup-per-stream kernel of
// the tracker: one wave walks the solver's search rounds, each a pass over its columns of the block (conflict-free: consecutive
// lanes read consecutive words) and one wave reduction.  The ID bookkeeping is restated here for one wave because
// associate_batched_kernel (track_batched.hip) is pinned as it is.
#include <math.h>

#include "batch_common.h"
#include "lds_assignment.h"
#include "rtk_common.h"
#include "rtk_fused.h"

#define TA_LDS_LIMIT (160 * 1024)      // one workgroup's LDS (ASSOC_LDS_LIMIT of track_batched.hip)
#define TA_WEIGHT_ONE 268435456.0f     // 2^28: an affinity of 1, the largest weight -- below la_solve_dense's 2^29

// LDS, in ints: the weight block [K * K], row stride K | the solver's tables at K x K | sid [K], the new IDs
constexpr int ta_words(int K) { return K * K + la_dense_words(K, K) + K; }
// K = 197 is what rtk_track_max_objects() admits: 155 236 B of weights + 788 B (u) + 3 940 B (five tables) = 159 964 B, + 788 B (sid)
static_assert((197 * 197 + 197 + 5 * 197) * sizeof(int) == 159964 && ta_words(197) * sizeof(int) == 160752 &&
              ta_words(197) * sizeof(int) <= TA_LDS_LIMIT, "the association at the largest K fits one workgroup's LDS");

struct AssignArgs {
    int N, K;
    const unsigned char *active, *reset;
    const float *aff;
    const int *num_objects, *obj, *prev_ids, *prev_count;
    double min_affinity;
    int *counter, *ids, *count, *object_ids;
    float *object_conf;
    int *indices1, *num_prev, *point_track_id;
    long long *total;
};

__global__ __launch_bounds__(RTK_WAVE) void associate_optimal_kernel(const AssignArgs a) {
    extern __shared__ __attribute__((aligned(16))) int ta_smem[];
    const int b = blockIdx.x, t = threadIdx.x, K = a.K, N = a.N;
    const int *prev_ids = a.prev_ids + (size_t)b * K;
    int *object_ids = a.object_ids + (size_t)b * K, *indices1 = a.indices1 + (size_t)b * K;
    float *object_conf = a.object_conf + (size_t)b * K;
    const float *__restrict__ aff = a.aff + (size_t)b * K * K;
    const int mp = count_clamp(a.prev_count[b], K);
    if (a.active && !a.active[b]) {       // state carried over, nothing reported
        for (int e = t; e < K; e += RTK_WAVE) {
            a.ids[(size_t)b * K + e] = prev_ids[e];
            object_ids[e] = -1; object_conf[e] = 0.f; indices1[e] = -1;
        }
        for (int p = t; p < N; p += RTK_WAVE) a.point_track_id[(size_t)b * N + p] = -1;
        if (t == 0) { a.count[b] = mp; a.num_prev[b] = 0; }
        return;
    }
    const int m = (a.reset && a.reset[b]) ? 0 : mp;
    const int n = count_clamp(a.num_objects[b], K);
    int *w = ta_smem, *work = w + K * K, *sid = work + la_dense_words(K, K);
    const int *cp = work + la_dense_cp_offset(m, n);
    const bool assoc = m > 0 && n > 0;
    long long total = 0;
    if (assoc) {
        // ---- the gate and the quantisation: the live block only, pair by pair in row-major order ----
        const double gate = a.min_affinity;
#pragma unroll 4
        for (int e = t; e < m * n; e += RTK_WAVE) {
            const int i = e / n, j = e - i * n;
            const float x = aff[(size_t)i * K + j];
            w[i * K + j] = (double)x >= gate ? (int)(fminf(x, 1.f) * TA_WEIGHT_ONE) : 0;      // a NaN fails the comparison
        }
        __syncthreads();
        total = la_solve_dense(m, n, w, K, work);
        __syncthreads();
    }
    // ---- track IDs: an unmatched object takes a fresh ID from the counter, in current-object order ----
    const int next = a.counter[b];
    int nfresh_total = 0;
    for (int j0 = 0; j0 < n; j0 += RTK_WAVE) {
        const int j = j0 + t;
        int k = -1;
        float conf = 0.f;
        if (j < n && assoc) {
            k = cp[j];
            if (k >= 0) conf = aff[(size_t)k * K + j];
        }
        const bool fresh = j < n && k < 0;
        const unsigned long long vote = __ballot(fresh);
        const int slot = __popcll(vote & ((1ull << t) - 1ull));
        if (j < n) {
            const int id = fresh ? next + nfresh_total + slot : prev_ids[k];
            sid[j] = id;
            object_ids[j] = id;
            object_conf[j] = conf;
            indices1[j] = k;
        }
        nfresh_total += __popcll(vote);
    }
    for (int j = n + t; j < K; j += RTK_WAVE) { object_ids[j] = -1; object_conf[j] = 0.f; indices1[j] = -1; }
    __syncthreads();
    if (t == 0) {
        a.counter[b] = next + nfresh_total; a.count[b] = n; a.num_prev[b] = m;
        if (a.total) a.total[b] = total;
    }
    for (int j = t; j < n; j += RTK_WAVE) a.ids[(size_t)b * K + j] = sid[j];
    const int *obj_b = a.obj + (size_t)b * N;
    for (int p = t; p < N; p += RTK_WAVE) {
        const int o = obj_b[p];
        a.point_track_id[(size_t)b * N + p] = (o >= 0 && o < n) ? sid[o] : -1;
    }
}

extern "C" int rtk_associate_optimal_lds_bytes(int K) {
    if (K < 1 || K > 4096) return -1;
    return (int)(ta_words(K) * sizeof(int));
}

extern "C" int rtk_associate_optimal(int B, int N, int K, const unsigned char *active, const unsigned char *reset, const float *aff,
                                     const int *num_objects, const int *obj, const int *prev_ids, const int *prev_count,
                                     double min_affinity, int *counter, int *ids, int *count, int *object_ids, float *object_conf,
                                     int *indices1, int *num_prev, int *point_track_id, long long *total, rtk_stream_t stream) {
    RTK_REQUIRE(B > 0 && B <= 65535 && N > 0 && aff && num_objects && obj && prev_ids && prev_count && counter && ids && count &&
                object_ids && object_conf && indices1 && num_prev && point_track_id, "associate_optimal: bad arguments");
    RTK_REQUIRE(K >= 1 && K <= rtk_track_max_objects(), "associate_optimal: K=%d object slots outside [1, %d] (the per-stream association "
                "table must fit one workgroup's LDS)", K, rtk_track_max_objects());
    RTK_REQUIRE(min_affinity >= 0.01 && min_affinity <= 1.0, "associate_optimal: min_affinity=%g outside [0.01, 1] (0.01 is the "
                "reference's confidence threshold; an affinity is a sigmoid)", min_affinity);
    const int lds = rtk_associate_optimal_lds_bytes(K);
    RTK_REQUIRE(lds > 0 && lds <= TA_LDS_LIMIT, "associate_optimal: K=%d needs %d bytes of LDS per stream, the limit is %d", K, lds,
                TA_LDS_LIMIT);
    const AssignArgs a = {N, K, active, reset, aff, num_objects, obj, prev_ids, prev_count, min_affinity, counter, ids, count,
                          object_ids, object_conf, indices1, num_prev, point_track_id, total};
    (void)hipFuncSetAttribute((const void *)associate_optimal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    associate_optimal_kernel<<<B, RTK_WAVE, (size_t)lds, (hipStream_t)stream>>>(a);
    RTK_CHECK_LAUNCH("associate_optimal");
    return RTK_OK;
}
