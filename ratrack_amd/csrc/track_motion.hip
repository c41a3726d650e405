// track_motion.hip -- rtk_track_memory_motion (include/rtk_fused.h): the state advance of rtk_track_memory (track_batched.hip) for a
// tracker whose coasted tracks move: every row of the table carries a velocity (the object's displacement per frame, from the mean
// predicted scene flow in its descriptor), and a row that survives unmatched has its centre advanced by it.  The lifecycle rules
// (ids, age, hits, n_det, count, flags, object_hits, object_gap, num_coasted) are rtk_track_memory's, word for word; that kernel is
// the default and is not touched.
//
// One workgroup per stream, thread t = row t of the tables (K <= 256), as there.  A current row's velocity is written by the thread
// of its own index, a survivor's by the thread of its SOURCE row (to the row it lands in), a row past the count by the thread of its
// own index: three disjoint row ranges, plain stores, no atomics -- every run gives the same bits.
#include "assoc_common.h"
#include "batch_common.h"
#include "rtk_common.h"
#include "rtk_fused.h"

#define MOTION_FLOW 134          // channels 134..136 of a descriptor: the object's mean predicted scene flow

struct MotionArgs {
    int K, max_age;
    float beta;
    const unsigned char *active, *reset;
    const int *num_objects, *indices1;
    const float *object_conf;
    const int *prev_ids, *prev_age, *prev_hits, *prev_n_det, *prev_count;
    const float *desc_prev, *prev_vel;
    int *ids, *age, *hits, *n_det, *count;
    float *desc, *vel;
    int *flags, *object_hits, *object_gap, *num_coasted;
    float *object_velocity;
};

__global__ __launch_bounds__(256) void track_motion_kernel(const MotionArgs a) {
#pragma clang fp contract(off)            // v + beta (f - v) is three roundings, the centre + velocity one: never an FMA
    __shared__ int s_wave[4], s_matched[256], s_src[256];
    const int b = blockIdx.x, t = threadIdx.x, K = a.K;
    const size_t row0 = (size_t)b * K;
    const int *prev_ids = a.prev_ids + row0, *prev_age = a.prev_age + row0, *prev_hits = a.prev_hits + row0;
    int *ids = a.ids + row0, *age = a.age + row0, *hits = a.hits + row0;
    int *object_hits = a.object_hits + row0, *object_gap = a.object_gap + row0;
    const float *prev_vel = a.prev_vel + row0 * 3;
    float *vel = a.vel + row0 * 3, *object_velocity = a.object_velocity + row0 * 3;
    const int mp = count_clamp(a.prev_count[b], K);
    if (a.active && !a.active[b]) {       // no frame passed: the table, its velocities included, stays what it was; no centre moves
        if (t < K) {
            age[t] = prev_age[t]; hits[t] = prev_hits[t]; object_hits[t] = 0; object_gap[t] = -1;
            for (int c = 0; c < 3; ++c) { vel[t * 3 + c] = prev_vel[t * 3 + c]; object_velocity[t * 3 + c] = 0.f; }
        }
        if (t == 0) {
            const int nd = a.prev_n_det[b];
            a.n_det[b] = nd;
            a.num_coasted[b] = mp - count_clamp(nd, mp);
        }
        return;
    }
    const int m = (a.reset && a.reset[b]) ? 0 : mp;
    const int n = count_clamp(a.num_objects[b], K);
    s_matched[t] = 0;
    __syncthreads();
    int from = -1;                         // the previous row whose ID current object t inherited
    if (t < n) {
        const int i = a.indices1[row0 + t];
        if (i >= 0 && i < m && a.object_conf[row0 + t] != 0.f) { from = i; s_matched[i] = 1; }
    }
    __syncthreads();
    if (t < n) {
        const int h = from >= 0 ? prev_hits[from] + 1 : 1;
        age[t] = 0; hits[t] = h;
        object_hits[t] = h; object_gap[t] = from >= 0 ? prev_age[from] : -1;
        // the measured flow of this frame (rtk_object_descriptors wrote the row), smoothed into the track's velocity
        const float *f = a.desc + (row0 + t) * RTK_DESC + MOTION_FLOW;
        for (int c = 0; c < 3; ++c) {
            float w = f[c];
            if (from >= 0 && a.beta != 1.f) {
                const float v = prev_vel[from * 3 + c];
                const float d = w - v;
                const float s = a.beta * d;
                w = v + s;
            }
            vel[t * 3 + c] = w; object_velocity[t * 3 + c] = w;
        }
    } else if (t < K) {
        object_hits[t] = 0; object_gap[t] = -1;
        for (int c = 0; c < 3; ++c) object_velocity[t * 3 + c] = 0.f;
    }
    const int pa = t < m ? prev_age[t] : 0;
    const bool survives = t < m && !s_matched[t] && pa < a.max_age;       // age + 1 <= max_age
    int S;
    const int slot = ordered_slot(survives, s_wave, &S);
    const int cnt = n + S < K ? n + S : K;
    if (survives && n + slot < K) {
        const int r = n + slot;
        ids[r] = prev_ids[t]; age[r] = pa + 1; hits[r] = prev_hits[t];
        for (int c = 0; c < 3; ++c) vel[r * 3 + c] = prev_vel[t * 3 + c];
        s_src[slot] = t;
    }
    if (t >= cnt && t < K) {
        ids[t] = -1; age[t] = 0; hits[t] = 0;
        for (int c = 0; c < 3; ++c) vel[t * 3 + c] = 0.f;
    }
    if (t == 0) {
        a.count[b] = cnt; a.n_det[b] = n; a.num_coasted[b] = cnt - n;
        if (n + S > K) a.flags[b] |= 4;
    }
    __syncthreads();
    // the survivors' descriptor rows, element by element: the centre (channels 0..2) moves one frame, the rest is copied as words
    const unsigned *src = reinterpret_cast<const unsigned *>(a.desc_prev) + row0 * RTK_DESC;
    unsigned *dst = reinterpret_cast<unsigned *>(a.desc) + (row0 + n) * RTK_DESC;
    for (int e = t; e < (cnt - n) * RTK_DESC; e += 256) {
        const int i = s_src[e / RTK_DESC], c = e % RTK_DESC;
        unsigned w = src[(size_t)i * RTK_DESC + c];
        if (c < 3) w = __float_as_uint(__uint_as_float(w) + prev_vel[i * 3 + c]);
        dst[e] = w;
    }
}

extern "C" int rtk_track_memory_motion(int B, int K, int max_age, float beta, const unsigned char *active, const unsigned char *reset,
                                       const int *num_objects, const int *indices1, const float *object_conf, const int *prev_ids,
                                       const int *prev_age, const int *prev_hits, const int *prev_n_det, const int *prev_count,
                                       const float *desc_prev, const float *prev_vel, int *ids, int *age, int *hits, int *n_det,
                                       int *count, float *desc, float *vel, int *flags, int *object_hits, int *object_gap,
                                       int *num_coasted, float *object_velocity, rtk_stream_t stream) {
    RTK_REQUIRE(B > 0 && B <= 65535 && num_objects && indices1 && object_conf && prev_ids && prev_age && prev_hits && prev_n_det &&
                prev_count && desc_prev && prev_vel && ids && age && hits && n_det && count && desc && vel && flags && object_hits &&
                object_gap && num_coasted && object_velocity, "track_memory_motion: bad arguments");
    RTK_REQUIRE(K >= 1 && K <= rtk_track_max_objects(), "track_memory_motion: K=%d object slots outside [1, %d] (the per-stream "
                "association table must fit one workgroup's LDS)", K, rtk_track_max_objects());
    RTK_REQUIRE(max_age >= 0, "track_memory_motion: max_age=%d is negative", max_age);
    RTK_REQUIRE(beta > 0.f && beta <= 1.f, "track_memory_motion: beta=%g outside (0, 1]", (double)beta);      // (a NaN fails both)
    RTK_REQUIRE(ids != prev_ids && age != prev_age && hits != prev_hits && desc != desc_prev && vel != prev_vel,
                "track_memory_motion: the new table must not alias the previous one");
    const MotionArgs a = {K, max_age, beta, active, reset, num_objects, indices1, object_conf, prev_ids, prev_age, prev_hits, prev_n_det,
                          prev_count, desc_prev, prev_vel, ids, age, hits, n_det, count, desc, vel, flags, object_hits, object_gap,
                          num_coasted, object_velocity};
    track_motion_kernel<<<B, 256, 0, (hipStream_t)stream>>>(a);
    RTK_CHECK_LAUNCH("track_memory_motion");
    return RTK_OK;
}
