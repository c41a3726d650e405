// track_batched.hip -- the post-backbone half of Track4D.forward (detection + association, models/track4d.py:53-65,108-223) for B
// independent streams at once: four launches per frame whatever B is, no host round trip (ratrack_amd/tracker.py); a fifth when
// the tracker keeps lost tracks (max_age).
//
//   rtk_dbscan_batched      one workgroup per stream: mover selection + DBSCAN (dbscan_workgroup, rtk_dbscan's) + the objects'
//                           reference order (by first member point)
//   rtk_object_descriptors  (stream, object-slot) workgroups: the 141-d descriptor of every object
//   rtk_affinity_pairs      (stream, pair-tile) workgroups: the Affinity MLP on the live m_b x n_b descriptor differences
//   rtk_associate_batched   one workgroup per stream: log-Sinkhorn (log_ot_lds, rtk_log_sinkhorn's), mutual best match,
//                           track IDs, point_track_id
//   rtk_track_memory        one workgroup per stream: the next table = this frame's detections + the unmatched previous rows that
//                           are still young enough, compacted in table order
//
// The DBSCAN and log-OT code lives in assoc_common.h, shared with the B = 1 kernels of fused_misc.hip.
//
// Every stream's counts (n_valid, movers, objects, previous objects) stay on the device; the tables are sized for N points / K
// object slots and only the live part is touched.
#include <math.h>

#include "assoc_common.h"
#include "batch_common.h"
#include "rtk_common.h"
#include "rtk_fused.h"

#define DB_LDS_BYTES (128 * 1024)

// ------------------------------------------------------------------------------------------------
// rtk_dbscan_batched: dbscan_workgroup (assoc_common.h) on one stream's columns, then step 5 numbers the objects as the reference's
// dict does (models/track4d.py:119-125: in order of their FIRST MEMBER point, border points included -- the numpy block of
// association.cluster_objects_device).  Tables (n points of the stream): f (n,8) | src | lab | aux | cl, 48 B per point.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dbscan_stream(const rtk_track_frame_t &fr, int b, int n, float thr, double eps, int min_samples,
                                              int K, float *f, int *labels_b, int *obj_b, int *num_objects, int *flags) {
    int *src = reinterpret_cast<int *>(f + (size_t)n * DB_D), *lab = src + n, *aux = lab + n;
    int *cl = aux + n;                                             // cluster id of each mover
    const int t = threadIdx.x;
    const auto [m, C] = dbscan_workgroup(n, f, src, lab, aux, eps, min_samples,
        [&](int i) { return bcn_at(fr.cls, b, 0, i) > thr; },
        [&](int i, float *fk) {
            fk[0] = bcn_at(fr.pc1, b, 0, i); fk[1] = bcn_at(fr.pc1, b, 1, i); fk[2] = bcn_at(fr.pc1, b, 2, i);
            fk[3] = bcn_at(fr.flow, b, 0, i); fk[4] = bcn_at(fr.flow, b, 1, i); fk[5] = bcn_at(fr.flow, b, 2, i);
            fk[6] = bcn_at(fr.feature1, b, 1, i);                  // v_r
            fk[7] = bcn_at(fr.prop, b, 0, i);
        },
        [&](int k, int s, int c) { cl[k] = c; labels_b[s] = c; });
    __syncthreads();
    // ---- 5. reference order: clusters ranked by their first member (movers are in column order: the smallest mover index) ----
    // C <= m: lab and aux are free again and hold C entries
    for (int c = t; c < C; c += 256) lab[c] = 0x7fffffff;
    __syncthreads();
    for (int i = t; i < m; i += 256)
        if (cl[i] >= 0) atomicMin(&lab[cl[i]], i);
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        const int first = lab[c];
        int r = 0;
        for (int d = 0; d < C; ++d) r += lab[d] < first ? 1 : 0;       // first members are distinct
        aux[c] = r;
    }
    __syncthreads();
    for (int i = t; i < m; i += 256) {
        const int k = cl[i] >= 0 ? aux[cl[i]] : -1;
        obj_b[src[i]] = k < K ? k : -1;      // objects beyond the K slots are not reported (flagged below)
    }
    if (t == 0) {
        num_objects[b] = C < K ? C : K;
        if (C > K) flags[b] |= 1;
    }
}

__global__ __launch_bounds__(256) void dbscan_batched_kernel(const rtk_track_frame_t fr, float thr, double eps, int min_samples, int K,
                                                             int lds_points, int *__restrict__ labels, int *__restrict__ obj,
                                                             int *__restrict__ num_objects, int *__restrict__ flags,
                                                             unsigned char *__restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tb_smem[];
    const int b = blockIdx.x, t = threadIdx.x, N = fr.N;
    int *labels_b = labels + (size_t)b * N, *obj_b = obj + (size_t)b * N;
    for (int i = t; i < N; i += 256) { labels_b[i] = -1; obj_b[i] = -1; }
    if (t == 0) {
        num_objects[b] = 0;
        flags[b] = (fr.n_valid && (fr.n_valid[b] < 0 || fr.n_valid[b] > N)) ? 2 : 0;
    }
    if (!stream_active(fr, b)) return;
    __syncthreads();
    const int n = stream_points(fr, b);
    if (n <= lds_points)
        dbscan_stream(fr, b, n, thr, eps, min_samples, K, reinterpret_cast<float *>(tb_smem), labels_b, obj_b, num_objects, flags);
    else      // this stream's tables exceed the LDS: its slice of the caller's workspace
        dbscan_stream(fr, b, n, thr, eps, min_samples, K,
                      reinterpret_cast<float *>(work + (size_t)b * N * RTK_DBSCAN_POINT_BYTES), labels_b, obj_b, num_objects, flags);
}

static int frame_ok(const rtk_track_frame_t *fr) {
    if (!fr || fr->B <= 0 || fr->N <= 0 || fr->B > 65535) return 0;
    const rtk_bcn_view_t *v[5] = {&fr->pc1, &fr->flow, &fr->feature1, &fr->prop, &fr->cls};
    for (int i = 0; i < 5; ++i)
        if (!v[i]->ptr) return 0;
    return 1;
}

static size_t assoc_lds_bytes(int K) {
    // Sinkhorn table (K+1) x ((K+1)|1), u, v; then max0 (K floats) and ind0, ind1, dec, sid (K ints each)
    return ((size_t)(K + 1) * ((K + 1) | 1) + 2 * (size_t)(K + 1) + 5 * (size_t)K) * sizeof(float);
}

#define ASSOC_LDS_LIMIT (160 * 1024)

extern "C" int rtk_track_max_objects(void) {
    int K = 1;
    while (K < 256 && assoc_lds_bytes(K + 1) + 64 <= ASSOC_LDS_LIMIT) ++K;      // (+ the kernel's static LDS)
    return K;
}

#define TRACK_REQUIRE_K(K, what) \
    RTK_REQUIRE((K) >= 1 && (K) <= rtk_track_max_objects(), what ": K=%d object slots outside [1, %d] (the per-stream association table " \
                "must fit one workgroup's LDS)", (K), rtk_track_max_objects())

extern "C" int rtk_dbscan_batched(const rtk_track_frame_t *frame, float threshold, double eps, int min_samples, int K, int *labels,
                                  int *obj, int *num_objects, int *flags, void *work, long long work_bytes, rtk_stream_t stream) {
    RTK_REQUIRE(frame_ok(frame) && labels && obj && num_objects && flags && min_samples >= 1, "dbscan_batched: bad arguments");
    TRACK_REQUIRE_K(K, "dbscan_batched");
    const int B = frame->B, N = frame->N;
    RTK_REQUIRE(N <= 65536, "dbscan_batched: N=%d > 65536 points (one workgroup tests all pairs of a stream)", N);
    const size_t per_stream = (size_t)N * RTK_DBSCAN_POINT_BYTES;
    const int lds_points = per_stream <= DB_LDS_BYTES ? N : DB_LDS_BYTES / RTK_DBSCAN_POINT_BYTES;
    if (lds_points < N)
        RTK_REQUIRE(work && work_bytes >= (long long)(per_stream * B), "dbscan_batched: N=%d needs a %zu-byte workspace (got %lld)", N,
                    per_stream * B, work ? work_bytes : 0ll);
    (void)hipFuncSetAttribute((const void *)dbscan_batched_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DB_LDS_BYTES);
    dbscan_batched_kernel<<<B, 256, (size_t)lds_points * RTK_DBSCAN_POINT_BYTES, (hipStream_t)stream>>>(
        *frame, threshold, eps, min_samples, K, lds_points, labels, obj, num_objects, flags, (unsigned char *)work);
    RTK_CHECK_LAUNCH("dbscan_batched");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_object_descriptors: workgroup (b, y) handles the objects y, y + G, ... of stream b.  Per chunk of 256 columns the object's
// members are compacted in column order into LDS; threads 0..127 keep the max of one prop channel, threads 128..135 the sum of one
// of the 8 statistics channels (xyz, flow, RCS, v_r); a second pass sums the squared deviations from the mean (torch.var's
// two-pass population variance).  Both sums are compensated (comp_add): a plain fp32 running sum over an object of several hundred
// points loses log2(n) bits, which the second pass squares when the object is far from the origin (80 m away, 1e-2 m across: a
// variance 5e-5 off) -- the sums then are as good as the reference's pairwise ones whatever the object's size.
// ------------------------------------------------------------------------------------------------
#define DESC_G 16

// acc += x with the rounding error of the addition carried in comp (Kahan); the build has contraction and fast-math off
__device__ __forceinline__ void comp_add(float &acc, float &comp, float x) {
    const float y = x - comp, t = acc + y;
    comp = (t - acc) - y;
    acc = t;
}

__device__ __forceinline__ float stat_channel(const rtk_track_frame_t &fr, int b, int s, int p) {
    return s < 3 ? bcn_at(fr.pc1, b, s, p) : (s < 6 ? bcn_at(fr.flow, b, s - 3, p) : bcn_at(fr.feature1, b, s - 6, p));
}

__global__ __launch_bounds__(256) void object_descriptors_kernel(const rtk_track_frame_t fr, int K, const int *__restrict__ obj,
                                                                 const int *__restrict__ num_objects, const int *__restrict__ prev_count,
                                                                 const float *__restrict__ desc_prev, float *__restrict__ desc) {
    __shared__ int s_list[256], s_wave[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const size_t base_b = (size_t)b * K * RTK_DESC;
    if (!stream_active(fr, b)) {          // the stream sits this frame out: its previous objects stay what they were
        int mp = prev_count[b];
        mp = mp < 0 ? 0 : (mp > K ? K : mp);
        for (int e = blockIdx.y * 256 + t; e < mp * RTK_DESC; e += gridDim.y * 256) desc[base_b + e] = desc_prev[base_b + e];
        return;
    }
    const int n = stream_points(fr, b), nobj = num_objects[b];
    const int *obj_b = obj + (size_t)b * fr.N;
    const bool is_prop = t < 128, is_stat = t >= 128 && t < 136;
    const int s = t - 128;
    for (int k = blockIdx.y; k < nobj; k += gridDim.y) {
        float acc = is_prop ? -INFINITY : 0.f, comp = 0.f, mean = 0.f;
        int cnt = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (int base = 0; base < n; base += 256) {
                const int p = base + t;
                const bool mine = p < n && obj_b[p] == k;
                int c;
                const int slot = ordered_slot(mine, s_wave, &c);
                if (mine) s_list[slot] = p;
                __syncthreads();
                if (pass == 0) {
                    if (is_prop) for (int q = 0; q < c; ++q) acc = fmaxf(acc, bcn_at(fr.prop, b, t, s_list[q]));
                    else if (is_stat) for (int q = 0; q < c; ++q) comp_add(acc, comp, stat_channel(fr, b, s, s_list[q]));
                    cnt += c;
                } else if (is_stat) {
                    for (int q = 0; q < c; ++q) {
                        const float d = stat_channel(fr, b, s, s_list[q]) - mean;
                        comp_add(acc, comp, d * d);
                    }
                }
                __syncthreads();
            }
            if (pass == 0) {
                float *dk = desc + base_b + (size_t)k * RTK_DESC;
                if (is_prop) dk[6 + t] = acc;
                if (is_stat) {
                    mean = acc / (float)cnt;
                    dk[s < 3 ? s : 131 + s] = mean;          // centre (0..2) | mean flow (134..136) | mean (RCS, v_r) (137..138)
                }
                acc = 0.f; comp = 0.f;
            } else if (is_stat && (s < 3 || s >= 6)) {
                desc[base_b + (size_t)k * RTK_DESC + (s < 3 ? 3 + s : 133 + s)] = acc / (float)cnt;   // var xyz (3..5) | var (139..140)
            }
        }
    }
}

extern "C" int rtk_object_descriptors(const rtk_track_frame_t *frame, int K, const int *obj, const int *num_objects,
                                      const int *prev_count, const float *desc_prev, float *desc, rtk_stream_t stream) {
    RTK_REQUIRE(frame_ok(frame) && obj && num_objects && prev_count && desc_prev && desc, "object_descriptors: bad arguments");
    TRACK_REQUIRE_K(K, "object_descriptors");
    dim3 grid(frame->B, K < DESC_G ? K : DESC_G);
    object_descriptors_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(*frame, K, obj, num_objects, prev_count, desc_prev, desc);
    RTK_CHECK_LAUNCH("object_descriptors");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_affinity_pairs: workgroup (b, y) takes the tiles y, y + G, ... of AFF_P pairs (row-major over (i prev, j curr), the reference's
// pair order) of stream b.  Activations live in LDS channel-major with the tile's pairs innermost ([c][AFF_P]); a thread computes one
// output channel for AFF_Q pairs: one weight load (coalesced across the wave: weights are stored transposed, (Cin, Cout)) per AFF_Q
// fp32 FMAs and one broadcast ds_read_b128.
// ------------------------------------------------------------------------------------------------
#define AFF_P 16
#define AFF_Q 4

__device__ __forceinline__ void aff_layer(const float *in, float *out, const float *__restrict__ wt, const float *__restrict__ bias,
                                          int cin, int cout, bool relu) {
    for (int e = threadIdx.x; e < cout * (AFF_P / AFF_Q); e += 256) {
        const int o = e % cout, g = e / cout;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        const float4 *x = reinterpret_cast<const float4 *>(in) + g;
        for (int c = 0; c < cin; ++c) {
            const float w = wt[(size_t)c * cout + o];
            const float4 v = x[c * (AFF_P / 4)];
            a0 = __fmaf_rn(v.x, w, a0);
            a1 = __fmaf_rn(v.y, w, a1);
            a2 = __fmaf_rn(v.z, w, a2);
            a3 = __fmaf_rn(v.w, w, a3);
        }
        const float bo = bias[o];
        a0 += bo; a1 += bo; a2 += bo; a3 += bo;
        if (relu) { a0 = fmaxf(a0, 0.f); a1 = fmaxf(a1, 0.f); a2 = fmaxf(a2, 0.f); a3 = fmaxf(a3, 0.f); }
        reinterpret_cast<float4 *>(out)[o * (AFF_P / 4) + g] = make_float4(a0, a1, a2, a3);
    }
}

__global__ __launch_bounds__(256) void affinity_pairs_kernel(int K, const float *__restrict__ W, const float *__restrict__ desc_prev,
                                                             const int *__restrict__ prev_count, const unsigned char *__restrict__ reset,
                                                             const float *__restrict__ desc, const int *__restrict__ num_objects,
                                                             float *__restrict__ aff) {
    __shared__ __attribute__((aligned(16))) float A[282 * AFF_P];      // input / layer-2 / layer-4 activations
    __shared__ __attribute__((aligned(16))) float Bf[564 * AFF_P];     // layer-1 / layer-3 activations
    const int b = blockIdx.x, t = threadIdx.x;
    int m = (reset && reset[b]) ? 0 : prev_count[b];
    m = m < 0 ? 0 : (m > K ? K : m);
    int n = num_objects[b];                          // inactive streams report no objects: no pairs
    n = n < 0 ? 0 : (n > K ? K : n);
    const int pairs = m * n;
    const float *W1 = W, *b1 = W1 + 141 * 564, *W2 = b1 + 564, *b2 = W2 + 564 * 282, *W3 = b2 + 282, *b3 = W3 + 282 * 70;
    const float *W4 = b3 + 70, *b4 = W4 + 70 * 35, *W5 = b4 + 35, *b5 = W5 + 35;
    const float *dc = desc + (size_t)b * K * RTK_DESC, *dp = desc_prev + (size_t)b * K * RTK_DESC;
    for (int q0 = blockIdx.y * AFF_P; q0 < pairs; q0 += gridDim.y * AFF_P) {
        for (int e = t; e < RTK_DESC * AFF_P; e += 256) {
            const int c = e / AFF_P, q = q0 + e % AFF_P;
            float v = 0.f;
            if (q < pairs) {
                const int i = q / n, j = q % n;
                v = dc[(size_t)j * RTK_DESC + c] - dp[(size_t)i * RTK_DESC + c];     // curr_j - prev_i
            }
            A[e] = v;
        }
        __syncthreads();
        aff_layer(A, Bf, W1, b1, 141, 564, true);
        __syncthreads();
        aff_layer(Bf, A, W2, b2, 564, 282, true);
        __syncthreads();
        aff_layer(A, Bf, W3, b3, 282, 70, true);
        __syncthreads();
        aff_layer(Bf, A, W4, b4, 70, 35, true);
        __syncthreads();
        if (t < AFF_P && q0 + t < pairs) {
            float a = 0.f;
            for (int c = 0; c < 35; ++c) a = __fmaf_rn(A[c * AFF_P + t], W5[c], a);
            a += b5[0];
            const int q = q0 + t, i = q / n, j = q % n;
            aff[((size_t)b * K + i) * K + j] = 1.f / (1.f + expf(-a));
        }
        __syncthreads();
    }
}

extern "C" int rtk_affinity_pairs(int B, int K, const float *weights, const float *desc_prev, const int *prev_count,
                                  const unsigned char *reset, const float *desc, const int *num_objects, float *aff,
                                  rtk_stream_t stream) {
    RTK_REQUIRE(B > 0 && B <= 65535 && weights && desc_prev && prev_count && desc && num_objects && aff, "affinity_pairs: bad arguments");
    TRACK_REQUIRE_K(K, "affinity_pairs");
    // enough tiles per stream in flight to fill the device at small B, few idle workgroups at large B
    int g = rtk_divup(2048, B), tiles = rtk_divup((long)K * K, AFF_P);
    g = g < 4 ? 4 : (g > tiles ? tiles : g);
    affinity_pairs_kernel<<<dim3(B, g), 256, 0, (hipStream_t)stream>>>(K, weights, desc_prev, prev_count, reset, desc, num_objects, aff);
    RTK_CHECK_LAUNCH("affinity_pairs");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_associate_batched: one workgroup per stream (association.sinkhorn_assignment + Associator.__call__).
// ------------------------------------------------------------------------------------------------
struct AssocArgs {
    int N, K;
    const unsigned char *active, *reset;
    const float *aff;
    const int *num_objects, *obj, *prev_ids, *prev_count;
    float alpha;
    int iters;
    int *counter, *ids, *count, *object_ids;
    float *object_conf;
    int *indices1, *num_prev, *point_track_id;
    float *scores;
};

__global__ __launch_bounds__(256) void associate_batched_kernel(const AssocArgs a) {
    extern __shared__ __attribute__((aligned(16))) float as_smem[];
    __shared__ int s_wave[4];
    const int b = blockIdx.x, t = threadIdx.x, K = a.K, N = a.N;
    const int *prev_ids = a.prev_ids + (size_t)b * K;
    int *object_ids = a.object_ids + (size_t)b * K, *indices1 = a.indices1 + (size_t)b * K;
    float *object_conf = a.object_conf + (size_t)b * K;
    const float *aff = a.aff + (size_t)b * K * K;
    int mp = a.prev_count[b];
    mp = mp < 0 ? 0 : (mp > K ? K : mp);
    if (a.active && !a.active[b]) {       // state carried over, nothing reported
        for (int e = t; e < K; e += 256) {
            a.ids[(size_t)b * K + e] = prev_ids[e];
            object_ids[e] = -1; object_conf[e] = 0.f; indices1[e] = -1;
        }
        for (int p = t; p < N; p += 256) a.point_track_id[(size_t)b * N + p] = -1;
        if (t == 0) { a.count[b] = mp; a.num_prev[b] = 0; }
        return;
    }
    const int m = (a.reset && a.reset[b]) ? 0 : mp;
    int n = a.num_objects[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    const int R = m + 1, C = n + 1, ld = C | 1;           // the layout of log_sinkhorn_kernel
    float *Z = as_smem, *u = Z + R * ld, *v = u + R;
    const size_t table = (size_t)(K + 1) * ((K + 1) | 1) + 2 * (size_t)(K + 1);
    float *max0 = as_smem + table;
    int *ind0 = reinterpret_cast<int *>(max0 + K), *ind1 = ind0 + K, *dec = ind1 + K, *sid = dec + K;
    const bool assoc = m > 0 && n > 0;
    if (assoc) {
        // ---- log_optimal_transport of this stream's live block (rtk_log_sinkhorn's) ----
        const float norm = log_ot_lds(m, n, aff, K, a.alpha, a.iters, Z, ld, u, v);
        if (a.scores) {                                   // optional: the whole (m+1, n+1) plan, rtk_log_sinkhorn's `out`
            float *sc = a.scores + (size_t)b * (K + 1) * (K + 1);
            for (int e = t; e < R * C; e += 256) {
                const int i = e / C, j = e % C;
                sc[(size_t)i * (K + 1) + j] = log_ot_plan(Z, ld, u, v, norm, i, j);
            }
            __syncthreads();                              // (the block below overwrites Z)
        }
        for (int e = t; e < m * n; e += 256) {            // the scores block, in place (each element read and written by one thread)
            const int i = e / n, j = e % n;
            Z[i * ld + j] = log_ot_plan(Z, ld, u, v, norm, i, j);
        }
        __syncthreads();
        // ---- mutual best match.  Exact ties: the lowest index wins (strict > while scanning upwards) ----
        for (int i = t; i < m; i += 256) {
            float mx = Z[i * ld];
            int arg = 0;
            for (int j = 1; j < n; ++j)
                if (Z[i * ld + j] > mx) { mx = Z[i * ld + j]; arg = j; }
            max0[i] = mx; ind0[i] = arg;
        }
        for (int j = t; j < n; j += 256) {
            float mx = Z[j];
            int arg = 0;
            for (int i = 1; i < m; ++i)
                if (Z[i * ld + j] > mx) { mx = Z[i * ld + j]; arg = i; }
            ind1[j] = arg;
        }
        __syncthreads();
        // valid0[k] = mutual0[k] & exp(max0[k]) > 0;  indices1[j] = mutual1[j] & valid0[ind1[j]] ? ind1[j] : -1
        for (int j = t; j < n; j += 256) {
            const int k = ind1[j];
            const bool mutual1 = ind0[k] == j;            // then mutual0[k] holds too
            dec[j] = (mutual1 && expf(max0[k]) > 0.f) ? k : -1;
        }
        __syncthreads();
    }
    // ---- track IDs: unmatched or aff < 0.01 -> a fresh ID from the counter, in current-object order ----
    const int next = a.counter[b];
    int nfresh_total = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {                 // K <= 256: one pass in practice
        const int j = j0 + t;
        int k = -1;
        float conf = 0.f;
        if (j < n && assoc) {
            k = dec[j];
            if (k >= 0) conf = aff[(size_t)k * K + j];
        }
        const bool fresh = j < n && (k < 0 || (double)conf < 0.01);
        int c;
        const int slot = ordered_slot(fresh, s_wave, &c);
        if (j < n) {
            const int id = fresh ? next + nfresh_total + slot : prev_ids[k];
            sid[j] = id;
            object_ids[j] = id;
            object_conf[j] = fresh ? 0.f : conf;
            indices1[j] = assoc ? k : -1;
        }
        nfresh_total += c;
    }
    for (int j = n + t; j < K; j += 256) { object_ids[j] = -1; object_conf[j] = 0.f; indices1[j] = -1; }
    __syncthreads();
    if (t == 0) { a.counter[b] = next + nfresh_total; a.count[b] = n; a.num_prev[b] = m; }
    for (int j = t; j < n; j += 256) a.ids[(size_t)b * K + j] = sid[j];
    const int *obj_b = a.obj + (size_t)b * N;
    for (int p = t; p < N; p += 256) {
        const int o = obj_b[p];
        a.point_track_id[(size_t)b * N + p] = (o >= 0 && o < n) ? sid[o] : -1;
    }
}

extern "C" int rtk_associate_batched(int B, int N, int K, const unsigned char *active, const unsigned char *reset, const float *aff,
                                     const int *num_objects, const int *obj, const int *prev_ids, const int *prev_count, float alpha,
                                     int iters, int *counter, int *ids, int *count, int *object_ids, float *object_conf, int *indices1,
                                     int *num_prev, int *point_track_id, float *scores, rtk_stream_t stream) {
    RTK_REQUIRE(B > 0 && B <= 65535 && N > 0 && iters >= 0 && aff && num_objects && obj && prev_ids && prev_count && counter && ids &&
                count && object_ids && object_conf && indices1 && num_prev && point_track_id, "associate_batched: bad arguments");
    TRACK_REQUIRE_K(K, "associate_batched");
    const AssocArgs a = {N, K, active, reset, aff, num_objects, obj, prev_ids, prev_count, alpha, iters, counter, ids, count,
                         object_ids, object_conf, indices1, num_prev, point_track_id, scores};
    (void)hipFuncSetAttribute((const void *)associate_batched_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)assoc_lds_bytes(K));
    associate_batched_kernel<<<B, 256, assoc_lds_bytes(K), (hipStream_t)stream>>>(a);
    RTK_CHECK_LAUNCH("associate_batched");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_track_memory: one workgroup per stream, thread t = row t of the tables (K <= 256).  The rules are stated once, in rtk_fused.h.
// The matched mask of the previous rows comes from indices1 / object_conf; a survivor's position is its rank among the survivors
// (ordered_slot: ballot + prefix over the four waves); the descriptor rows then move element by element, consecutive threads on
// consecutive floats.  Plain stores to rows that no other thread writes: nothing depends on the order of execution.
// ------------------------------------------------------------------------------------------------
struct MemArgs {
    int K, max_age;
    const unsigned char *active, *reset;
    const int *num_objects, *indices1;
    const float *object_conf;
    const int *prev_ids, *prev_age, *prev_hits, *prev_n_det, *prev_count;
    const float *desc_prev;
    int *ids, *age, *hits, *n_det, *count;
    float *desc;
    int *flags, *object_hits, *object_gap, *num_coasted;
};

__global__ __launch_bounds__(256) void track_memory_kernel(const MemArgs a) {
    __shared__ int s_wave[4], s_matched[256], s_src[256];
    const int b = blockIdx.x, t = threadIdx.x, K = a.K;
    const size_t row0 = (size_t)b * K;
    const int *prev_ids = a.prev_ids + row0, *prev_age = a.prev_age + row0, *prev_hits = a.prev_hits + row0;
    int *ids = a.ids + row0, *age = a.age + row0, *hits = a.hits + row0;
    int *object_hits = a.object_hits + row0, *object_gap = a.object_gap + row0;
    const int mp = count_clamp(a.prev_count[b], K);
    if (a.active && !a.active[b]) {       // the table stays what it was (ids and count: rtk_associate_batched); no track ages
        if (t < K) { age[t] = prev_age[t]; hits[t] = prev_hits[t]; object_hits[t] = 0; object_gap[t] = -1; }
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
    } else if (t < K) {
        object_hits[t] = 0; object_gap[t] = -1;
    }
    const int pa = t < m ? prev_age[t] : 0;
    const bool survives = t < m && !s_matched[t] && pa < a.max_age;       // age + 1 <= max_age
    int S;
    const int slot = ordered_slot(survives, s_wave, &S);
    const int cnt = n + S < K ? n + S : K;
    if (survives && n + slot < K) {
        const int r = n + slot;
        ids[r] = prev_ids[t]; age[r] = pa + 1; hits[r] = prev_hits[t];
        s_src[slot] = t;
    }
    if (t >= cnt && t < K) { ids[t] = -1; age[t] = 0; hits[t] = 0; }
    if (t == 0) {
        a.count[b] = cnt; a.n_det[b] = n; a.num_coasted[b] = cnt - n;
        if (n + S > K) a.flags[b] |= 4;
    }
    __syncthreads();
    const unsigned *src = reinterpret_cast<const unsigned *>(a.desc_prev) + row0 * RTK_DESC;
    unsigned *dst = reinterpret_cast<unsigned *>(a.desc) + (row0 + n) * RTK_DESC;
    for (int e = t; e < (cnt - n) * RTK_DESC; e += 256) dst[e] = src[(size_t)s_src[e / RTK_DESC] * RTK_DESC + e % RTK_DESC];
}

extern "C" int rtk_track_memory(int B, int K, int max_age, const unsigned char *active, const unsigned char *reset,
                                const int *num_objects, const int *indices1, const float *object_conf, const int *prev_ids,
                                const int *prev_age, const int *prev_hits, const int *prev_n_det, const int *prev_count,
                                const float *desc_prev, int *ids, int *age, int *hits, int *n_det, int *count, float *desc, int *flags,
                                int *object_hits, int *object_gap, int *num_coasted, rtk_stream_t stream) {
    RTK_REQUIRE(B > 0 && B <= 65535 && num_objects && indices1 && object_conf && prev_ids && prev_age && prev_hits && prev_n_det &&
                prev_count && desc_prev && ids && age && hits && n_det && count && desc && flags && object_hits && object_gap &&
                num_coasted, "track_memory: bad arguments");
    TRACK_REQUIRE_K(K, "track_memory");
    RTK_REQUIRE(max_age >= 0, "track_memory: max_age=%d is negative", max_age);
    RTK_REQUIRE(ids != prev_ids && age != prev_age && hits != prev_hits && desc != desc_prev,
                "track_memory: the new table must not alias the previous one");
    const MemArgs a = {K, max_age, active, reset, num_objects, indices1, object_conf, prev_ids, prev_age, prev_hits, prev_n_det, prev_count,
                       desc_prev, ids, age, hits, n_det, count, desc, flags, object_hits, object_gap, num_coasted};
    track_memory_kernel<<<B, 256, 0, (hipStream_t)stream>>>(a);
    RTK_CHECK_LAUNCH("track_memory");
    return RTK_OK;
}
