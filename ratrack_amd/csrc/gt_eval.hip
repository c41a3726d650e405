// gt_eval.hip -- ground truth and scoring of a batch of frame pairs on the device (include/rtk_gt.h, ratrack_amd/gt_device.py).
//
//   rtk_gt_labels    one workgroup per stream: oriented-box membership of both frames (float64), the GT ids of frame 1, the
//                    ego-motion compensated cloud and the GT warped positions (what vod_gt.filter_object_points + gt_scene_flow
//                    compute per frame on the host; track4d_utils.py:105-141, :337-359)
//   rtk_eval_frame   one workgroup per stream: the sums and the values of metrics.eval_scene_flow / eval_motion_seg
//                    (main_utils.py:272-389), float64
//
// Layout of both: 256 threads = 4 waves of 64; a thread owns the columns t, t + 256, ... of its stream.  The box tables of a stream
// (both frames: 16 float64 per box, the motion matrices, the pairing, the counters) sit in LDS; every lane of a wave reads the SAME
// box word at a time (a broadcast: no bank conflict whatever the layout).  Per-box point counts are one ballot + popcount per wave
// and box; the metric sums are per-thread float64 partials, a wave64 shuffle tree, then the four wave results added in wave order
// by one thread per sum: a fixed order, the same bits on every run.
//
// What is float64 and why: membership is a comparison, and the host path (Open3D's test restated in vod_gt.points_in_box) makes it
// in float64 -- an fp32 projection would move points across a face.  The metrics are float64 because the reference's thresholds
// (sas / ras) and its epoch means are taken on values of very different magnitudes and the fixtures pin them to 1e-6.  The only fp32
// arithmetic is the application of the box motion, which the reference also does in fp32.
#include <math.h>

#include "batch_common.h"
#include "rtk_common.h"
#include "rtk_gt.h"

#define GT_THREADS 256
#define GT_WAVES (GT_THREADS / RTK_WAVE)

// per-stream LDS: box1[K][16] | box2[K][16] (float64) | motion[K][12] (fp32) | pair[K] | id1[K] | c1[K] | c2[K] (int32)
static size_t gt_lds_bytes(int K) { return (size_t)K * (2 * RTK_GT_BOX_WORDS * sizeof(double) + 12 * sizeof(float) + 4 * sizeof(int)); }

__global__ __launch_bounds__(GT_THREADS) void gt_labels_kernel(const rtk_gt_in_t in, const rtk_gt_out_t out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gt_smem[];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1);
    const int N = in.N, N2 = in.N2, K = in.K;
    double *box1 = reinterpret_cast<double *>(gt_smem), *box2 = box1 + (size_t)K * RTK_GT_BOX_WORDS;
    float *mot = reinterpret_cast<float *>(box2 + (size_t)K * RTK_GT_BOX_WORDS);
    int *pair = reinterpret_cast<int *>(mot + (size_t)K * 12), *id1 = pair + K, *c1 = id1 + K, *c2 = c1 + K;

    const int raw1 = in.frame1.count[b], raw2 = in.frame2.count[b];
    const int cnt1 = count_clamp(raw1, K), cnt2 = count_clamp(raw2, K);
    const int nv1 = in.n_valid ? in.n_valid[b] : N, nv2 = in.n_valid ? in.n_valid[in.B + b] : N2;
    const int n1 = count_clamp(nv1, N), n2 = count_clamp(nv2, N2);
    if (t == 0) out.flags[b] = ((raw1 != cnt1 || raw2 != cnt2) ? 1 : 0) | ((nv1 != n1 || nv2 != n2) ? 2 : 0);

    const size_t kb = (size_t)b * K;
    for (int e = t; e < cnt1 * RTK_GT_BOX_WORDS; e += GT_THREADS) box1[e] = in.frame1.boxes[kb * RTK_GT_BOX_WORDS + e];
    for (int e = t; e < cnt2 * RTK_GT_BOX_WORDS; e += GT_THREADS) box2[e] = in.frame2.boxes[kb * RTK_GT_BOX_WORDS + e];
    for (int e = t; e < cnt1 * 12; e += GT_THREADS) mot[e] = in.motion[kb * 12 + e];
    for (int k = t; k < K; k += GT_THREADS) {
        int pr = k < cnt1 ? in.pair[kb + k] : -1;
        pair[k] = (pr >= 0 && pr < cnt2) ? pr : -1;
        id1[k] = k < cnt1 ? in.frame1.box_id[kb + k] : -1;
        c1[k] = 0;
        c2[k] = 0;
    }
    __syncthreads();

    // ---- frame 2: how many valid points each box holds ----
    for (int base = 0; base < n2; base += GT_THREADS) {
        const int p = base + t;
        const bool live = p < n2;
        double x = 0.0, y = 0.0, z = 0.0;
        if (live) { x = (double)bcn_at(in.pc2, b, 0, p); y = (double)bcn_at(in.pc2, b, 1, p); z = (double)bcn_at(in.pc2, b, 2, p); }
        for (int k = 0; k < cnt2; ++k) {
            const bool hit = live && box_inside(box2 + (size_t)k * RTK_GT_BOX_WORDS, x, y, z);
            const unsigned long long m = __ballot(hit);
            if (lane == 0 && m) atomicAdd(&c2[k], __popcll(m));
        }
    }
    __syncthreads();

    // ---- frame 1: ids, compensated position, GT warped position ----
    const double *E = in.ego ? in.ego + (size_t)b * 12 : nullptr;
    const size_t pb = (size_t)b * N, cb = (size_t)b * 3 * N;
    for (int base = 0; base < N; base += GT_THREADS) {
        const int p = base + t;
        const bool col = p < N, live = p < n1;
        float xf = 0.f, yf = 0.f, zf = 0.f;
        if (col) { xf = bcn_at(in.pc1, b, 0, p); yf = bcn_at(in.pc1, b, 1, p); zf = bcn_at(in.pc1, b, 2, p); }
        const double x = (double)xf, y = (double)yf, z = (double)zf;
        int last = -1;
        for (int k = 0; k < cnt1; ++k) {
            const bool hit = live && box_inside(box1 + (size_t)k * RTK_GT_BOX_WORDS, x, y, z);
            const unsigned long long m = __ballot(hit);
            if (lane == 0 && m) atomicAdd(&c1[k], __popcll(m));
            last = hit ? k : last;
        }
        if (!col) continue;
        float comp[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (E) {
                comp[j] = (float)(((x * E[4 * j] + y * E[4 * j + 1]) + z * E[4 * j + 2]) + E[4 * j + 3]);
                out.pc1_comp[cb + (size_t)j * N + p] = comp[j];
            } else {
                comp[j] = out.pc1_comp[cb + (size_t)j * N + p];
            }
        }
        out.gt_cls[pb + p] = last >= 0 ? 1 : 0;
        out.box_index[pb + p] = last;
        out.obj_id[pb + p] = last >= 0 ? id1[last] : -1;
        const int partner = last >= 0 ? pair[last] : -1;
        const bool moves = partner >= 0 && c2[partner] > 0;
        const float *T = mot + (size_t)(last >= 0 ? last : 0) * 12;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float w = ((T[4 * j] * xf + T[4 * j + 1] * yf) + T[4 * j + 2] * zf) + T[4 * j + 3];
            out.gt_warp[cb + (size_t)j * N + p] = moves ? w : comp[j];
        }
    }
    __syncthreads();
    for (int k = t; k < K; k += GT_THREADS) {
        out.counts1[kb + k] = c1[k];
        out.counts2[kb + k] = c2[k];
    }
}

static int gt_view_ok(const rtk_bcn_view_t *v) { return v->ptr != nullptr; }

extern "C" int rtk_gt_labels(const rtk_gt_in_t *in, const rtk_gt_out_t *out, rtk_stream_t stream) {
    RTK_REQUIRE(in && out, "gt_labels: null argument block");
    RTK_REQUIRE(in->B >= 1 && in->B <= 65535 && in->N >= 1 && in->N2 >= 1, "gt_labels: bad sizes B=%d N=%d N2=%d", in->B, in->N, in->N2);
    RTK_REQUIRE(in->K >= 1 && in->K <= RTK_GT_MAX_BOXES, "gt_labels: K=%d box slots outside [1, %d] (both frames' tables of a stream "
                "must fit one workgroup's LDS)", in->K, RTK_GT_MAX_BOXES);
    RTK_REQUIRE(gt_view_ok(&in->pc1) && gt_view_ok(&in->pc2) && in->frame1.boxes && in->frame1.box_id && in->frame1.count &&
                in->frame2.boxes && in->frame2.box_id && in->frame2.count && in->pair && in->motion, "gt_labels: null input");
    RTK_REQUIRE(out->gt_cls && out->box_index && out->obj_id && out->gt_warp && out->pc1_comp && out->counts1 && out->counts2 &&
                out->flags, "gt_labels: null output");
    const size_t lds = gt_lds_bytes(in->K);
    (void)hipFuncSetAttribute((const void *)gt_labels_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gt_lds_bytes(RTK_GT_MAX_BOXES));
    gt_labels_kernel<<<in->B, GT_THREADS, lds, (hipStream_t)stream>>>(*in, *out);
    RTK_CHECK_LAUNCH("gt_labels");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_eval_frame
// ------------------------------------------------------------------------------------------------
// sqrt(sum_j sum_i |J_ji| res_i + 1e-20): the per-point Cartesian resolution of a sensor with range / elevation / azimuth
// resolution res (main_utils.py:272-311), from the spherical angles of the point
__device__ __forceinline__ double eval_resolution(double r, double st, double ct, double sp, double cp, const double *res) {
    const double gx = (fabs(cp * ct) * res[0] + fabs(-r * st * cp) * res[1]) + fabs(-r * ct * sp) * res[2];
    const double gy = (fabs(sp * ct) * res[0] + fabs(-r * sp * st) * res[1]) + fabs(r * ct * cp) * res[2];
    const double gz = (fabs(st) * res[0] + fabs(r * ct) * res[1]) + 0.0 * res[2];
    return sqrt(((gx + gy) + gz) + 1e-20);
}

__device__ __forceinline__ double eval_wave_sum(double v) {
#pragma unroll
    for (int d = RTK_WAVE / 2; d >= 1; d >>= 1) v += __shfl_down(v, d, RTK_WAVE);
    return v;      // lane 0 holds the wave's sum
}

__global__ __launch_bounds__(GT_THREADS) void eval_frame_kernel(const rtk_eval_in_t in, double *__restrict__ sums,
                                                                double *__restrict__ values) {
    __shared__ double s_part[GT_WAVES][RTK_EVAL_SUMS];
    __shared__ double s_tot[RTK_EVAL_SUMS];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1), wave = t / RTK_WAVE, N = in.N;
    double *S = sums + (size_t)b * RTK_EVAL_SUMS, *V = values + (size_t)b * RTK_EVAL_VALUES;
    if (in.active && !in.active[b]) {
        if (t < RTK_EVAL_SUMS) S[t] = 0.0;
        if (t < RTK_EVAL_VALUES) V[t] = 0.0;
        return;
    }
    const int n = in.n_valid ? count_clamp(in.n_valid[b], N) : N;
    // LRR30 radar / HDL-64E lidar: range (m), elevation, azimuth (rad)
    const double pi = 3.141592653589793;
    const double res_radar[3] = {0.2, 1.0 * pi / 180, 1.6 * pi / 180};
    const double res_lidar[3] = {0.04, 0.4 * pi / 180, 0.08 * pi / 180};
    double acc[RTK_EVAL_SUMS];
#pragma unroll
    for (int i = 0; i < RTK_EVAL_SUMS; ++i) acc[i] = 0.0;
    const float *mask = in.mask + (size_t)b * N;
    const unsigned char *gcls = in.gt_cls + (size_t)b * N;
    for (int p = t; p < n; p += GT_THREADS) {
        const double x = (double)bcn_at(in.pc1, b, 0, p), y = (double)bcn_at(in.pc1, b, 1, p), z = (double)bcn_at(in.pc1, b, 2, p);
        double e2 = 0.0, l2 = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double w = (double)bcn_at(in.warp, b, j, p), g = (double)bcn_at(in.gt_warp, b, j, p), d = w - g;
            e2 += d * d;
            l2 += g * g;
        }
        const double error = sqrt(e2 + 1e-20), gt_len = sqrt(l2 + 1e-20);
        const double r = sqrt((x * x + y * y) + z * z);
        const double theta = asin(z / r), phi = atan2(y, x);
        const double st = sin(theta), ct = cos(theta), sp = sin(phi), cp = cos(phi);
        const double res_r = eval_resolution(r, st, ct, sp, cp, res_radar), res_l = eval_resolution(r, st, ct, sp, cp, res_lidar);
        const double rn = error / (res_r / res_l);
        const float m = mask[p];
        const bool moving = m == 0.f, is_static = m == 1.f;
        acc[0] += 1.0;
        acc[1] += error;
        acc[2] += rn;
        if (moving) { acc[3] += rn; acc[4] += 1.0; }
        if (is_static) { acc[5] += rn; acc[6] += 1.0; }
        const double rel = rn / gt_len;
        if (rn <= 0.10 || rel <= 0.10) acc[7] += 1.0;
        if (rn <= 0.20 || rel <= 0.20) acc[8] += 1.0;
        const bool pre = bcn_at(in.cls, b, 0, p) > in.threshold, gt = gcls[p] != 0;
        acc[9] += (pre && gt) ? 1.0 : 0.0;        // tp
        acc[10] += (!pre && !gt) ? 1.0 : 0.0;     // tn
        acc[11] += (pre && !gt) ? 1.0 : 0.0;      // fp
        acc[12] += (!pre && gt) ? 1.0 : 0.0;      // fn
    }
#pragma unroll
    for (int i = 0; i < RTK_EVAL_SUMS; ++i) {
        const double w = eval_wave_sum(acc[i]);
        if (lane == 0) s_part[wave][i] = w;
    }
    __syncthreads();
    if (t < RTK_EVAL_SUMS) {
        double v = s_part[0][t];
#pragma unroll
        for (int w = 1; w < GT_WAVES; ++w) v += s_part[w][t];
        s_tot[t] = v;
        S[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        const double cnt = s_tot[0];
        const double mov = s_tot[3] / (s_tot[4] + 1e-6), stat = s_tot[5] / s_tot[6];      // 0 / 0: NaN, the mean of an empty slice
        const double tp = s_tot[9] + 1e-20, tn = s_tot[10] + 1e-20, fp = s_tot[11] + 1e-20, fn = s_tot[12] + 1e-20;
        V[0] = s_tot[2] / cnt;
        V[1] = (mov + stat) / 2;
        V[2] = mov;
        V[3] = stat;
        V[4] = s_tot[7] / cnt;
        V[5] = s_tot[8] / cnt;
        V[6] = s_tot[1] / cnt;
        V[7] = (tp + tn) / (((tp + tn) + fp) + fn);
        V[8] = tp / (tp + fn);
        V[9] = 0.5 * (tp / (((tp + fp) + fn) + 1e-4) + tn / (((tn + fp) + fn) + 1e-4));
    }
}

extern "C" int rtk_eval_frame(const rtk_eval_in_t *in, double *sums, double *values, rtk_stream_t stream) {
    RTK_REQUIRE(in && sums && values, "eval_frame: null argument");
    RTK_REQUIRE(in->B >= 1 && in->B <= 65535 && in->N >= 1, "eval_frame: bad sizes B=%d N=%d", in->B, in->N);
    RTK_REQUIRE(gt_view_ok(&in->pc1) && gt_view_ok(&in->warp) && gt_view_ok(&in->gt_warp) && gt_view_ok(&in->cls) && in->mask &&
                in->gt_cls, "eval_frame: null input");
    eval_frame_kernel<<<in->B, GT_THREADS, 0, (hipStream_t)stream>>>(*in, sums, values);
    RTK_CHECK_LAUNCH("eval_frame");
    return RTK_OK;
}
