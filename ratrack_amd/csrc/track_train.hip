// track_train.hip -- the backward of the tracking term (losses/loss.py:48-72) for B streams at once (ratrack_amd/track_train.py):
//
//   rtk_affinity_train          BCE -> sigmoid -> the five-layer Affinity MLP on every live (previous, current) pair: loss (B), the
//                               gradient of the current objects' descriptors, and the pairs' activations / pre-activation gradients
//                               in the workspace
//   rtk_affinity_wgrad          the gradient of the packed weight image from those rows
//   rtk_object_descriptors_bwd  descriptor gradients -> flow (through the mean) and prop (through the max)
//
// fp32 throughout, no floating-point atomics: every sum has one order (stated at each kernel), so the term is reproducible bit for
// bit.  The forward's chains are rtk_affinity_pairs' (one fmaf chain per output); the backward's own sums -- over up to 564 channels,
// 128 previous objects, 512 rows -- are blocked: short chains added up in a fixed order, whose rounding error grows with the
// number of blocks instead of the number of terms (a plain chain over 500 rows sat at 1.1e-6 of the gradient's largest element).
// The launch count depends on nothing; the streams' counts stay on the device.
#include <math.h>

#include "assoc_common.h"
#include "batch_common.h"
#include "rtk_common.h"
#include "rtk_fused.h"
#include "rtk_train.h"

#define TT_P 16                      // pairs per tile (rtk_affinity_pairs' AFF_P: the forward is its arithmetic)
#define TT_ROW RTK_AFF_TRAIN_ROW
#define TT_ACT 1092                  // 141 + 564 + 282 + 70 + 35: a row's activations
#define TT_DELTA 951                 // 564 + 282 + 70 + 35: a row's hidden pre-activation gradients, behind the activations
#define TT_D1 1092
#define TT_D5 2043
#define TT_TERM 2044
#define TT_NW RTK_AFFINITY_WEIGHTS
#define TT_BLOCK 32                  // the backward's sums are blocked: chains of at most this many terms, the blocks added in order

// the live block of stream b, with rtk_affinity_pairs' clamping; 0 pairs when the stream sits the term out
struct TtStreams {
    int K;
    const int *prev_count, *num_objects;
    const unsigned char *reset, *active, *aff_defined;
};

__device__ __forceinline__ int tt_block(const TtStreams &s, int b, int *m_out, int *n_out) {
    int m = (s.reset && s.reset[b]) ? 0 : s.prev_count[b];
    m = count_clamp(m, s.K);
    const int n = count_clamp(s.num_objects[b], s.K);
    *m_out = m;
    *n_out = n;
    if ((s.active && !s.active[b]) || !s.aff_defined[b]) return 0;
    return m * n;
}

// ------------------------------------------------------------------------------------------------
// Launch 1: the streams' first rows.  One workgroup scans the pair counts in stream order; a stream whose rows would end beyond
// max_pairs is flagged and left out (the running sum is monotonic: so is every stream with pairs behind it).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tt_prefix_kernel(int B, TtStreams s, int max_pairs, int *__restrict__ pair_offset,
                                                        int *__restrict__ flags) {
    __shared__ int scan[256];
    __shared__ unsigned long long s_total;
    const int t = threadIdx.x;
    if (t == 0) s_total = 0ull;
    long long carry = 0;
    for (int base = 0; base < B; base += 256) {
        const int b = base + t;
        int m, n;
        const int cnt = b < B ? tt_block(s, b, &m, &n) : 0;
        scan[t] = cnt;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int v = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const long long end = carry + scan[t];
        if (b < B) {
            const bool over = cnt > 0 && end > (long long)max_pairs;
            pair_offset[b] = over ? -1 : (int)(end - cnt > (long long)max_pairs ? max_pairs : end - cnt);
            flags[b] = over ? 1 : 0;
            if (!over && cnt > 0) atomicMax(&s_total, (unsigned long long)end);
        }
        carry += scan[255];
        __syncthreads();
    }
    if (t == 0) pair_offset[B] = (int)s_total;
}

// the cross-entropy term of one pair, F.binary_cross_entropy's: logs clamped at -100
__device__ __forceinline__ float tt_bce(float a, float tg) {
    const float la = fmaxf(logf(a), -100.f), l1a = fmaxf(log1pf(-a), -100.f);
    return (tg - 1.f) * l1a - tg * la;
}

// a workgroup's sum of one float per thread, as a fixed tree
__device__ __forceinline__ float tt_block_sum(float v, float *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) red[t] += red[t + d];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------------------
// Loss only (scale == NULL): one workgroup per stream reads aff; thread t adds the pairs t, t + 256, ..., then the tree.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tt_loss_kernel(TtStreams s, const int *__restrict__ pair_offset, const float *__restrict__ aff,
                                                      const float *__restrict__ target, float *__restrict__ loss) {
    __shared__ float red[256];
    const int b = blockIdx.x, t = threadIdx.x, K = s.K;
    int m, n;
    int pairs = tt_block(s, b, &m, &n);
    if (pair_offset[b] < 0) pairs = 0;
    float acc = 0.f;
    for (int q = t; q < pairs; q += 256) {
        const size_t at = ((size_t)b * K + q / n) * K + q % n;
        acc += tt_bce(aff[at], target[at]);
    }
    const float sum = tt_block_sum(acc, red);
    if (t == 0) loss[b] = pairs ? sum / (float)pairs : 0.f;
}

// ------------------------------------------------------------------------------------------------
// Launch 2: workgroup (b, y) takes the tiles y, y + G, ... of TT_P pairs of stream b.  The tile's activations live in LDS
// channel-major with the pairs innermost ([c][TT_P]), all five tensors one after the other, so that a tile's part of the
// workspace rows is one strided copy.  Forward: rtk_affinity_pairs' layers (same chains).  Backward: the gradient of a hidden
// layer overwrites that layer's activation in place, each element by the thread that read its ReLU mask.
// ------------------------------------------------------------------------------------------------
template <bool BWD>
__device__ __forceinline__ void tt_layer(const float *in, float *out, const float *__restrict__ wt, const float *__restrict__ bias,
                                         int cin, int cout) {
    for (int e = threadIdx.x; e < cout * (TT_P / 4); e += 256) {
        const int o = e % cout, g = e / cout;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        const float4 *x = reinterpret_cast<const float4 *>(in) + g;
        if (BWD) {      // blocks of TT_BLOCK channels, one fmaf chain each, added up in block order (see the file header)
            for (int c0 = 0; c0 < cin; c0 += TT_BLOCK) {
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                const int c1 = c0 + TT_BLOCK < cin ? c0 + TT_BLOCK : cin;
                for (int c = c0; c < c1; ++c) {
                    const float w = wt[(size_t)c * cout + o];
                    const float4 v = x[c * (TT_P / 4)];
                    s0 = __fmaf_rn(v.x, w, s0);
                    s1 = __fmaf_rn(v.y, w, s1);
                    s2 = __fmaf_rn(v.z, w, s2);
                    s3 = __fmaf_rn(v.w, w, s3);
                }
                a0 += s0; a1 += s1; a2 += s2; a3 += s3;
            }
        } else {        // the forward is rtk_affinity_pairs': one chain over all input channels
            for (int c = 0; c < cin; ++c) {
                const float w = wt[(size_t)c * cout + o];
                const float4 v = x[c * (TT_P / 4)];
                a0 = __fmaf_rn(v.x, w, a0);
                a1 = __fmaf_rn(v.y, w, a1);
                a2 = __fmaf_rn(v.z, w, a2);
                a3 = __fmaf_rn(v.w, w, a3);
            }
        }
        float4 *dst = reinterpret_cast<float4 *>(out) + o * (TT_P / 4) + g;
        if (BWD) {      // out holds the layer's ReLU output: its mask (torch's threshold_backward: output > 0)
            const float4 h = *dst;
            *dst = make_float4(h.x > 0.f ? a0 : 0.f, h.y > 0.f ? a1 : 0.f, h.z > 0.f ? a2 : 0.f, h.w > 0.f ? a3 : 0.f);
        } else {
            const float bo = bias[o];
            a0 += bo; a1 += bo; a2 += bo; a3 += bo;
            *dst = make_float4(fmaxf(a0, 0.f), fmaxf(a1, 0.f), fmaxf(a2, 0.f), fmaxf(a3, 0.f));
        }
    }
}

#define TT_LDS_BYTES (TT_ACT * TT_P * sizeof(float))

__global__ __launch_bounds__(256) void tt_train_kernel(TtStreams s, const float *__restrict__ W, const float *__restrict__ Wb,
                                                       const float *__restrict__ desc_prev, const float *__restrict__ desc,
                                                       const float *__restrict__ target, const float *__restrict__ scale,
                                                       const int *__restrict__ pair_offset, float *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float tt_smem[];
    __shared__ float s_dz[TT_P];
    float *X0 = tt_smem, *H1 = X0 + 141 * TT_P, *H2 = H1 + 564 * TT_P, *H3 = H2 + 282 * TT_P, *H4 = H3 + 70 * TT_P;
    const int b = blockIdx.x, t = threadIdx.x, K = s.K;
    const int off = pair_offset[b];
    int m, n;
    const int pairs = tt_block(s, b, &m, &n);
    if (off < 0 || pairs == 0) return;
    const float *W1 = W, *b1 = W1 + 141 * 564, *W2 = b1 + 564, *b2 = W2 + 564 * 282, *W3 = b2 + 282, *b3 = W3 + 282 * 70;
    const float *W4 = b3 + 70, *b4 = W4 + 70 * 35, *W5 = b4 + 35, *b5 = W5 + 35;
    const float *V2 = Wb + 141 * 564, *V3 = V2 + 564 * 282, *V4 = V3 + 282 * 70;      // (Cout, Cin) images of layers 2, 3, 4
    const float *dc = desc + (size_t)b * K * RTK_DESC, *dp = desc_prev + (size_t)b * K * RTK_DESC;
    const float gm = scale[b] / (float)pairs;                      // the mean's share of the upstream gradient
    for (int q0 = blockIdx.y * TT_P; q0 < pairs; q0 += gridDim.y * TT_P) {
        for (int e = t; e < RTK_DESC * TT_P; e += 256) {
            const int c = e / TT_P, q = q0 + e % TT_P;
            float v = 0.f;
            if (q < pairs) {
                const int i = q / n, j = q % n;
                v = dc[(size_t)j * RTK_DESC + c] - dp[(size_t)i * RTK_DESC + c];     // curr_j - prev_i
            }
            X0[e] = v;
        }
        __syncthreads();
        tt_layer<false>(X0, H1, W1, b1, 141, 564);
        __syncthreads();
        tt_layer<false>(H1, H2, W2, b2, 564, 282);
        __syncthreads();
        tt_layer<false>(H2, H3, W3, b3, 282, 70);
        __syncthreads();
        tt_layer<false>(H3, H4, W4, b4, 70, 35);
        __syncthreads();
        const int live = pairs - q0 < TT_P ? pairs - q0 : TT_P;
        float *rows = ws + (size_t)(off + q0) * TT_ROW;
        for (int e = t; e < TT_ACT * live; e += 256) {
            const int q = e / TT_ACT, c = e % TT_ACT;
            rows[(size_t)q * TT_ROW + c] = tt_smem[c * TT_P + q];
        }
        if (t < TT_P) {
            float dz = 0.f;
            if (t < live) {
                float z = 0.f;
                for (int c = 0; c < 35; ++c) z = __fmaf_rn(H4[c * TT_P + t], W5[c], z);
                z += b5[0];
                const float a = 1.f / (1.f + expf(-z));
                const int q = q0 + t, i = q / n, j = q % n;
                const float tg = target[((size_t)b * K + i) * K + j];
                // F.binary_cross_entropy's backward, then sigmoid's
                const float gb = gm * (a - tg) / fmaxf((1.f - a) * a, 1e-12f);
                dz = gb * (1.f - a) * a;
                rows[(size_t)t * TT_ROW + TT_D5] = dz;
                rows[(size_t)t * TT_ROW + TT_TERM] = tt_bce(a, tg);
            }
            s_dz[t] = dz;
        }
        __syncthreads();
        for (int e = t; e < 35 * TT_P; e += 256) {                  // layer 5 has one output: d4 = W5 d5 under a4's mask
            const int c = e / TT_P, q = e % TT_P;
            H4[e] = H4[e] > 0.f ? W5[c] * s_dz[q] : 0.f;
        }
        __syncthreads();
        tt_layer<true>(H4, H3, V4, nullptr, 35, 70);
        __syncthreads();
        tt_layer<true>(H3, H2, V3, nullptr, 70, 282);
        __syncthreads();
        tt_layer<true>(H2, H1, V2, nullptr, 282, 564);
        __syncthreads();
        for (int e = t; e < TT_DELTA * live; e += 256) {
            const int q = e / TT_DELTA, c = e % TT_DELTA;
            rows[(size_t)q * TT_ROW + TT_D1 + c] = H1[c * TT_P + q];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// Launch 3: workgroup (b, y).  y == 0 also forms loss[b]: thread t adds the terms of the rows t, t + 256, ..., then the tree.
// Current objects j = y, y + G, ...: s = the sum over i = 0 .. m-1 of d1 of pair (i, j), in that order in blocks of 8 (the first
// layer is linear in its input: one product with W1 for the sum instead of one per pair), then d_desc[b][j][c] = the sum over o of
// W1[o][c] s[o], fmaf chains over blocks of TT_BLOCK added in order.  Rows of d_desc past the live block, and of streams that sit the term out, are zeros.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tt_reduce_kernel(TtStreams s, const float *__restrict__ Wb, const int *__restrict__ pair_offset,
                                                        const float *__restrict__ ws, float *__restrict__ loss,
                                                        float *__restrict__ d_desc) {
    __shared__ float sum1[564];
    __shared__ float red[256];
    const int b = blockIdx.x, t = threadIdx.x, K = s.K;
    const int off = pair_offset[b];
    int m, n;
    int pairs = tt_block(s, b, &m, &n);
    if (off < 0) pairs = 0;
    const float *rows = ws + (size_t)(off < 0 ? 0 : off) * TT_ROW;
    if (blockIdx.y == 0) {
        float acc = 0.f;
        for (int q = t; q < pairs; q += 256) acc += rows[(size_t)q * TT_ROW + TT_TERM];
        const float sum = tt_block_sum(acc, red);
        if (t == 0) loss[b] = pairs ? sum / (float)pairs : 0.f;
    }
    float *dd = d_desc + (size_t)b * K * RTK_DESC;
    for (int j = blockIdx.y; j < K; j += gridDim.y) {
        if (pairs == 0 || j >= n) {
            for (int c = t; c < RTK_DESC; c += 256) dd[(size_t)j * RTK_DESC + c] = 0.f;
            continue;
        }
        for (int o = t; o < 564; o += 256) {
            float acc = 0.f;
            for (int i0 = 0; i0 < m; i0 += 8) {
                float part = 0.f;
                for (int i = i0; i < m && i < i0 + 8; ++i) part += rows[(size_t)(i * n + j) * TT_ROW + TT_D1 + o];
                acc += part;
            }
            sum1[o] = acc;
        }
        __syncthreads();
        if (t < RTK_DESC) {
            float acc = 0.f;
            for (int o0 = 0; o0 < 564; o0 += TT_BLOCK) {
                float part = 0.f;
                for (int o = o0; o < 564 && o < o0 + TT_BLOCK; ++o) part = __fmaf_rn(Wb[(size_t)o * 141 + t], sum1[o], part);
                acc += part;
            }
            dd[(size_t)j * RTK_DESC + t] = acc;
        }
        __syncthreads();
    }
}

static int tt_chunks(int max_pairs) { return rtk_divup(max_pairs, RTK_AFF_TRAIN_CHUNK); }
static long tt_workspace_floats(int max_pairs) { return (long)max_pairs * TT_ROW + (long)tt_chunks(max_pairs) * TT_NW; }

extern "C" int rtk_affinity_train(int B, int K, const float *weights, const float *weights_bwd, const float *desc_prev,
                                  const int *prev_count, const unsigned char *reset, const unsigned char *active, const float *desc,
                                  const int *num_objects, const float *aff, const float *aff_target, const unsigned char *aff_defined,
                                  const float *scale, int max_pairs, float *loss, float *d_desc, int *pair_offset, int *flags,
                                  float *workspace, long workspace_floats, rtk_stream_t stream) {
    RTK_REQUIRE(B > 0 && B <= 65535 && prev_count && num_objects && aff_target && aff_defined && loss && pair_offset && flags,
                "affinity_train: bad arguments");
    RTK_REQUIRE(K >= 1 && K <= rtk_track_max_objects(), "affinity_train: K=%d object slots outside [1, %d]", K, rtk_track_max_objects());
    RTK_REQUIRE(max_pairs >= 1 && max_pairs <= (1 << 20), "affinity_train: max_pairs=%d outside [1, %d]", max_pairs, 1 << 20);
    const TtStreams s = {K, prev_count, num_objects, reset, active, aff_defined};
    hipStream_t st = (hipStream_t)stream;
    if (!scale) {
        RTK_REQUIRE(aff, "affinity_train: the loss alone (scale == NULL) is read off aff, which is NULL");
        tt_prefix_kernel<<<1, 256, 0, st>>>(B, s, max_pairs, pair_offset, flags);
        RTK_CHECK_LAUNCH("affinity_train (rows)");
        tt_loss_kernel<<<B, 256, 0, st>>>(s, pair_offset, aff, aff_target, loss);
        RTK_CHECK_LAUNCH("affinity_train (loss)");
        return RTK_OK;
    }
    RTK_REQUIRE(weights && weights_bwd && desc_prev && desc && d_desc && workspace, "affinity_train: bad arguments (backward)");
    RTK_REQUIRE(workspace_floats >= tt_workspace_floats(max_pairs), "affinity_train: max_pairs=%d needs a workspace of %ld floats (got %ld)",
                max_pairs, tt_workspace_floats(max_pairs), workspace_floats);
    tt_prefix_kernel<<<1, 256, 0, st>>>(B, s, max_pairs, pair_offset, flags);
    RTK_CHECK_LAUNCH("affinity_train (rows)");
    // tiles per stream in flight as in rtk_affinity_pairs: the device filled at small B, few idle workgroups at large B
    int g = rtk_divup(2048, B), tiles = rtk_divup((long)K * K, TT_P);
    g = g < 4 ? 4 : (g > tiles ? tiles : g);
    (void)hipFuncSetAttribute((const void *)tt_train_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TT_LDS_BYTES);
    tt_train_kernel<<<dim3(B, g), 256, TT_LDS_BYTES, st>>>(s, weights, weights_bwd, desc_prev, desc, aff_target, scale, pair_offset, workspace);
    RTK_CHECK_LAUNCH("affinity_train");
    tt_reduce_kernel<<<dim3(B, K < 16 ? K : 16), 256, 0, st>>>(s, weights_bwd, pair_offset, workspace, loss, d_desc);
    RTK_CHECK_LAUNCH("affinity_train (reduce)");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_affinity_wgrad.  Workgroup (tile, chunk): a 64 (input channel) x 64 (output channel) block of one layer's dW^T over the rows
// [chunk * RTK_AFF_TRAIN_CHUNK, ...) in row order, 4 x 4 outputs per thread: an fmaf chain per tile of 16 rows, the tiles added in
// order in groups of 8, the groups in order; the bias gradient (a compensated sum of the same rows in row order: the last layer's is
// ONE number, the sum of every row's d5 with both signs, and a plain sum left it at the mercy of its cancellation) rides with the
// blocks of input-channel tile 0.  Then element e of the image = the chunks' partials in chunk order, compensated alike.
// Layers' 64 x 64 blocks: 3x9, 9x5, 5x2, 2x1, 1x1 = 85.
// ------------------------------------------------------------------------------------------------
#define TW_TILES 85

// sum += x with the rounding error of the addition carried in comp (Kahan): plain fp32 operations in a fixed order; the file is
// built with -ffp-contract=off and without fast-math, so they stay as written
__device__ __forceinline__ void tt_kahan_add(float &sum, float &comp, float x) {
    const float y = x - comp, t = sum + y;
    comp = (t - sum) - y;
    sum = t;
}

__global__ __launch_bounds__(256) void tt_wgrad_kernel(int B, const int *__restrict__ pair_offset, const float *__restrict__ ws,
                                                       float *__restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float As[TT_P][64];
    __shared__ __attribute__((aligned(16))) float Ds[TT_P][64];
    const int total = pair_offset[B], t = threadIdx.x;
    const int p0 = blockIdx.y * RTK_AFF_TRAIN_CHUNK;
    if (p0 >= total) return;
    const int p1 = p0 + RTK_AFF_TRAIN_CHUNK < total ? p0 + RTK_AFF_TRAIN_CHUNK : total;
    const int cins[5] = {141, 564, 282, 70, 35}, couts[5] = {564, 282, 70, 35, 1};
    const int first[6] = {0, 27, 72, 82, 84, 85}, otiles[5] = {9, 5, 2, 1, 1};
    int L = 0;
    while ((int)blockIdx.x >= first[L + 1]) ++L;
    int aoff = 0, doff = TT_D1, woff = 0;
    for (int l = 0; l < L; ++l) {
        aoff += cins[l];
        doff += couts[l];
        woff += cins[l] * couts[l] + couts[l];
    }
    const int cin = cins[L], cout = couts[L];
    const int tile = blockIdx.x - first[L], c0 = (tile / otiles[L]) * 64, o0 = (tile % otiles[L]) * 64;
    const int tx = t & 15, ty = t >> 4;
    float acc[4][4], mid[4][4], top[4][4];      // a tile of 16 rows | 8 tiles | the chunk
    float bsum[4], bcomp[4];                    // the bias gradient: a compensated (Kahan) sum over the chunk's rows
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bsum[i] = bcomp[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) mid[i][j] = top[i][j] = 0.f;
    }
    const int lc = t & 63, lr = t >> 6;
    for (int p = p0; p < p1; p += TT_P) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = lr + 4 * k, pp = p + r;
            const float *row = ws + (size_t)pp * TT_ROW;
            As[r][lc] = (pp < p1 && c0 + lc < cin) ? row[aoff + c0 + lc] : 0.f;
            Ds[r][lc] = (pp < p1 && o0 + lc < cout) ? row[doff + o0 + lc] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < TT_P; ++r) {
            const float4 a4 = *reinterpret_cast<const float4 *>(&As[r][ty * 4]);
            const float4 d4 = *reinterpret_cast<const float4 *>(&Ds[r][tx * 4]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __fmaf_rn(a[i], d[j], acc[i][j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) tt_kahan_add(bsum[j], bcomp[j], d[j]);
        }
        __syncthreads();
        const bool flush = ((p - p0) / TT_P) % 8 == 7 || p + TT_P >= p1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mid[i][j] += acc[i][j];
                if (flush) { top[i][j] += mid[i][j]; mid[i][j] = 0.f; }
            }
        }
    }
    float *out = partials + (size_t)blockIdx.y * TT_NW + woff;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = o0 + tx * 4 + j;
            if (c < cin && o < cout) out[(size_t)c * cout + o] = top[i][j];
        }
    }
    if (c0 == 0 && ty == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = o0 + tx * 4 + j;
            if (o < cout) out[(size_t)cin * cout + o] = bsum[j];
        }
    }
}

__global__ __launch_bounds__(256) void tt_wgrad_sum_kernel(int B, const int *__restrict__ pair_offset, const float *__restrict__ partials,
                                                           float *__restrict__ d_weights) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= TT_NW) return;
    const int chunks = (pair_offset[B] + RTK_AFF_TRAIN_CHUNK - 1) / RTK_AFF_TRAIN_CHUNK;
    float acc = 0.f, comp = 0.f;
    for (int c = 0; c < chunks; ++c) tt_kahan_add(acc, comp, partials[(size_t)c * TT_NW + e]);
    d_weights[e] = acc;
}

extern "C" int rtk_affinity_wgrad(int B, int max_pairs, const int *pair_offset, float *workspace, long workspace_floats,
                                  float *d_weights, rtk_stream_t stream) {
    RTK_REQUIRE(B > 0 && B <= 65535 && pair_offset && workspace && d_weights, "affinity_wgrad: bad arguments");
    RTK_REQUIRE(max_pairs >= 1 && max_pairs <= (1 << 20), "affinity_wgrad: max_pairs=%d outside [1, %d]", max_pairs, 1 << 20);
    RTK_REQUIRE(workspace_floats >= tt_workspace_floats(max_pairs), "affinity_wgrad: max_pairs=%d needs a workspace of %ld floats (got %ld)",
                max_pairs, tt_workspace_floats(max_pairs), workspace_floats);
    float *partials = workspace + (size_t)max_pairs * TT_ROW;
    tt_wgrad_kernel<<<dim3(TW_TILES, tt_chunks(max_pairs)), 256, 0, (hipStream_t)stream>>>(B, pair_offset, workspace, partials);
    RTK_CHECK_LAUNCH("affinity_wgrad");
    tt_wgrad_sum_kernel<<<rtk_divup(TT_NW, 256), 256, 0, (hipStream_t)stream>>>(B, pair_offset, partials, d_weights);
    RTK_CHECK_LAUNCH("affinity_wgrad (sum)");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_object_descriptors_bwd.  Launch 1, (stream, object-slot) workgroups as in rtk_object_descriptors: the object's members are
// compacted in column order per chunk of 256 columns; thread c < 128 keeps the first member that attains the maximum of prop channel
// c (strict > while scanning upwards).  Launch 2, one thread per point: plain stores of every element of d_flow and d_prop.
// ------------------------------------------------------------------------------------------------
#define TD_G 16

__global__ __launch_bounds__(256) void tt_desc_argmax_kernel(const rtk_track_frame_t fr, int K, const int *__restrict__ obj,
                                                             const int *__restrict__ num_objects, int *__restrict__ arg,
                                                             int *__restrict__ size) {
    __shared__ int s_list[256], s_wave[4];
    const int b = blockIdx.x, t = threadIdx.x;
    if (!stream_active(fr, b)) return;
    const int n = stream_points(fr, b), nobj = count_clamp(num_objects[b], K);
    const int *obj_b = obj + (size_t)b * fr.N;
    for (int k = blockIdx.y; k < nobj; k += gridDim.y) {
        float best = 0.f;
        int at = -1, cnt = 0;
        for (int base = 0; base < n; base += 256) {
            const int p = base + t;
            const bool mine = p < n && obj_b[p] == k;
            int c;
            const int slot = ordered_slot(mine, s_wave, &c);
            if (mine) s_list[slot] = p;
            __syncthreads();
            if (t < 128) {
                for (int q = 0; q < c; ++q) {
                    const float v = bcn_at(fr.prop, b, t, s_list[q]);
                    if (at < 0 || v > best) { best = v; at = s_list[q]; }
                }
            }
            cnt += c;
            __syncthreads();
        }
        if (t < 128) arg[((size_t)b * K + k) * 128 + t] = at;
        if (t == 128) size[(size_t)b * K + k] = cnt;
    }
}

__global__ __launch_bounds__(256) void tt_desc_points_kernel(const rtk_track_frame_t fr, int K, const int *__restrict__ obj,
                                                             const int *__restrict__ num_objects, const float *__restrict__ d_desc,
                                                             const int *__restrict__ arg, const int *__restrict__ size,
                                                             float *__restrict__ d_flow, float *__restrict__ d_prop) {
    const int b = blockIdx.x, p = blockIdx.y * 256 + threadIdx.x, N = fr.N;
    if (p >= N) return;
    int k = -1;
    if (stream_active(fr, b) && p < stream_points(fr, b)) {
        k = obj[(size_t)b * N + p];
        if (k >= count_clamp(num_objects[b], K)) k = -1;
    }
    const float *dk = d_desc + ((size_t)b * K + (k < 0 ? 0 : k)) * RTK_DESC;
    const int *ak = arg + ((size_t)b * K + (k < 0 ? 0 : k)) * 128;
    const float cnt = k < 0 ? 1.f : (float)size[(size_t)b * K + k];
    for (int c = 0; c < 3; ++c) d_flow[((size_t)b * 3 + c) * N + p] = k < 0 ? 0.f : dk[134 + c] / cnt;
    for (int c = 0; c < 128; ++c) d_prop[((size_t)b * 128 + c) * N + p] = (k >= 0 && ak[c] == p) ? dk[6 + c] : 0.f;
}

extern "C" int rtk_object_descriptors_bwd(const rtk_track_frame_t *frame, int K, const int *obj, const int *num_objects,
                                          const float *d_desc, float *d_flow, float *d_prop, int *arg_ws, rtk_stream_t stream) {
    RTK_REQUIRE(frame && frame->B > 0 && frame->B <= 65535 && frame->N > 0 && frame->prop.ptr && obj && num_objects && d_desc && d_flow &&
                d_prop && arg_ws, "object_descriptors_bwd: bad arguments");
    RTK_REQUIRE(K >= 1 && K <= rtk_track_max_objects(), "object_descriptors_bwd: K=%d object slots outside [1, %d]", K,
                rtk_track_max_objects());
    const int B = frame->B, N = frame->N;
    RTK_REQUIRE(rtk_divup(N, 256) <= 65535, "object_descriptors_bwd: N=%d points", N);
    int *arg = arg_ws, *size = arg_ws + (size_t)B * K * 128;
    tt_desc_argmax_kernel<<<dim3(B, K < TD_G ? K : TD_G), 256, 0, (hipStream_t)stream>>>(*frame, K, obj, num_objects, arg, size);
    RTK_CHECK_LAUNCH("object_descriptors_bwd (arg-max)");
    tt_desc_points_kernel<<<dim3(B, rtk_divup(N, 256)), 256, 0, (hipStream_t)stream>>>(*frame, K, obj, num_objects, d_desc, arg, size,
                                                                                      d_flow, d_prop);
    RTK_CHECK_LAUNCH("object_descriptors_bwd");
    return RTK_OK;
}
