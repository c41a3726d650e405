// fused_pointwise.hip -- rtk_pointwise_mlp: a chain of up to four 1x1-conv (+folded BN, +activation)
// layers applied per point, with the input vector assembled on the fly from
//   [three-NN inverse-distance interpolation of a coarser level]  ||  skip features  ||  per-sample
//   (broadcast) features,
// i.e. the reference's PointnetFPModule.forward (lib/pointnet2_modules.py:140-158), the nn.Linear
// bottlenecks of PNHead (model_utils.py:414-418) and the Flow/Cls predictors (model_utils.py:308-357),
// each as ONE kernel instead of 4-12 framework ops with materialised intermediates.
//
// Structure: see fused_common.h.  A wave owns 16 points; all layers run back to back on the MFMA
// pipe with activations held in registers; HBM sees each input row once and each output row once.
//
// Three entry points: rtk_pointwise_mlp (the chain), rtk_pointwise_mlp_tap (the encoder's last layer and the cost volume's projection
// of its output on the same tile) and rtk_pointwise_mlp_pair (two chains on the same rows).  They share one host launch layer -- the
// pw_* validators and pw_grid, after the first kernel -- and each adds the fields, the instance and the launch that only it has.
#include <string.h>

#include "rtk_common.h"
#include "fused_common.h"
#include "rtk_fused.h"

struct PwParams {
    int rows, rows_per_sample;
    rtk_interp_t interp;
    int nsrc;
    rtk_src_t src[RTK_MAX_SRC];
    const float *sample_bias;
    rtk_layer_t layer[RTK_MAX_LAYERS];
    float *out;
    int out_pitch, out_channels, out_cm;
    const int *row_nuniq;
    float *colmax;
    int gx;                 // > 0: XCD-aware 1-D grid (rtk_decode_block)
};

template <int V>
__device__ __forceinline__ void init_bias(f4 (&acc)[V], const float *__restrict__ bias, int g) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = bias_frag(bias, v, g);
}
template <int V>
__device__ __forceinline__ void init_zero(f4 (&acc)[V]) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = f4_zero();
}
// split layers: y = acc c + b, c = this lane's 2^-(kw + kx)
template <int V>
__device__ __forceinline__ void scale_bias(f4 (&acc)[V], float c, const float *__restrict__ bias, int g) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = __builtin_elementwise_fma(acc[v], (f4){c, c, c, c}, bias_frag(bias, v, g));
}

// One layer of the chain: fp32-input MFMA with the bias in the accumulators, or (SPLIT) the fp16 split path -- the lane's power-of-two
// scale from its position's largest input, zero accumulators, scale and bias in one fma afterwards.
template <bool SPLIT, int U, int V, int FBASE, class WS>
__device__ __forceinline__ void pw_layer(WS &ws, const f4 (&h)[U], f4 (&acc)[V], const rtk_layer_t &L, int g, const float *sample_bias, bool first) {
    if constexpr (SPLIT) {
        const LaneScale sc = lane_scale16(h);
        init_zero<V>(acc);
        if (first) ws.next_if_deferred();
        mlp_layer_ws_split<U, V, FBASE>(ws, h, sc.s, acc);
        scale_bias<V>(acc, sc.inv * L.inv_scale, L.bias, g);
    } else {
        init_bias<V>(acc, L.bias, g);
        if (first) ws.next_if_deferred();
        mlp_layer_ws<U, V, FBASE>(ws, h, acc);
    }
    if (sample_bias) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += bias_frag(sample_bias, v, g);
    }
    apply_act<V>(acc, L.act);
}

template <int V>
__device__ __forceinline__ void store_tile(const PwParams &P, const f4 (&acc)[V], int p, int b, int g, bool valid) {
    if (P.colmax) {
        // per-sample column maximum: DPP max over the tile's 16 rows, then one atomic max per channel on the float bits
        // (outputs are >= 0 after ReLU, so unsigned order == float order and the zero-initialised buffer is the identity)
        unsigned *cm = reinterpret_cast<unsigned *>(P.colmax) + (size_t)b * 16 * V + 4 * g;
        const bool lead = (threadIdx.x & 15) == 0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            f4 m = valid ? acc[v] : f4_zero();
            row_max16_f4(m);
            if (lead) {
                atomicMax(cm + 16 * v + 0, __float_as_uint(m.x));
                atomicMax(cm + 16 * v + 1, __float_as_uint(m.y));
                atomicMax(cm + 16 * v + 2, __float_as_uint(m.z));
                atomicMax(cm + 16 * v + 3, __float_as_uint(m.w));
            }
        }
    }
    if (!valid) return;
    if (!P.out_cm) {
        float *o = P.out + (size_t)p * P.out_pitch;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = 16 * v + 4 * g;
            if (c + 3 < P.out_channels) {
                *reinterpret_cast<f4 *>(o + c) = acc[v];
            } else {
                if (c + 0 < P.out_channels) o[c + 0] = acc[v].x;
                if (c + 1 < P.out_channels) o[c + 1] = acc[v].y;
                if (c + 2 < P.out_channels) o[c + 2] = acc[v].z;
            }
        }
    } else {
        const int n = P.rows_per_sample;
        float *o = P.out + (size_t)b * P.out_channels * n + (p - b * n);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = 16 * v + 4 * g;
            if (c + 0 < P.out_channels) o[(size_t)(c + 0) * n] = acc[v].x;
            if (c + 1 < P.out_channels) o[(size_t)(c + 1) * n] = acc[v].y;
            if (c + 2 < P.out_channels) o[(size_t)(c + 2) * n] = acc[v].z;
            if (c + 3 < P.out_channels) o[(size_t)(c + 3) * n] = acc[v].w;
        }
    }
}

// slots u < nslots of this lane's input: the three-NN inverse-distance interpolation of row p (lib/pointnet2_modules.py:141-146)
template <int U>
__device__ __forceinline__ void load_interp(const PwParams &P, int p, int b, int g, int nslots, f4 (&h)[U]) {
    const int *idp = P.interp.idx + (size_t)p * 3;
    int id[3] = {idp[0], idp[1], idp[2]};
    if (P.interp.nuniq) {       // known rows beyond the sample's unique count are copies of its row 0
        const int e = P.interp.nuniq[b];
        id[0] = id[0] < e ? id[0] : 0; id[1] = id[1] < e ? id[1] : 0; id[2] = id[2] < e ? id[2] : 0;
    }
    const float *d2 = P.interp.dist2 + (size_t)p * 3;
    const float r0 = __fdiv_rn(1.0f, __fadd_rn(__fsqrt_rn(d2[0]), 1e-8f));
    const float r1 = __fdiv_rn(1.0f, __fadd_rn(__fsqrt_rn(d2[1]), 1e-8f));
    const float r2 = __fdiv_rn(1.0f, __fadd_rn(__fsqrt_rn(d2[2]), 1e-8f));
    const float norm = __fadd_rn(__fadd_rn(r0, r1), r2);
    const float w0 = __fdiv_rn(r0, norm), w1 = __fdiv_rn(r1, norm), w2 = __fdiv_rn(r2, norm);
    const float *k0 = P.interp.known_feats + ((size_t)b * P.interp.m + id[0]) * P.interp.pitch;
    const float *k1 = P.interp.known_feats + ((size_t)b * P.interp.m + id[1]) * P.interp.pitch;
    const float *k2 = P.interp.known_feats + ((size_t)b * P.interp.m + id[2]) * P.interp.pitch;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (u < nslots) {
            // unconditional loads (lanes past the last channel re-read channel 0 and discard): a load under a per-lane
            // condition is a basic block of its own and the compiler waits for it before issuing the next one
            const int c = 16 * u + 4 * g;
            const bool ok = c < P.interp.channels;
            const int cc = ok ? c : 0;
            const f4 a0 = *reinterpret_cast<const f4 *>(k0 + cc);
            const f4 a1 = *reinterpret_cast<const f4 *>(k1 + cc);
            const f4 a2 = *reinterpret_cast<const f4 *>(k2 + cc);
            // interpolate_gpu.cu:168  w0*p0 + w1*p1 + w2*p2  (nvcc: fma(w2,p2,fma(w1,p1,w0*p0)))
            f4 v;
            v.x = __fmaf_rn(w2, a2.x, __fmaf_rn(w1, a1.x, __fmul_rn(w0, a0.x)));
            v.y = __fmaf_rn(w2, a2.y, __fmaf_rn(w1, a1.y, __fmul_rn(w0, a0.y)));
            v.z = __fmaf_rn(w2, a2.z, __fmaf_rn(w1, a1.z, __fmul_rn(w0, a0.z)));
            v.w = __fmaf_rn(w2, a2.w, __fmaf_rn(w1, a1.w, __fmul_rn(w0, a0.w)));
            h[u] = ok ? v : f4_zero();
        }
    }
}

#define PW_NW 4    // waves per workgroup
// A workgroup steps over groups of PW_NW * 16 rows, and load_interp reads the three-NN rows of the whole last group -- the rows past
// row_nuniq too, clamped to the sample, masked only at the store.  The three-NN kernels write whole multiples of this group
// (ops_pointnet2.hip asserts KV_QPW % RTK_INTERP_ROW_GROUP == 0), so those rows hold in-range indices even in an unfilled workspace.
static_assert(PW_NW * 16 == RTK_INTERP_ROW_GROUP, "PW_NW: the row group the three-NN tables are written for");
#ifndef PW_WGS_TARGET
#define PW_WGS_TARGET 256      // workgroups per launch: about one per CU, the rest is looped.  Round 6, same box, alternating (ab_knobs.py):
                               // 512 (rounds 2-5): base; 448 / 384 / 320: +0.4 ... +0.5 %; 256: +0.9 % (B=64, N=256), +1.0 % (B=32, N=1024), +-0.1 %
                               // (B=32 / 8 / 1, N=256); 192: -0.5 %; 128: -0.1 %
#endif
#ifndef PW_F
#define PW_F 16    // fragments (KiB) per half of the LDS weight double buffer (16 vs 32: same kernel speed, 1 % more end-to-end
                   // throughput with two batches in flight -- smaller footprints co-reside, tools/experiments/exp_pwf.sh)
#endif

// SPLIT: the layers on the fp16 matrix pipe (two pieces per operand, three products per fp32 product, a power-of-two scale per weight
// matrix and per position: fused_common.h, split_mfma.h): same tile, registers and stream, the blob holds split images.
template <int U, int V1, int V2, int V3, int V4, bool INTERP, bool SPLIT>
__global__ __launch_bounds__(64 * PW_NW, 2) void pointwise_mlp_kernel(const PwParams P) {
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * PW_F * 64];
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int wave_in_wg = threadIdx.x >> 6;
    // A workgroup owns one sample and strides over its 64-row groups (one 16-row tile per wave).  No division inside the
    // loop; a tile never straddles two samples; workgroups whose groups are all duplicate rows (>= row_nuniq[b]) exit
    // before touching the weight stream.  The trip count is uniform over the workgroup, which the barriers inside the
    // weight stream require.
    int b, bx, nbx;
    rtk_decode_block(P.gx, b, bx, nbx);
    const int rps = P.rows_per_sample;
    const int live_rows = P.row_nuniq ? min(rps, __builtin_amdgcn_readfirstlane(P.row_nuniq[b])) : rps;
    const int live_groups = (live_rows + PW_NW * 16 - 1) / (PW_NW * 16);
    if (bx >= live_groups) return;
    constexpr int F1 = SPLIT ? split16_nf(U, V1) : U * V1, F2 = SPLIT ? split16_nf(V1, V2) : V1 * V2,
                  F3 = SPLIT ? split16_nf(V2, V3) : V2 * V3, F4 = SPLIT ? split16_nf(V3, V4) : V3 * V4;
    constexpr int NF = F1 + F2 + F3 + F4;
    // A blob of several chunks: the stream is entered at the top of every tile AFTER the tile's input loads have been issued (the
    // wrap to chunk 0 -- for the first tile: the arrival of chunk 0 -- and those loads then share one round trip; most workgroups
    // have exactly one tile, and the two round trips in a row were 1-2 us of a 10-25 us launch).
    WStream<PW_NW, PW_F, NF> ws;
    if constexpr (NF > PW_F) ws.start_deferred(reinterpret_cast<const f4 *>(P.layer[0].w_packed), s_w, wave_in_wg, lane);
    else ws.start(reinterpret_cast<const f4 *>(P.layer[0].w_packed), s_w, wave_in_wg, lane);

    // 16-channel slot where each segment starts (wave-uniform)
    int ustart[RTK_MAX_SRC + 1];
    ustart[0] = INTERP ? (P.interp.channels + 15) >> 4 : 0;
#pragma unroll
    for (int s = 0; s < RTK_MAX_SRC; ++s) ustart[s + 1] = ustart[s] + (s < P.nsrc ? (P.src[s].channels + 15) >> 4 : 0);
    const int uend = ustart[RTK_MAX_SRC];

    for (int G = bx; G < live_groups; G += nbx) {
        asm volatile("" ::: "memory");   // keep loop-invariant loads/addresses inside the loop (registers are the scarce resource)
        const int r = G * (PW_NW * 16) + wave_in_wg * 16 + j;           // row within the sample
        const bool valid = r < live_rows;
        const int p = b * rps + (r < rps ? r : rps - 1);                  // global row (clamped: out-of-range lanes compute garbage, never stored)

        f4 h[U];
        // ---- segment 0 (optional): three-NN interpolation, lib/pointnet2_modules.py:141-146 -------------
        if (INTERP) load_interp<U>(P, p, b, g, ustart[0], h);
        // ---- plain / per-sample segments --------------------------------------------------------------
        // per-lane row base of every source (row = point, or sample for broadcast sources), then one
        // load per 16-channel slot from the source that owns it (selection is wave-uniform)
        const float *rowp[RTK_MAX_SRC];
        const float *dummy = reinterpret_cast<const float *>(P.layer[0].w_packed);      // any readable 16-byte aligned address
#pragma unroll
        for (int q = 0; q < RTK_MAX_SRC; ++q)
            rowp[q] = q < P.nsrc ? P.src[q].ptr + (P.src[q].per_sample ? (size_t)b : (size_t)p) * P.src[q].pitch + 4 * g : nullptr;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!INTERP || u >= ustart[0]) {
                const float *rp = rowp[0];
                int us = ustart[0], ch = P.src[0].channels;
#pragma unroll
                for (int q = 1; q < RTK_MAX_SRC; ++q)
                    if (q < P.nsrc && u >= ustart[q]) { rp = rowp[q]; us = ustart[q]; ch = P.src[q].channels; }
                const int c = 16 * (u - us);
                const bool ok = u < uend && c + 4 * g < ch;
                const f4 v = *reinterpret_cast<const f4 *>(ok ? rp + c : dummy);       // unconditional load, see above
                h[u] = ok ? v : f4_zero();
            }
        }

        // ---- layer chain ------------------------------------------------------------------------------
        // (the first layer enters the weight stream: chunk 0's request has been travelling with the loads above)
        f4 a1[V1];
        pw_layer<SPLIT, U, V1, 0>(ws, h, a1, P.layer[0], g, P.sample_bias ? P.sample_bias + (size_t)b * 16 * V1 : nullptr, true);
        if constexpr (V2 == 0) {
            store_tile<V1>(P, a1, p, b, g, valid);
        } else {
            f4 a2[V2];
            pw_layer<SPLIT, V1, V2, F1>(ws, a1, a2, P.layer[1], g, nullptr, false);
            if constexpr (V3 == 0) {
                store_tile<V2>(P, a2, p, b, g, valid);
            } else {
                f4 a3[V3];
                pw_layer<SPLIT, V2, V3, F1 + F2>(ws, a2, a3, P.layer[2], g, nullptr, false);
                if constexpr (V4 == 0) {
                    store_tile<V3>(P, a3, p, b, g, valid);
                } else {
                    f4 a4[V4];
                    pw_layer<SPLIT, V3, V4, F1 + F2 + F3>(ws, a3, a4, P.layer[3], g, nullptr, false);
                    store_tile<V4>(P, a4, p, b, g, valid);
                }
            }
        }
    }
    ws.finish();
}

// ---- the host launch layer of the three entry points --------------------------------------------------------------------------
// `who` is the entry point's name, for the messages.  Every helper returns a count >= 0 or, after rtk_set_error, RTK_ERR_INVALID.
static int pw_rows(const char *who, PwParams &P, int rows, int rows_per_sample) {
    RTK_REQUIRE(rows > 0 && rows_per_sample > 0 && rows % rows_per_sample == 0 && rows / rows_per_sample <= 65535,
                "%s: bad row counts (%d, %d)", who, rows, rows_per_sample);
    P.rows = rows; P.rows_per_sample = rows_per_sample;
    return RTK_OK;
}

// P.src, P.nsrc -> the 16-channel input slots the sources take
static int pw_sources(const char *who, PwParams &P, int nsrc, const rtk_src_t *srcs) {
    RTK_REQUIRE(nsrc >= 0 && nsrc <= RTK_MAX_SRC && (nsrc == 0 || srcs), "%s: nsrc=%d", who, nsrc);
    int U = 0;
    for (int s = 0; s < nsrc; ++s) {
        RTK_REQUIRE(srcs[s].ptr && srcs[s].pitch % 4 == 0 && srcs[s].channels > 0 && srcs[s].pitch >= ((srcs[s].channels + 3) / 4) * 4,
                    "%s: bad source %d (pitch %d, channels %d)", who, s, srcs[s].pitch, srcs[s].channels);
        P.src[s] = srcs[s];
        U += (srcs[s].channels + 15) / 16;
    }
    P.nsrc = nsrc;
    return U;
}

// P.interp -> the slots the interpolation segment takes, which must be `slots` of them unless that is 0
static int pw_interp(const char *who, PwParams &P, const rtk_interp_t *interp, int slots) {
    RTK_REQUIRE(interp && interp->known_feats && interp->idx && interp->dist2 && interp->pitch % 4 == 0 && interp->channels % 4 == 0 &&
                (slots == 0 || (interp->channels + 15) / 16 == slots), "%s: bad interp segment (%d slots of 16 channels; 0: any)", who, slots);
    P.interp = *interp;
    return (interp->channels + 15) / 16;
}

// A chain of n layers, copied to dst with the image flag stripped from act.  All of its images are split images or all fp32 ones
// (`split`); layer l takes want[l] blocks of 16 channels and gives want[l + 1] (<= 0: any number); every image lies where the one
// before it ends, because the kernels stream a chain as one blob.  *next (optional): in, where the first image must lie unless null;
// out, where the last one ends.
static int pw_chain(const char *who, const char *what, int n, const rtk_layer_t *layers, bool split, const int *want, const float **next,
                    rtk_layer_t *dst) {
    RTK_REQUIRE(n >= 1 && n <= RTK_MAX_LAYERS && layers, "%s: %s: %d layers", who, what, n);
    const float *w = next ? *next : nullptr;
    int cin = want[0];
    for (int l = 0; l < n; ++l) {
        const rtk_layer_t &L = layers[l];
        RTK_REQUIRE(L.w_packed && L.bias && L.cin16 == cin && L.cout16 > 0 && (want[l + 1] <= 0 || L.cout16 == want[l + 1]),
                    "%s: %s: layer %d expects cin16=%d, cout16=%d (0: any), got %d, %d", who, what, l, cin, want[l + 1], L.cin16, L.cout16);
        RTK_REQUIRE(((L.act & RTK_LAYER_SPLIT) != 0) == split, "%s: %s: layer %d must be %s image like the rest of the chain", who, what, l,
                    split ? "a split" : "an fp32");
        RTK_REQUIRE(!w || L.w_packed == w, "%s: %s: the packed weights of a chain must be contiguous (layer %d)", who, what, l);
        w = L.w_packed + (size_t)(split ? split16_nf(L.cin16, L.cout16) : L.cin16 * L.cout16) * 256;
        dst[l] = L;
        dst[l].act = L.act & 0xff;
        cin = L.cout16;
    }
    if (next) *next = w;
    return RTK_OK;
}

// An output of `channels` <= max_channels channels; a row-major one has a pitch
static int pw_out(const char *who, const char *what, const float *out, int channels, int max_channels, bool row_major, int pitch) {
    RTK_REQUIRE(out && channels > 0 && channels <= max_channels, "%s: %s: %d channels (at most %d)", who, what, channels, max_channels);
    RTK_REQUIRE(!row_major || (pitch % 4 == 0 && pitch >= channels), "%s: %s: bad pitch %d for %d channels", who, what, pitch, channels);
    return RTK_OK;
}

// The family's grid: a workgroup owns one sample and strides over its groups of PW_NW * 16 rows; about wgs_target workgroups per
// launch, the rest is looped (1024: 5 % slower end to end)
static dim3 pw_grid(PwParams &P, int wgs_target) {
    const int samples = P.rows / P.rows_per_sample;
    const int groups = (P.rows_per_sample + PW_NW * 16 - 1) / (PW_NW * 16);
    int gx = wgs_target / samples;
    if (gx < 1) gx = 1;
    if (gx > groups) gx = groups;
    return rtk_xcd_grid(samples, gx, P.gx);
}

template <int U, int V1, int V2, int V3, int V4>
static int launch_pw(const PwParams &P0, bool interp, bool split, hipStream_t s) {
    PwParams P = P0;
    const dim3 blocks = pw_grid(P, PW_WGS_TARGET);
    if (interp && split) pointwise_mlp_kernel<U, V1, V2, V3, V4, true, true><<<blocks, 256, 0, s>>>(P);
    else if (interp) pointwise_mlp_kernel<U, V1, V2, V3, V4, true, false><<<blocks, 256, 0, s>>>(P);
    else if (split) pointwise_mlp_kernel<U, V1, V2, V3, V4, false, true><<<blocks, 256, 0, s>>>(P);
    else pointwise_mlp_kernel<U, V1, V2, V3, V4, false, false><<<blocks, 256, 0, s>>>(P);
    return 0;
}

extern "C" int rtk_pointwise_mlp(int rows, int rows_per_sample, const rtk_interp_t *interp, int nsrc,
                                 const rtk_src_t *srcs, const float *sample_bias, int nlayers,
                                 const rtk_layer_t *layers, float *out, int out_pitch, int out_channels,
                                 int out_channel_major, const int *row_nuniq, float *colmax, rtk_stream_t stream) {
    static const char who[] = "pointwise_mlp";
    PwParams P;
    memset(&P, 0, sizeof(P));
    if (pw_rows(who, P, rows, rows_per_sample) < 0) return RTK_ERR_INVALID;
    const int ui = interp ? pw_interp(who, P, interp, 0) : 0, us = pw_sources(who, P, nsrc, srcs);
    if (ui < 0 || us < 0) return RTK_ERR_INVALID;
    const int U = ui + us, want[RTK_MAX_LAYERS + 1] = {U, 0, 0, 0, 0};
    const bool split = nlayers >= 1 && layers && (layers[0].act & RTK_LAYER_SPLIT) != 0;      // the chain's images are split images (rtk_fused.h)
    if (pw_chain(who, "chain", nlayers, layers, split, want, nullptr, P.layer) < 0) return RTK_ERR_INVALID;
    int V[RTK_MAX_LAYERS] = {0, 0, 0, 0};
    for (int l = 0; l < nlayers; ++l) V[l] = P.layer[l].cout16;
    if (pw_out(who, "out", out, out_channels, 16 * V[nlayers - 1], !out_channel_major, out_pitch) < 0) return RTK_ERR_INVALID;
    P.sample_bias = sample_bias; P.row_nuniq = row_nuniq; P.colmax = colmax;
    P.out = out; P.out_pitch = out_pitch; P.out_channels = out_channels; P.out_cm = out_channel_major;
    hipStream_t s = (hipStream_t)stream;
    const bool it = interp != nullptr;
    const long key = ((((long)U * 32 + V[0]) * 32 + V[1]) * 32 + V[2]) * 32 + V[3];
#define PW_CASE(u, v1, v2, v3, v4)                                               \
    case ((((long)(u) * 32 + (v1)) * 32 + (v2)) * 32 + (v3)) * 32 + (v4):        \
        launch_pw<u, v1, v2, v3, v4>(P, it, split, s);                           \
        break;
    switch (key) {
        PW_CASE(1, 2, 0, 0, 0)     // raw (RCS, v_r) -> sa1 layer-1 projections (2 scales x 16)
        PW_CASE(4, 6, 0, 0, 0)     // sa1 out 64 -> linear1 (32) || sa2 projections (32+32)
        PW_CASE(6, 12, 0, 0, 0)    // sa2 out 96 -> linear2 (64) || sa3 projections (64+64)
        PW_CASE(8, 4, 0, 0, 0)     // sa3 out 128 -> linear3 (64): a launch of its own only on the comparison path (fused.FOLD_LIN3 off)
        PW_CASE(8, 8, 0, 0, 0)     // fp1 (interp 128) -> 128; fp3 (interp 64 || skip 64) on linear3's output (comparison path)
        PW_CASE(10, 8, 0, 0, 0)    // fp2 (interp 128 || skip 32) -> 128
        PW_CASE(12, 8, 0, 0, 0)    // fp3 with linear3 composed in (interp of sa3's 128 || skip 64) -> 128
        PW_CASE(8, 16, 0, 0, 0)    // local features 128 -> cost-volume layer-1 projection 256
        PW_CASE(16, 8, 4, 2, 1)    // cls head 256 -> 128 -> 64 -> 32 -> 1
        PW_CASE(8, 8, 4, 2, 1)     // flow head (prop 128 + per-sample GRU term) -> 128 -> 64 -> 32 -> 3
        PW_CASE(25, 2, 0, 0, 0)    // decoder embeddings (2 || 128 || 256 + per-sample) -> mse.sa1 projections
        PW_CASE(8, 2, 0, 0, 0)
        default:
            rtk_set_error("pointwise_mlp: no kernel instance for shape U=%d V=(%d,%d,%d,%d)", U, V[0], V[1], V[2], V[3]);
            return RTK_ERR_UNSUPPORTED;
    }
#undef PW_CASE
    RTK_CHECK_LAUNCH("pointwise_mlp");
    return RTK_OK;
}

// ---- rtk_pointwise_mlp_tap ---------------------------------------------------------------------------------------------
// The encoder's last layer (fp1: interpolation -> 128, ReLU, column max) followed, on the tile still in registers, by a linear
// 128 -> 256 projection whose image is chosen per sample (frame 1 / frame 2 of the cost volume): the two per-point launches that
// read the layer's output back are gone.  The 256 outputs are computed as two halves of eight 16-channel blocks on the same
// activation pieces (one split per tile): a 16-block accumulator set next to the layer's would not fit two waves per SIMD.
//
// The weight stream runs over two images: chunks [0, C1) are the layer's, the rest the frame's projection image, visited half by
// half -- logical fragment F1 + PH h + PR up + r (half h, input block pair up, r < PR = 2 VH) is fragment PR (2 up + h) + r of the
// split image (layout of fused_common.h: frag[up][v][p] with 2 VH output blocks), so a chunk is one contiguous run of the image.
template <int NW, int F, int NF, int C1, int UP, int VH>
struct WStreamTap {       // WStream's protocol (start_deferred, next, frag, finish) over the two sources; not a WStream, so that no
                          // routine written for one can take it and issue from the wrong image
    static constexpr int NCHUNKS = NF / F, PR = 2 * VH, PH = UP * PR;
    static_assert(NF % F == 0 && PR % F == 0 && C1 < NCHUNKS, "whole chunks; a chunk of the projection is one run of the image");
    const char *blob;     // the layer's image (chunks [0, C1))
    const char *proj;     // the sample's projection image
    f4 *lds;
    unsigned lane_off;
    int cur, buf, wave, lane;
    __device__ __forceinline__ void issue(int chunk, int into) {
        const char *base;
        if (chunk < C1) {
            base = blob + (size_t)chunk * F * 1024;
        } else {
            const int l = (chunk - C1) * F, h = l / PH, up = (l % PH) / PR, r = l % PR;
            base = proj + (size_t)(PR * (2 * up + h) + r) * 1024;
        }
#pragma unroll
        for (int i = 0; i < (F + NW - 1) / NW; ++i) {
            const int f = wave + i * NW;
            if (f < F)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(base + (size_t)i * NW * 1024 + lane_off),
                                                 (__attribute__((address_space(3))) void *)(lds + (into * F + f) * 64), 16, 0, 0);
        }
    }
    // WStream::start_deferred: chunk 0 requested, the state that of a pass that has just ended; the first next() waits
    __device__ __forceinline__ void start_deferred(const f4 *blob_, const f4 *proj_, f4 *lds_, int wave_, int lane_) {
        blob = reinterpret_cast<const char *>(blob_);
        proj = reinterpret_cast<const char *>(proj_);
        lds = lds_; wave = wave_; lane = lane_;
        lane_off = (unsigned)(wave * 64 + lane) * 16u;
        cur = NCHUNKS - 1; buf = 1;
        issue(0, 0);
    }
    __device__ __forceinline__ void next() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
        cur = cur + 1 == NCHUNKS ? 0 : cur + 1;
        asm volatile("" : "+s"(cur));      // (WStream::next)
        issue(cur + 1 == NCHUNKS ? 0 : cur + 1, buf ^ 1);
    }
    __device__ __forceinline__ f4 frag(int f_in_chunk) const { return lds[(buf * F + f_in_chunk) * 64 + lane]; }
    __device__ __forceinline__ void finish() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

struct TapParams {
    PwParams pw;                  // the layer: interpolation segment, layer[0], out (the layer's output), colmax
    const float *proj_w[2];       // split images of the projection: samples < frame_split, the others
    const float *proj_b[2];
    float proj_inv[2];
    int frame_split;
    float *pout;                  // (rows, pout_pitch): the projection
    int pout_pitch;
};

template <int U, int V1, int VP>
__global__ __launch_bounds__(64 * PW_NW, 2) void pointwise_tap_kernel(const TapParams T) {
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * PW_F * 64];
    const PwParams &P = T.pw;
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int wave_in_wg = threadIdx.x >> 6;
    int b, bx, nbx;
    rtk_decode_block(P.gx, b, bx, nbx);
    const int rps = P.rows_per_sample;
    const int groups = (rps + PW_NW * 16 - 1) / (PW_NW * 16);
    if (bx >= groups) return;
    constexpr int UP = (V1 + 1) / 2, VH = VP / 2, F1 = split16_nf(U, V1), PH = UP * 2 * VH;
    static_assert(VP % 2 == 0 && F1 % PW_F == 0, "whole chunks of the layer, two equal halves of the projection");
    WStreamTap<PW_NW, PW_F, F1 + 2 * PH, F1 / PW_F, UP, VH> ws;
    const bool f2 = b >= T.frame_split;                    // uniform over the workgroup: one sample
    const float *pbias = f2 ? T.proj_b[1] : T.proj_b[0];
    const float pinv = f2 ? T.proj_inv[1] : T.proj_inv[0];
    ws.start_deferred(reinterpret_cast<const f4 *>(P.layer[0].w_packed), reinterpret_cast<const f4 *>(f2 ? T.proj_w[1] : T.proj_w[0]), s_w,
                      wave_in_wg, lane);

    for (int G = bx; G < groups; G += nbx) {
        asm volatile("" ::: "memory");
        const int r = G * (PW_NW * 16) + wave_in_wg * 16 + j;
        const bool valid = r < rps;
        const int p = b * rps + (valid ? r : rps - 1);
        f4 h[U];
        load_interp<U>(P, p, b, g, U, h);
        // the layer: pw_layer's split path (the first next() waits for chunk 0 together with the loads above)
        f4 a1[V1];
        {
            const LaneScale s1 = lane_scale16(h);
            init_zero<V1>(a1);
            ws.next();
            mlp_layer_split_impl<U, V1, 0, decltype(ws), PW_F>(ws, h, s1.s, a1, std::make_integer_sequence<int, ((U + 1) / 2) * ((V1 + 1) / 2)>{});
            scale_bias<V1>(a1, s1.inv * P.layer[0].inv_scale, P.layer[0].bias, g);
            apply_act<V1>(a1, P.layer[0].act);
        }
        store_tile<V1>(P, a1, p, b, g, valid);
        // the projection: a1's pieces once, then each half on them (rtk_pointwise_mlp's arithmetic for the same layer: bit for bit)
        const LaneScale sc = lane_scale16(a1);
        u4v pc[UP][2];
#pragma unroll
        for (int up = 0; up < UP; ++up) split2(a1[2 * up], 2 * up + 1 < V1 ? a1[2 * up + 1] : f4_zero(), sc.s, pc[up]);
        const float c = sc.inv * pinv;
        float *o = T.pout + (size_t)p * T.pout_pitch + 4 * g;
        auto half = [&](auto hc) {
            constexpr int hv = decltype(hc)::value;
            f4 acc[VH];
            init_zero<VH>(acc);
            mlp_layer_pieces_impl<V1, VH, F1 + hv * PH, decltype(ws), PW_F>(ws, pc, acc, std::make_integer_sequence<int, UP * (VH / 2)>{});
            scale_bias<VH>(acc, c, pbias + 16 * VH * hv, g);
            if (valid) {
#pragma unroll
                for (int v = 0; v < VH; ++v) *reinterpret_cast<f4 *>(o + 16 * (VH * hv + v)) = acc[v];
            }
        };
        half(std::integral_constant<int, 0>{});
        half(std::integral_constant<int, 1>{});
    }
    ws.finish();
}

extern "C" int rtk_pointwise_mlp_tap(int rows, int rows_per_sample, const rtk_interp_t *interp, const rtk_layer_t *layer, float *out,
                                     int out_pitch, float *colmax, const rtk_layer_t *proj, int frame_split, float *proj_out, int proj_pitch,
                                     rtk_stream_t stream) {
    static const char who[] = "pointwise_mlp_tap";
    static const int layer_blocks[2] = {8, 8}, proj_blocks[2] = {8, 16};
    TapParams T;
    memset(&T, 0, sizeof(T));
    PwParams &P = T.pw;
    if (pw_rows(who, P, rows, rows_per_sample) < 0 || pw_interp(who, P, interp, 8) < 0 ||
        pw_chain(who, "the split 128 -> 128 layer", 1, layer, true, layer_blocks, nullptr, P.layer) < 0 ||
        pw_out(who, "out", out, 128, 128, true, out_pitch) < 0 || pw_out(who, "proj_out", proj_out, 256, 256, true, proj_pitch) < 0)
        return RTK_ERR_INVALID;
    RTK_REQUIRE(proj && frame_split >= 0, "%s: bad projection (frame_split %d)", who, frame_split);
    for (int k = 0; k < 2; ++k) {
        rtk_layer_t L;
        if (pw_chain(who, "a split 128 -> 256 projection", 1, proj + k, true, proj_blocks, nullptr, &L) < 0) return RTK_ERR_INVALID;
        RTK_REQUIRE(L.act == 0, "%s: projection %d must have no activation", who, k);
        T.proj_w[k] = L.w_packed; T.proj_b[k] = L.bias; T.proj_inv[k] = L.inv_scale;
    }
    P.out = out; P.out_pitch = out_pitch; P.out_channels = 128; P.colmax = colmax;
    T.frame_split = frame_split; T.pout = proj_out; T.pout_pitch = proj_pitch;
    const dim3 blocks = pw_grid(P, PW_WGS_TARGET);
    pointwise_tap_kernel<8, 8, 16><<<blocks, 64 * PW_NW, 0, (hipStream_t)stream>>>(T);
    RTK_CHECK_LAUNCH("pointwise_mlp_tap");
    return RTK_OK;
}

// ---- rtk_pointwise_mlp_pair --------------------------------------------------------------------------------------------
// Two chains that read the same wide rows in one launch (the decoder front: the sa1 projection of [raw | f1 | cor] and the class
// head on cor): the tile's 25 input slots are loaded once, chain A (25 -> 2 blocks, one layer) runs on all of them and is stored,
// then chain B (16 -> 8 -> 4 -> 2 -> 1) runs on the last 16 slots of the same registers.  Each chain does pw_layer's split
// arithmetic with its own position scale (chain B's from its 16 slots only), images, inverse scales and bias: both outputs are
// rtk_pointwise_mlp's bit for bit.  One weight stream over one blob: chain A's fragments first, then chain B's.
struct PairParams {
    PwParams pw;                  // the sources, chain A (layer[0], sample_bias, out: row-major), the grid
    rtk_layer_t lb[4];            // chain B
    float *out_b;                 // (samples, out_b_channels, rows_per_sample) channel-major
    int out_b_channels;
};

template <int U, int VA, int UB, int V1, int V2, int V3, int V4>
__global__ __launch_bounds__(64 * PW_NW, 2) void pointwise_pair_kernel(const PairParams T) {
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * PW_F * 64];
    const PwParams &P = T.pw;
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int wave_in_wg = threadIdx.x >> 6;
    int b, bx, nbx;
    rtk_decode_block(P.gx, b, bx, nbx);
    const int rps = P.rows_per_sample;
    const int groups = (rps + PW_NW * 16 - 1) / (PW_NW * 16);
    if (bx >= groups) return;
    constexpr int FA = split16_nf(U, VA), F1 = split16_nf(UB, V1), F2 = split16_nf(V1, V2), F3 = split16_nf(V2, V3), F4 = split16_nf(V3, V4);
    WStream<PW_NW, PW_F, FA + F1 + F2 + F3 + F4> ws;
    ws.start_deferred(reinterpret_cast<const f4 *>(P.layer[0].w_packed), s_w, wave_in_wg, lane);

    int ustart[RTK_MAX_SRC + 1];
    ustart[0] = 0;
#pragma unroll
    for (int s = 0; s < RTK_MAX_SRC; ++s) ustart[s + 1] = ustart[s] + (s < P.nsrc ? (P.src[s].channels + 15) >> 4 : 0);
    const int uend = ustart[RTK_MAX_SRC];

    for (int G = bx; G < groups; G += nbx) {
        asm volatile("" ::: "memory");
        const int r = G * (PW_NW * 16) + wave_in_wg * 16 + j;
        const bool valid = r < rps;
        const int p = b * rps + (valid ? r : rps - 1);
        // ---- the input slots, as pointwise_mlp_kernel loads them ---------------------------------------
        f4 h[U];
        const float *rowp[RTK_MAX_SRC];
        const float *dummy = reinterpret_cast<const float *>(P.layer[0].w_packed);
#pragma unroll
        for (int q = 0; q < RTK_MAX_SRC; ++q)
            rowp[q] = q < P.nsrc ? P.src[q].ptr + (P.src[q].per_sample ? (size_t)b : (size_t)p) * P.src[q].pitch + 4 * g : nullptr;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float *rp = rowp[0];
            int us = ustart[0], ch = P.src[0].channels;
#pragma unroll
            for (int q = 1; q < RTK_MAX_SRC; ++q)
                if (q < P.nsrc && u >= ustart[q]) { rp = rowp[q]; us = ustart[q]; ch = P.src[q].channels; }
            const int c = 16 * (u - us);
            const bool ok = u < uend && c + 4 * g < ch;
            const f4 v = *reinterpret_cast<const f4 *>(ok ? rp + c : dummy);
            h[u] = ok ? v : f4_zero();
        }
        // ---- chain A on every slot; its accumulators are stored before chain B starts --------------------
        {
            f4 a[VA];
            pw_layer<true, U, VA, 0>(ws, h, a, P.layer[0], g, P.sample_bias ? P.sample_bias + (size_t)b * 16 * VA : nullptr, true);
            store_tile<VA>(P, a, p, b, g, valid);
        }
        // ---- chain B on the last UB slots ------------------------------------------------------------------
        f4 hb[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) hb[u] = h[U - UB + u];
        f4 a1[V1], a2[V2], a3[V3], a4[V4];
        pw_layer<true, UB, V1, FA>(ws, hb, a1, T.lb[0], g, nullptr, false);
        pw_layer<true, V1, V2, FA + F1>(ws, a1, a2, T.lb[1], g, nullptr, false);
        pw_layer<true, V2, V3, FA + F1 + F2>(ws, a2, a3, T.lb[2], g, nullptr, false);
        pw_layer<true, V3, V4, FA + F1 + F2 + F3>(ws, a3, a4, T.lb[3], g, nullptr, false);
        if (valid) {
            float *o = T.out_b + (size_t)b * T.out_b_channels * rps + (p - b * rps);
#pragma unroll
            for (int v = 0; v < V4; ++v) {
                const int c = 16 * v + 4 * g;
                if (c + 0 < T.out_b_channels) o[(size_t)(c + 0) * rps] = a4[v].x;
                if (c + 1 < T.out_b_channels) o[(size_t)(c + 1) * rps] = a4[v].y;
                if (c + 2 < T.out_b_channels) o[(size_t)(c + 2) * rps] = a4[v].z;
                if (c + 3 < T.out_b_channels) o[(size_t)(c + 3) * rps] = a4[v].w;
            }
        }
    }
    ws.finish();
}

extern "C" int rtk_pointwise_mlp_pair(int rows, int rows_per_sample, int nsrc, const rtk_src_t *srcs, const float *sample_bias,
                                      const rtk_layer_t *layer_a, float *out_a, int out_a_pitch, int out_a_channels, int nlayers_b,
                                      const rtk_layer_t *layers_b, float *out_b, int out_b_channels, rtk_stream_t stream) {
    static const char who[] = "pointwise_mlp_pair";
    static const int a_blocks[2] = {25, 2}, b_blocks[5] = {16, 8, 4, 2, 1};
    PairParams T;
    memset(&T, 0, sizeof(T));
    PwParams &P = T.pw;
    if (pw_rows(who, P, rows, rows_per_sample) < 0) return RTK_ERR_INVALID;
    const int U = pw_sources(who, P, nsrc, srcs);
    if (U < 0) return RTK_ERR_INVALID;
    // the one instance: [.. | 256 channels] -> 32 next to 256 -> 128 -> 64 -> 32 -> 16 on the last source, split images in one blob
    const int UB = nsrc >= 1 ? (srcs[nsrc - 1].channels + 15) / 16 : 0;
    RTK_REQUIRE(U == 25 && UB == 16 && nlayers_b == 4, "%s: no kernel instance for U=%d UB=%d, %d layers", who, U, UB, nlayers_b);
    const float *w = nullptr;
    if (pw_chain(who, "chain A", 1, layer_a, true, a_blocks, &w, P.layer) < 0 || pw_chain(who, "chain B", 4, layers_b, true, b_blocks, &w, T.lb) < 0 ||
        pw_out(who, "out_a", out_a, out_a_channels, 32, true, out_a_pitch) < 0 || pw_out(who, "out_b", out_b, out_b_channels, 16, false, 0) < 0)
        return RTK_ERR_INVALID;
    P.sample_bias = sample_bias; P.out = out_a; P.out_pitch = out_a_pitch; P.out_channels = out_a_channels;
    T.out_b = out_b; T.out_b_channels = out_b_channels;
    const dim3 blocks = pw_grid(P, PW_WGS_TARGET);
    pointwise_pair_kernel<25, 2, 16, 8, 4, 2, 1><<<blocks, 64 * PW_NW, 0, (hipStream_t)stream>>>(T);
    RTK_CHECK_LAUNCH("pointwise_mlp_pair");
    return RTK_OK;
}
