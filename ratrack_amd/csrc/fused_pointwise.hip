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

// A pointer read from memory is a generic one (flat instructions, which count as LDS accesses too); the kernel's own pointer
// arguments are known to be global.  The cast there and back tells the compiler what it knows of the arguments themselves.
template <class X>
__device__ __forceinline__ void pw_global(X *&p) { p = (X *)(__attribute__((address_space(1))) X *)(unsigned long long)p; }
__device__ __forceinline__ void pw_globalize(PwParams &P) {
    pw_global(P.interp.known_feats); pw_global(P.interp.idx); pw_global(P.interp.dist2); pw_global(P.interp.nuniq);
#pragma unroll
    for (int q = 0; q < RTK_MAX_SRC; ++q) pw_global(P.src[q].ptr);
#pragma unroll
    for (int l = 0; l < RTK_MAX_LAYERS; ++l) { pw_global(P.layer[l].w_packed); pw_global(P.layer[l].bias); }
    pw_global(P.sample_bias); pw_global(P.out); pw_global(P.row_nuniq); pw_global(P.colmax);
}

// The kernel's arguments, read again from the kernarg segment where a phase of the tile uses them (T: the kernel's one argument).
// Held in scalar registers from the top of the kernel they outlive every tile, 60 - 90 of the 102 registers, and the allocator
// parks them in lanes of vector registers; a phase that reads its own copy through an offset the optimiser cannot see (so that the
// reads stay inside the trip) holds only the fields it uses, for as long as it uses them.  The reads hit the scalar cache.
// pw_args_now reads sizeof(T) bytes from offset 0 of the kernarg segment: right only in a kernel whose one by-value argument is a T.
// It therefore takes a PwKernarg<T>, which a __global__ function makes from that argument and hands down to the body it calls -- a
// body cannot name the block it reads without having been given it by its kernel.  (A kernel with a second argument in front of
// the T, or a body meant to work on a modified copy of the arguments, must not make one.)
template <class T>
struct PwKernarg {
    __device__ __forceinline__ explicit PwKernarg(const T &the_kernels_only_argument) { (void)the_kernels_only_argument; }
};
template <class T>
__device__ __forceinline__ T pw_args_now(PwKernarg<T>) {
    unsigned z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    typedef const __attribute__((address_space(4))) unsigned long long *words_t;
    static_assert(sizeof(T) % 8 == 0, "whole 8-byte words");
    const words_t k = (words_t)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + z);
    union { T a; unsigned long long w[sizeof(T) / 8]; } u;
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 8; ++i) u.w[i] = k[i];
    pw_globalize(u.a);
    return u.a;
}

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
// `entered` runs once the first layer of a tile has entered the weight stream (behind the wait every tile makes there): the place
// where the pipelined loops request the next group's rows, with a whole chunk of products in front of the stream's next wait.
struct PwNothing { __device__ __forceinline__ void operator()() const {} };
template <bool SPLIT, int U, int V, int FBASE, class WS, class Entered = PwNothing>
__device__ __forceinline__ void pw_layer(WS &ws, const f4 (&h)[U], f4 (&acc)[V], const rtk_layer_t &L, int g, const float *sample_bias, bool first,
                                         Entered entered = Entered()) {
    if constexpr (SPLIT) {
        const LaneScale sc = lane_scale16(h);
        init_zero<V>(acc);
        if (first) { ws.next_if_deferred(); entered(); }
        mlp_layer_ws_split<U, V, FBASE>(ws, h, sc.s, acc);
        scale_bias<V>(acc, sc.inv * L.inv_scale, L.bias, g);
    } else {
        init_bias<V>(acc, L.bias, g);
        if (first) { ws.next_if_deferred(); entered(); }
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

// ---- the same input assembly in pieces, for the pipelined loops: request, address, gather, use -----------------------------------
// The three-NN row of global row p: its addresses depend on nothing loaded.
struct InterpRow { int id[3]; float d2[3]; };
__device__ __forceinline__ void interp_request(const PwParams &P, int p, InterpRow &q) {
    const int *idp = P.interp.idx + (size_t)p * 3;
    const float *d2 = P.interp.dist2 + (size_t)p * 3;
    q.id[0] = idp[0]; q.id[1] = idp[1]; q.id[2] = idp[2];
    q.d2[0] = d2[0]; q.d2[1] = d2[1]; q.d2[2] = d2[2];
}
// load_interp's clamp (e: the sample's interp.nuniq, or INT_MAX without one), weights and row addresses
struct InterpTaps { const float *k[3]; float w[3]; };
__device__ __forceinline__ void interp_taps(const PwParams &P, int b, int e, const InterpRow &q, InterpTaps &t) {
    const float r0 = __fdiv_rn(1.0f, __fadd_rn(__fsqrt_rn(q.d2[0]), 1e-8f));
    const float r1 = __fdiv_rn(1.0f, __fadd_rn(__fsqrt_rn(q.d2[1]), 1e-8f));
    const float r2 = __fdiv_rn(1.0f, __fadd_rn(__fsqrt_rn(q.d2[2]), 1e-8f));
    const float norm = __fadd_rn(__fadd_rn(r0, r1), r2);
    t.w[0] = __fdiv_rn(r0, norm); t.w[1] = __fdiv_rn(r1, norm); t.w[2] = __fdiv_rn(r2, norm);
#pragma unroll
    for (int i = 0; i < 3; ++i) t.k[i] = P.interp.known_feats + ((size_t)b * P.interp.m + (q.id[i] < e ? q.id[i] : 0)) * P.interp.pitch;
}
// the three known rows of NI slots, requested (load_interp's unconditional loads) ...
template <int NI>
__device__ __forceinline__ void interp_gather(const PwParams &P, const InterpTaps &t, int g, f4 (&ga)[3][NI]) {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const int c = 16 * u + 4 * g, cc = c < P.interp.channels ? c : 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) ga[i][u] = *reinterpret_cast<const f4 *>(t.k[i] + cc);
    }
}
// ... and combined into the slots u < NI of the lane's input: load_interp's arithmetic, two channels per instruction.  The three
// weights are pinned as pairs of their own: carried through the loop in single registers, the compiler broadcasts the one that
// lands in the odd half of a pair through the packed instruction's op_sel modifier -- the form that misreads next to matrix work
// (tests/test_isa_cpu.py keeps it out of this file).
template <int NI, int U>
__device__ __forceinline__ void interp_combine(const PwParams &P, const InterpTaps &t, int g, const f4 (&ga)[3][NI], f4 (&h)[U]) {
    f2v w0 = {t.w[0], t.w[0]}, w1 = {t.w[1], t.w[1]}, w2 = {t.w[2], t.w[2]};
    asm volatile("" : "+v"(w0), "+v"(w1), "+v"(w2));
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const f4 a0 = ga[0][u], a1 = ga[1][u], a2 = ga[2][u];
        // interpolate_gpu.cu:168  w0*p0 + w1*p1 + w2*p2  (nvcc: fma(w2,p2,fma(w1,p1,w0*p0)); fp-contract is off: a product, two fmas)
        const f2v lo = __builtin_elementwise_fma(w2, (f2v){a2.x, a2.y}, __builtin_elementwise_fma(w1, (f2v){a1.x, a1.y}, w0 * (f2v){a0.x, a0.y}));
        const f2v hi = __builtin_elementwise_fma(w2, (f2v){a2.z, a2.w}, __builtin_elementwise_fma(w1, (f2v){a1.z, a1.w}, w0 * (f2v){a0.z, a0.w}));
        const f4 v = {lo[0], lo[1], hi[0], hi[1]};
        h[u] = 16 * u + 4 * g < P.interp.channels ? v : f4_zero();
    }
}
// The plain slots u >= U0 of global row p (sample b), requested into raw[] by the serial loop's rule (the source that owns the slot
// is wave-uniform; lanes past its last channel read the dummy address) and, in plain_use, masked into the lane's input.  The owner's
// fields are selected as scalars and the lane's address is formed per slot: a selection among the lanes' row pointers becomes an
// indexed array in scratch.  The mask is a word the optimiser cannot see through: from `ok ? loaded : 0` it makes a branch around
// the load, and the load waits there.
struct PlainSrc { unsigned long long ptr; int pitch, per_sample, ch; };
struct PlainSlot { PlainSrc s; int c; };
typedef const __attribute__((address_space(1))) f4 *pw_global_f4;
__device__ __forceinline__ int plain_nsrc(const PwParams &P) {      // P.nsrc, opaque and read where it is called: what is selected by it is not
    int nsrc = P.nsrc;                                               // carried through the tile loop, one set of registers per slot
    asm volatile("" : "+s"(nsrc));
    return nsrc;
}
__device__ __forceinline__ PlainSlot plain_slot(const PwParams &P, int nsrc, int u0, int u) {
    PlainSrc S[RTK_MAX_SRC];        // (registers, not memory: a selection among loads of P.src[] becomes a copy of it in scratch)
#pragma unroll
    for (int q = 0; q < RTK_MAX_SRC; ++q) {
        S[q] = PlainSrc{(unsigned long long)P.src[q].ptr, P.src[q].pitch, P.src[q].per_sample, P.src[q].channels};
        asm("" : "+s"(S[q].ptr), "+s"(S[q].pitch), "+s"(S[q].per_sample), "+s"(S[q].ch));
    }
    PlainSlot r{S[0], 0};
    int us = u0, next = u0;
#pragma unroll
    for (int q = 1; q < RTK_MAX_SRC; ++q) {
        next += (S[q - 1].ch + 15) >> 4;
        const bool take = q < nsrc && u >= next;
        r.s.ptr = take ? S[q].ptr : r.s.ptr; r.s.pitch = take ? S[q].pitch : r.s.pitch;
        r.s.per_sample = take ? S[q].per_sample : r.s.per_sample; r.s.ch = take ? S[q].ch : r.s.ch;
        us = take ? next : us;
    }
    r.c = 16 * (u - us);
    return r;
}
// (u0: the first plain slot, U0 <= u0: a constant in the pipelined loops, the interpolation segment's slot count in the serial one)
template <int U0, int U>
__device__ __forceinline__ void plain_request(const PwParams &P, int u0, int p, int b, int g, f4 (&raw)[U]) {
    const unsigned long long dummy = (unsigned long long)P.layer[0].w_packed;
    const int nsrc = plain_nsrc(P);
#pragma unroll
    for (int u = U0; u < U; ++u) {
        if (u < u0) continue;
        const PlainSlot r = plain_slot(P, nsrc, u0, u);
        unsigned long long a = r.s.ptr + 4ull * ((r.s.per_sample ? (size_t)b : (size_t)p) * r.s.pitch + 4 * g + r.c);
        asm("" : "+v"(a));          // (formed for every lane: under the lane's condition it would be a block of its own)
        raw[u] = *reinterpret_cast<pw_global_f4>(r.c + 4 * g < r.s.ch ? a : dummy);
        __builtin_amdgcn_sched_barrier(0);      // (slot by slot: scheduled together, the slots' scalars do not fit the scalar registers)
    }
}
template <int U0, int U>
__device__ __forceinline__ void plain_use(const PwParams &P, int u0, int g, const f4 (&raw)[U], f4 (&h)[U]) {
    const int nsrc = plain_nsrc(P);
#pragma unroll
    for (int u = U0; u < U; ++u) {
        if (u < u0) continue;
        const PlainSlot r = plain_slot(P, nsrc, u0, u);
        unsigned m = r.c + 4 * g < r.s.ch ? 0xffffffffu : 0u;
        asm("" : "+v"(m));
        h[u] = (f4){__uint_as_float(__float_as_uint(raw[u].x) & m), __uint_as_float(__float_as_uint(raw[u].y) & m),
                    __uint_as_float(__float_as_uint(raw[u].z) & m), __uint_as_float(__float_as_uint(raw[u].w) & m)};
        __builtin_amdgcn_sched_barrier(0);
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

#define PW_PIPE_NI 8       // interpolation slots (128 channels) of the pipelined interpolating instances: launch_pw routes the others to the serial loop

// The tile loop software-pipelined by one group.  The serial loop (below) makes, per group and strictly one after the other: the
// three-NN row -> the known rows and the source rows -> the wrap of the weight stream -> products -> stores; and before its first
// group it waits for row_nuniq[b] with nothing in flight.  Here
//   - row_nuniq[b], interp.nuniq[b] and the first group's three-NN row (without interpolation: its source rows) are requested
//     together; liveness is decided when row_nuniq has arrived, and only then does the workgroup start the stream (a workgroup that
//     exits has no LDS-DMA outstanding) and form an address from an index;
//   - the next group's three-NN row (without interpolation: its source rows, into registers of their own) is requested as soon as
//     the tile has entered the stream -- a chunk of products lies before the stream's next wait, which is as old as the request;
//   - an interpolating instance cannot hold three known rows per slot next to its accumulators through the products; it computes
//     the next group's weights and addresses and requests its known and source rows in front of the stores, when only the last
//     layer's accumulators are live.  One round trip per group is left exposed there, none without interpolation.
// A next group's rows are requested only if that group is live (the three-NN tables hold in-range indices up to the last live
// group: PW_NW below), so the loop body exists twice: steady state and last group -- a wave-uniform test around the requests makes
// the compiler wait at the join.  Same loads, same arithmetic in the same order as the serial loop: the same bits.
template <int U, int V1, int V2, int V3, int V4, bool INTERP, bool SPLIT>
__device__ __forceinline__ void pw_pipelined(const PwParams &P, PwKernarg<PwParams> ka, f4 *s_w) {
    constexpr int NI = INTERP ? PW_PIPE_NI : 0;
    static_assert(NI <= U, "the interpolation segment is part of the input");
    const int lane = threadIdx.x & 63, g0 = lane >> 4, j = lane & 15;
    const int wave_in_wg = threadIdx.x >> 6;
    int b, bx, nbx;
    rtk_decode_block(P.gx, b, bx, nbx);
    const int rps = P.rows_per_sample;
    const int rw = wave_in_wg * 16 + j;                               // row within a group
    auto row_of = [&](int G) { const int r = G * (PW_NW * 16) + rw; return b * rps + (r < rps ? r : rps - 1); };
    // ---- prologue: whatever depends on nothing loaded goes out together ----------------------------------------------------
    int nu = rps, e = 0x7fffffff;
    if (P.row_nuniq) nu = P.row_nuniq[b];
    if (INTERP && P.interp.nuniq) e = P.interp.nuniq[b];
    InterpRow q;                    // of the group whose known rows are requested next
    f4 raw[U];                      // plain slots: requested rows of the next group to use them
    if constexpr (INTERP) interp_request(P, row_of(bx), q);
    else plain_request<0, U>(P, 0, row_of(bx), b, g0, raw);
    __builtin_amdgcn_sched_barrier(0);
    const int live_rows = min(rps, __builtin_amdgcn_readfirstlane(nu));
    const int live_groups = (live_rows + PW_NW * 16 - 1) / (PW_NW * 16);
    if (bx >= live_groups) return;
    constexpr int F1 = SPLIT ? split16_nf(U, V1) : U * V1, F2 = SPLIT ? split16_nf(V1, V2) : V1 * V2,
                  F3 = SPLIT ? split16_nf(V2, V3) : V2 * V3, F4 = SPLIT ? split16_nf(V3, V4) : V3 * V4;
    constexpr int NF = F1 + F2 + F3 + F4;
    WStream<PW_NW, PW_F, NF> ws;
    if constexpr (NF > PW_F) ws.start_deferred(reinterpret_cast<const f4 *>(P.layer[0].w_packed), s_w, wave_in_wg, lane);
    else ws.start(reinterpret_cast<const f4 *>(P.layer[0].w_packed), s_w, wave_in_wg, lane);
    InterpTaps t;
    constexpr int NG = NI > 0 ? NI : 1;             // (an array cannot be empty; without interpolation it is never touched)
    f4 ga[3][NG] = {};
    if constexpr (INTERP) {
        interp_taps(P, b, e, q, t);
        interp_gather<NG>(P, t, g0, ga);
        plain_request<NI, U>(P, NI, row_of(bx), b, g0, raw);
    }

    int G = bx;
    auto tile = [&](auto more) {
        constexpr bool MORE = decltype(more)::value;
        asm volatile("" ::: "memory");
        int g = g0;
        asm volatile("" : "+v"(g));     // per-lane addresses (bias fragments, stores) are formed in the tile: hoisted out of the loop they are spilled
        const int r = G * (PW_NW * 16) + rw;
        const bool valid = r < live_rows;
        const int p = row_of(G), pn = row_of(G + nbx);
        f4 h[U];
        {
            const PwParams P = pw_args_now(ka);
            if constexpr (INTERP) interp_combine<NG, U>(P, t, g, ga, h);
            plain_use<NI, U>(P, NI, g, raw, h);
        }
        auto entered = [&]() {
            if constexpr (MORE) {
                const PwParams P = pw_args_now(ka);
                if constexpr (INTERP) interp_request(P, pn, q);
                else plain_request<0, U>(P, 0, pn, b, g, raw);
                __builtin_amdgcn_sched_barrier(0);      // (the requests stay here: the scheduler otherwise moves them down to their first use)
            }
        };
        auto store = [&](auto &acc) {
            const PwParams P = pw_args_now(ka);
            if constexpr (MORE && INTERP) {
                __builtin_amdgcn_sched_barrier(0);
                interp_taps(P, b, e, q, t);
                interp_gather<NG>(P, t, g, ga);
                plain_request<NI, U>(P, NI, pn, b, g, raw);
                __builtin_amdgcn_sched_barrier(0);
            }
            store_tile(P, acc, p, b, g, valid);
        };
        auto layer = [&](auto l) { return pw_args_now(ka).layer[decltype(l)::value]; };      // (a layer's fields, read in front of it)
        const float *sbias = pw_args_now(ka).sample_bias;
        f4 a1[V1];
        pw_layer<SPLIT, U, V1, 0>(ws, h, a1, layer(std::integral_constant<int, 0>{}), g, sbias ? sbias + (size_t)b * 16 * V1 : nullptr, true, entered);
        if constexpr (V2 == 0) {
            store(a1);
        } else {
            f4 a2[V2];
            pw_layer<SPLIT, V1, V2, F1>(ws, a1, a2, layer(std::integral_constant<int, 1>{}), g, nullptr, false);
            if constexpr (V3 == 0) {
                store(a2);
            } else {
                f4 a3[V3];
                pw_layer<SPLIT, V2, V3, F1 + F2>(ws, a2, a3, layer(std::integral_constant<int, 2>{}), g, nullptr, false);
                if constexpr (V4 == 0) {
                    store(a3);
                } else {
                    f4 a4[V4];
                    pw_layer<SPLIT, V3, V4, F1 + F2 + F3>(ws, a3, a4, layer(std::integral_constant<int, 3>{}), g, nullptr, false);
                    store(a4);
                }
            }
        }
    };
    while (G + nbx < live_groups) {
        tile(std::true_type{});
        G += nbx;
    }
    tile(std::false_type{});
    ws.finish();
}

// SPLIT: the layers on the fp16 matrix pipe (two pieces per operand, three products per fp32 product, a power-of-two scale per weight
// matrix and per position: fused_common.h, split_mfma.h): same tile, registers and stream, the blob holds split images.
// PIPE: the tile loop software-pipelined (pw_pipelined: rtk_pointwise_mlp_pipelined, the comparison implementation); false: the
// serial loop, which the default entry runs -- measured against each other in one build, the pipelined loop does not pay (DESIGN
// section 4.6).  The two compute the same bits.  The flag selects the body of two kernels: pointwise_mlp_kernel keeps its name and
// its template arguments (the code-object tests look instances up by them), pointwise_mlp_pipelined_kernel runs the pipelined loop.
template <int U, int V1, int V2, int V3, int V4, bool INTERP, bool SPLIT, bool PIPE>
__device__ __forceinline__ void pw_kernel_body(const PwParams &P, PwKernarg<PwParams> ka, f4 *s_w) {
    if constexpr (PIPE) {
        pw_pipelined<U, V1, V2, V3, V4, INTERP, SPLIT>(P, ka, s_w);
        return;
    }
    const int lane = threadIdx.x & 63, j = lane & 15;
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

    for (int G = bx; G < live_groups; G += nbx) {
        asm volatile("" ::: "memory");   // keep loop-invariant loads/addresses inside the loop (registers are the scarce resource)
        int g = lane >> 4;
        asm volatile("" : "+v"(g));      // ... and per-lane addresses (bias fragments, stores) too: hoisted out of the loop they are spilled
        const int r = G * (PW_NW * 16) + wave_in_wg * 16 + j;           // row within the sample
        const bool valid = r < live_rows;
        const int p = b * rps + (r < rps ? r : rps - 1);                  // global row (clamped: out-of-range lanes compute garbage, never stored)

        f4 h[U];
        {
            // 16-channel slot where the plain segments start (wave-uniform)
            auto first_plain = [&]() { return INTERP ? (pw_args_now(ka).interp.channels + 15) >> 4 : 0; };
            // ---- segment 0 (optional): three-NN interpolation, lib/pointnet2_modules.py:141-146 -------------
            if (INTERP) load_interp<U>(pw_args_now(ka), p, b, g, first_plain(), h);
            // ---- plain / per-sample segments: one load per 16-channel slot from the source that owns it ----------
            plain_request<0, U>(pw_args_now(ka), first_plain(), p, b, g, h);      // (requested into the slots they are masked in)
            plain_use<0, U>(pw_args_now(ka), first_plain(), g, h, h);
        }

        // ---- layer chain ------------------------------------------------------------------------------
        // (the first layer enters the weight stream: chunk 0's request has been travelling with the loads above)
        auto layer = [&](auto l) { return pw_args_now(ka).layer[decltype(l)::value]; };      // (a layer's fields, read in front of it)
        auto store = [&](auto &acc) { store_tile(pw_args_now(ka), acc, p, b, g, valid); };
        const float *sbias = pw_args_now(ka).sample_bias;
        f4 a1[V1];
        pw_layer<SPLIT, U, V1, 0>(ws, h, a1, layer(std::integral_constant<int, 0>{}), g, sbias ? sbias + (size_t)b * 16 * V1 : nullptr, true);
        if constexpr (V2 == 0) {
            store(a1);
        } else {
            f4 a2[V2];
            pw_layer<SPLIT, V1, V2, F1>(ws, a1, a2, layer(std::integral_constant<int, 1>{}), g, nullptr, false);
            if constexpr (V3 == 0) {
                store(a2);
            } else {
                f4 a3[V3];
                pw_layer<SPLIT, V2, V3, F1 + F2>(ws, a2, a3, layer(std::integral_constant<int, 2>{}), g, nullptr, false);
                if constexpr (V4 == 0) {
                    store(a3);
                } else {
                    f4 a4[V4];
                    pw_layer<SPLIT, V3, V4, F1 + F2 + F3>(ws, a3, a4, layer(std::integral_constant<int, 3>{}), g, nullptr, false);
                    store(a4);
                }
            }
        }
    }
    ws.finish();
}

template <int U, int V1, int V2, int V3, int V4, bool INTERP, bool SPLIT>
__global__ __launch_bounds__(64 * PW_NW, 2) void pointwise_mlp_kernel(const PwParams P) {
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * PW_F * 64];
    pw_kernel_body<U, V1, V2, V3, V4, INTERP, SPLIT, false>(P, PwKernarg<PwParams>(P), s_w);
}
template <int U, int V1, int V2, int V3, int V4, bool INTERP, bool SPLIT>
__global__ __launch_bounds__(64 * PW_NW, 2) void pointwise_mlp_pipelined_kernel(const PwParams P) {
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * PW_F * 64];
    pw_kernel_body<U, V1, V2, V3, V4, INTERP, SPLIT, true>(P, PwKernarg<PwParams>(P), s_w);
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

// Which instances have a pipelined loop for rtk_pointwise_mlp_pipelined to run (decided from their code objects: no scratch, at most
// 256 registers); the others run the serial loop under either entry point.
template <int U, int V1, int V2, int V3, int V4, bool INTERP>
constexpr bool pw_has_pipe() {
    if (INTERP && U < PW_PIPE_NI) return false;      // the pipelined interpolating instances take a 128-channel segment
    if (!INTERP && U >= 25) return false;            // 100 registers of next input: 256 registers and 28 / 68 bytes of scratch
    if (V2 != 0) return false;                       // the heads: one trip at N = 256, and in the bench's profile the flow head's average
                                                     // rose with the pipelined loop (16.3 -> 20.9 us; serial loop of the same build 15.5)
    return true;
}

template <int U, int V1, int V2, int V3, int V4, bool INTERP, bool SPLIT>
static void launch_pw_instance(const PwParams &P, dim3 blocks, bool pipe, hipStream_t s) {
    if constexpr (pw_has_pipe<U, V1, V2, V3, V4, INTERP>()) {
        if (pipe && (!INTERP || (P.interp.channels + 15) / 16 == PW_PIPE_NI)) {
            pointwise_mlp_pipelined_kernel<U, V1, V2, V3, V4, INTERP, SPLIT><<<blocks, 256, 0, s>>>(P);
            return;
        }
    }
    pointwise_mlp_kernel<U, V1, V2, V3, V4, INTERP, SPLIT><<<blocks, 256, 0, s>>>(P);
}

template <int U, int V1, int V2, int V3, int V4>
static int launch_pw(const PwParams &P0, bool interp, bool split, bool pipe, hipStream_t s) {
    PwParams P = P0;
    const dim3 blocks = pw_grid(P, PW_WGS_TARGET);
    if (interp && split) launch_pw_instance<U, V1, V2, V3, V4, true, true>(P, blocks, pipe, s);
    else if (interp) launch_pw_instance<U, V1, V2, V3, V4, true, false>(P, blocks, pipe, s);
    else if (split) launch_pw_instance<U, V1, V2, V3, V4, false, true>(P, blocks, pipe, s);
    else launch_pw_instance<U, V1, V2, V3, V4, false, false>(P, blocks, pipe, s);
    return 0;
}

static int pointwise_mlp_launch(bool pipe, int rows, int rows_per_sample, const rtk_interp_t *interp, int nsrc,
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
        launch_pw<u, v1, v2, v3, v4>(P, it, split, pipe, s);                     \
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

extern "C" int rtk_pointwise_mlp(int rows, int rows_per_sample, const rtk_interp_t *interp, int nsrc,
                                 const rtk_src_t *srcs, const float *sample_bias, int nlayers,
                                 const rtk_layer_t *layers, float *out, int out_pitch, int out_channels,
                                 int out_channel_major, const int *row_nuniq, float *colmax, rtk_stream_t stream) {
    return pointwise_mlp_launch(false, rows, rows_per_sample, interp, nsrc, srcs, sample_bias, nlayers, layers, out, out_pitch, out_channels,
                                out_channel_major, row_nuniq, colmax, stream);
}

extern "C" int rtk_pointwise_mlp_pipelined(int rows, int rows_per_sample, const rtk_interp_t *interp, int nsrc,
                                           const rtk_src_t *srcs, const float *sample_bias, int nlayers,
                                           const rtk_layer_t *layers, float *out, int out_pitch, int out_channels,
                                           int out_channel_major, const int *row_nuniq, float *colmax, rtk_stream_t stream) {
    return pointwise_mlp_launch(true, rows, rows_per_sample, interp, nsrc, srcs, sample_bias, nlayers, layers, out, out_pitch, out_channels,
                                out_channel_major, row_nuniq, colmax, stream);
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

__device__ __forceinline__ void pw_globalize(TapParams &T) {
    pw_globalize(T.pw);
    pw_global(T.proj_w[0]); pw_global(T.proj_w[1]); pw_global(T.proj_b[0]); pw_global(T.proj_b[1]); pw_global(T.pout);
}

// PIPE: the tile loop software-pipelined by one group, as pw_pipelined does for an interpolating chain: the next group's three-NN
// row is requested when the tile has entered the stream, its known rows under the projection's second half (the layer's
// accumulators are dead by then); every group is live here (rtk_pointwise_mlp_tap_pipelined, the comparison implementation).
// false: the serial loop, which the default entry runs.
template <int U, int V1, int VP, bool PIPE>
__global__ __launch_bounds__(64 * PW_NW, 2) void pointwise_tap_kernel(const TapParams T) {
    const PwKernarg<TapParams> ka(T);
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

    if constexpr (PIPE) {
        const int rw = wave_in_wg * 16 + j;
        auto row_of = [&](int G) { const int r = G * (PW_NW * 16) + rw; return b * rps + (r < rps ? r : rps - 1); };
        const int e = P.interp.nuniq ? P.interp.nuniq[b] : 0x7fffffff;
        InterpRow q;
        InterpTaps t;
        f4 ga[3][U];
        const int g0 = g;
        interp_request(P, row_of(bx), q);
        interp_taps(P, b, e, q, t);
        interp_gather<U>(P, t, g0, ga);
        int G = bx;
        auto tile = [&](auto more) {
            constexpr bool MORE = decltype(more)::value;
            asm volatile("" ::: "memory");
            int g = g0;
            asm volatile("" : "+v"(g));     // (pw_pipelined: per-lane addresses are formed in the tile)
            const TapParams T = pw_args_now(ka);      // (... and the arguments read in the trip)
            const PwParams &P = T.pw;
            const bool valid = G * (PW_NW * 16) + rw < rps;
            const int p = row_of(G);
            f4 h[U];
            interp_combine<U, U>(P, t, g, ga, h);
            f4 a1[V1];
            {
                const LaneScale s1 = lane_scale16(h);
                init_zero<V1>(a1);
                ws.next();
                if constexpr (MORE) {
                    interp_request(P, row_of(G + nbx), q);
                    __builtin_amdgcn_sched_barrier(0);      // (the requests stay here: the scheduler otherwise moves them down to their first use)
                }
                mlp_layer_split_impl<U, V1, 0, decltype(ws), PW_F>(ws, h, s1.s, a1, std::make_integer_sequence<int, ((U + 1) / 2) * ((V1 + 1) / 2)>{});
                scale_bias<V1>(a1, s1.inv * P.layer[0].inv_scale, P.layer[0].bias, g);
                apply_act<V1>(a1, P.layer[0].act);
            }
            store_tile<V1>(P, a1, p, b, g, valid);
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
            if constexpr (MORE) {
                const TapParams T2 = pw_args_now(ka);
                __builtin_amdgcn_sched_barrier(0);
                interp_taps(T2.pw, b, e, q, t);
                interp_gather<U>(T2.pw, t, g, ga);
                __builtin_amdgcn_sched_barrier(0);
            }
            half(std::integral_constant<int, 1>{});
        };
        while (G + nbx < groups) {
            tile(std::true_type{});
            G += nbx;
        }
        tile(std::false_type{});
        ws.finish();
        return;
    }
    const int g_lane = g;
    for (int G = bx; G < groups; G += nbx) {
        asm volatile("" ::: "memory");
        int g = g_lane;
        asm volatile("" : "+v"(g));         // (per-lane addresses are formed in the trip, the arguments read in it: pw_args_now)
        const TapParams T = pw_args_now(ka);
        const PwParams &P = T.pw;
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

static int pointwise_mlp_tap_launch(bool pipe, int rows, int rows_per_sample, const rtk_interp_t *interp, const rtk_layer_t *layer, float *out,
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
    if (pipe) pointwise_tap_kernel<8, 8, 16, true><<<blocks, 64 * PW_NW, 0, (hipStream_t)stream>>>(T);
    else pointwise_tap_kernel<8, 8, 16, false><<<blocks, 64 * PW_NW, 0, (hipStream_t)stream>>>(T);
    RTK_CHECK_LAUNCH("pointwise_mlp_tap");
    return RTK_OK;
}

extern "C" int rtk_pointwise_mlp_tap(int rows, int rows_per_sample, const rtk_interp_t *interp, const rtk_layer_t *layer, float *out,
                                     int out_pitch, float *colmax, const rtk_layer_t *proj, int frame_split, float *proj_out, int proj_pitch,
                                     rtk_stream_t stream) {
    return pointwise_mlp_tap_launch(false, rows, rows_per_sample, interp, layer, out, out_pitch, colmax, proj, frame_split, proj_out, proj_pitch,
                                    stream);
}

extern "C" int rtk_pointwise_mlp_tap_pipelined(int rows, int rows_per_sample, const rtk_interp_t *interp, const rtk_layer_t *layer, float *out,
                                               int out_pitch, float *colmax, const rtk_layer_t *proj, int frame_split, float *proj_out,
                                               int proj_pitch, rtk_stream_t stream) {
    return pointwise_mlp_tap_launch(true, rows, rows_per_sample, interp, layer, out, out_pitch, colmax, proj, frame_split, proj_out, proj_pitch,
                                    stream);
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
