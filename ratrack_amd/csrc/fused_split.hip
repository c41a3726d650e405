// fused_split.hip -- kernels on the split matrix path (split_mfma.h): fp32 results from v_mfma_f32_32x32x16_f16, two fp16 pieces
// per operand, three products, a power-of-two scale per weight matrix and per position.
#include "rtk_common.h"
#include "rtk_fused.h"
#include "split_mfma.h"

namespace {

#ifndef SP_NW
#define SP_NW 4           // waves per workgroup = one per SIMD: the tile keeps ~400 registers per lane
#endif
#ifndef SP_F
#define SP_F 32           // fragments (KiB) per half of the LDS double buffer: a power of two (a layer is 256 fragments)
#endif
// The forward cost volume streams in halves of 32 KiB (eight group steps of six MFMAs per chunk: the 1 536 matrix clocks the
// 24 KiB halves of the six-product kernel lasted), next to the 64 KiB of staged rows of layer 1.
constexpr int CV_F = 32;

// ---- packing: (cout x cin) row-major fp32 weights -> split image + the inverse of its power-of-two scale (split_mfma.h) ---------
// Every workgroup scans the whole matrix for max|w| itself (at most 256 KiB, L2-resident: one launch, no atomics, no scratch).
// TILE16: the fragment order of the 16-position tile (fused_common.h) -- 16-row blocks, k-steps of 32:
// frag[up][v][p][lane = 16 g + i][t] = piece_p(2^k W[16 v + i][32 up + 16 (t / 4) + 4 g + t % 4]); the same scale, the same pieces.
template <bool TILE16>
__global__ __launch_bounds__(256) void pack_split_kernel(int cout, int cin, const float *__restrict__ w, int transposed, u4v *__restrict__ out,
                                                         float *__restrict__ inv_scale) {
    __shared__ unsigned s_m[4];
    float m = 0.f;
    const f4 *w4 = reinterpret_cast<const f4 *>(w);
    for (int i = threadIdx.x; i < cout * cin / 4; i += 256) {
        const f4 t = w4[i];
        m = __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fabsf(t.x)), __builtin_fabsf(t.y));
        m = __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fabsf(t.z)), __builtin_fabsf(t.w));
    }
    unsigned mb = __float_as_uint(m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned o = __shfl_xor(mb, d, 64); mb = o > mb ? o : mb; }
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mb;
    __syncthreads();
    mb = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
    const LaneScale sc = lane_scale_of(mb);
    if (blockIdx.x == 0 && threadIdx.x == 0) *inv_scale = sc.inv;
    const int VB = cout / (TILE16 ? 16 : 32), slot = blockIdx.x * 256 + threadIdx.x;      // slot = (s, v, lane)
    if (slot >= (cin / (TILE16 ? 32 : 16)) * VB * 64) return;
    const int lane = slot & 63, v = (slot >> 6) % VB, s = (slot >> 6) / VB, hh = lane >> 5, i = lane & 31;
    // this slot: W[o][c0 .. c0 + 3], W[o][c0 + C1 .. c0 + C1 + 3]
    constexpr int C1 = TILE16 ? 16 : 8;
    const int o = TILE16 ? 16 * v + (lane & 15) : 32 * v + i, c0 = TILE16 ? 32 * s + 4 * (lane >> 4) : 32 * (s >> 1) + 16 * (s & 1) + 4 * hh;
    f4 x0, x1;
    if (transposed) {                                                          // W = w^T, w (cin, cout) row-major
#pragma unroll
        for (int r = 0; r < 4; ++r) { x0[r] = w[(size_t)(c0 + r) * cout + o]; x1[r] = w[(size_t)(c0 + C1 + r) * cout + o]; }
    } else {
        const float *row = w + (size_t)o * cin + c0;
        x0 = *reinterpret_cast<const f4 *>(row); x1 = *reinterpret_cast<const f4 *>(row + C1);
    }
    u4v b[2];
    split2(x0, x1, sc.s, b);
#pragma unroll
    for (int p = 0; p < 2; ++p) out[((size_t)(s * VB + v) * 2 + p) * 64 + lane] = b[p];
}

// y = leaky(acc c + b) for a whole accumulator set (c = this lane's 2^-(kw + kx)): the epilogue between two split layers
__device__ __forceinline__ f4 leaky_med4(f4 t, float inf) {
    const f4 u = t * 0.1f;                                                  // two v_pk_mul_f32
    return (f4){__builtin_amdgcn_fmed3f(t.x, u.x, inf), __builtin_amdgcn_fmed3f(t.y, u.y, inf), __builtin_amdgcn_fmed3f(t.z, u.z, inf),
                __builtin_amdgcn_fmed3f(t.w, u.w, inf)};
}
__device__ __forceinline__ f4 scale_bias4(f4 a, float c, f4 b) { return __builtin_elementwise_fma(a, (f4){c, c, c, c}, b); }

// ---- two 256 x 256 layers with LeakyReLU(0.1) over a list of positions (the inner layers of the cost volume, standalone) ----
__global__ __launch_bounds__(64 * SP_NW) __attribute__((amdgpu_waves_per_eu(1, 1)))
void split_mlp2_kernel(int positions, const float *__restrict__ x, const f4 *__restrict__ blob, const float *__restrict__ wsc,
                       const float *__restrict__ bias1, const float *__restrict__ bias2, float *__restrict__ y) {
    const float kinf = rtk_hidden_inf();
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * SP_F * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5, col = lane & 31;
    constexpr int NF = 2 * SPLIT_NF;
    WStreamA<SP_NW, SP_F, NF> ws;
    ws.start_parts(blob, s_w, wave, lane);
    const float wi1 = ldc(wsc), wi2 = ldc(wsc + 1);
    const int tiles = (positions + 32 * SP_NW - 1) / (32 * SP_NW);
    for (int T = blockIdx.x; T < tiles; T += gridDim.x) {
        asm volatile("" ::: "memory");
        const long pos = (long)T * 32 * SP_NW + 32 * wave + col;
        const bool valid = pos < positions;
        const float *xr = x + (valid ? pos : (long)positions - 1) * 256 + 4 * hh;
        f4 h[32], bq[2][8];
#pragma unroll
        for (int i = 0; i < 32; ++i) h[i] = *reinterpret_cast<const f4 *>(xr + 8 * i);      // channels 32 (i/4) + 8 (i%4) + 4 hh ..
        f16v acc[SPLIT_VB];
        LaneScale sc = lane_scale32(h);
        split_layer<0>(ws, h, sc.s, acc, BiasSide{bias1 + 4 * hh, bq});
        float c = sc.inv * wi1;
        split_epilogue(acc, bias1 + 4 * hh, bq, [&](int e, f4 a, f4 b) { h[e] = leaky_med4(scale_bias4(a, c, b), kinf); });
        sc = lane_scale32(h);
        split_layer<SPLIT_NF>(ws, h, sc.s, acc, BiasSide{bias2 + 4 * hh, bq});
        ws.sync();
        c = sc.inv * wi2;
        float *yr = y + pos * 256 + 4 * hh;
        split_epilogue(acc, bias2 + 4 * hh, bq, [&](int e, f4 a, f4 b) {
            if (valid) *reinterpret_cast<f4 *>(yr + 8 * e) = leaky_med4(scale_bias4(a, c, b), kinf);
        });
    }
    ws.finish();
}

// ---- rtk_cost_volume on the split path ------------------------------------------------------------------------------------
// Same operator as cost_volume_kernel (fused_group.hip); a wave owns TWO query points x their 16 neighbours (the 32 columns of
// the 32x32 tile), a workgroup (one wave per SIMD) eight points per iteration.  Layer 1 (K = 3) and the WeightNet's last
// layer (K = 8) stay on the fp32-input MFMA (v_mfma_f32_32x32x2_f32, same C/D layout); the two 256 x 256 layers -- 99 % of the
// flops -- run split.
struct CvSplitParams {
    int samples, n1, n2, gx;
    const float *xyz1, *xyz2;
    const int64_t *knn;
    const float *p1, *p2;
    const float *st;              // optional (samples, 256): per-sample term of layer 1, added to the p1 row of each point of the sample
    const float *wd;              // [16][64] image of [Wd | 0] (fused_common.h): Wd[c][k] = wd[(c / 16) * 64 + 16 k + c % 16]
    const f4 *blob;               // split images of layers 2, 3 ...
    const float *wsc;             // ... and the inverses of their power-of-two weight scales (rtk_pack_split_layer)
    const float *bias2, *bias3;
    WnSplit wn;
    float *out;
    int out_pitch;
    float *amax;                  // training kernels: [2] zero-initialised, the largest |element| of (a1, a2) -- forward -- / (dz3, dz2) -- backward
    float *sv1, *sv2, *sv3;       // training forward (SAVE): the three activations (positions, 256) ...
    uint2 *mk1, *mk2;             // ... and the sign masks of a1, a2 in the format of cost_volume_kernel<true> (fused_group.hip): word
                                  // (position, g), bit 4 v16 + r = [a[channel 16 v16 + 4 g + r] > 0]
};

// This lane's channels 32 v + 8 q + 4 hh + r are the 16-wide kernels' (v16 = 2 v + q / 2, g = 2 (q % 2) + hh, r): it owns the two
// complete mask words g = hh (q even) and g = 2 + hh (q odd) of its position.
__device__ __forceinline__ void split_sign_masks(const f4 (&a)[32], uint2 (&m)[2]) {
    m[0] = m[1] = make_uint2(0u, 0u);
#pragma unroll
    for (int v = 0; v < SPLIT_VB; ++v)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned bit = (a[4 * v + q][r] > 0.f ? 1u : 0u) << (4 * ((2 * v + (q >> 1)) & 7) + r);
                if (v < 4) m[q & 1].x |= bit; else m[q & 1].y |= bit;
            }
}
__device__ __forceinline__ unsigned split_mask_bits(const uint2 (&m)[2], int v, int q) {      // [z > 0] of (v, q, r = 0..3) in the low four bits
    return ((v < 4 ? m[q & 1].x : m[q & 1].y) >> (4 * ((2 * v + (q >> 1)) & 7))) & 15u;
}

__device__ __forceinline__ f4 *cv_at(float *base, unsigned byte_off) { return reinterpret_cast<f4 *>(reinterpret_cast<char *>(base) + byte_off); }
__device__ __forceinline__ const f4 *cv_at(const float *base, unsigned byte_off) {
    return reinterpret_cast<const f4 *>(reinterpret_cast<const char *>(base) + byte_off);
}

// (the WeightNet's hidden layers, wn_hidden: wn_tile.h)
// relu(Wc.t2 + bc) for the 32-channel block v in the tile layout (K = 8 on the fp32-input MFMA: four k-steps of two), in two
// halves: this lane's operands of the block (bias, four weights: 20 registers), and the product.  The epilogues request block
// v + 1's operands before they work on block v -- the conditional stores of a block end a basic block each, and hipcc's scheduler
// moves no load across them, so every block started with an exposed round trip.
struct WnBlock {
    f16v bias;
    float w[4];
};
__device__ __forceinline__ WnBlock wn_block(const WnSplit &W, int v, int hh, int col) {
    WnBlock k;
    k.bias = split_bias(W.bc, v, hh);
    const int ch = 32 * v + col;                                         // A[i = col][k = hh]
    const float *wr = W.wc + ((ch >> 4) * 64 + (ch & 15)) * 4;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const int kk = 2 * st + hh;
        k.w[st] = ldc(wr + 64 * (kk >> 2) + (kk & 3));
    }
    return k;
}
__device__ __forceinline__ f16v wn_pre(const WnBlock &k, int hh, const float (&t2)[8]) {      // Wc.t2 + bc, before the ReLU
    f16v w = k.bias;
#pragma unroll
    for (int st = 0; st < 4; ++st) w = mfma_f32x2(k.w[st], hh ? t2[2 * st + 1] : t2[2 * st], w);
    return w;
}
// (relu1 / relu_med4, the one-instruction ReLU on a hidden +inf: wn_tile.h)

// CV_LDS_HIDDEN: the WeightNet's hidden weights (104 words, wave-uniform) in the image too, read as broadcasts into vector registers
// instead of four 16-word scalar loads per tile into scalar registers the kernel does not have (they were spilled to lanes and back).
#ifndef CV_LDS_HIDDEN
#define CV_LDS_HIDDEN 1
#endif
// CV_WN_AHEAD: how many output blocks ahead of their use the epilogue requests a block's WeightNet operands from the LDS image (2: the
// distance the global loads needed; 1: the block's operands are read at the top of the block before it).
#ifndef CV_WN_AHEAD
#define CV_WN_AHEAD 2
#endif
// ---- the forward kernel's constants, resident in LDS ----------------------------------------------------------------------------
// What every tile of every workgroup reads and no tile owns -- layer 1's direction weights, the WeightNet's output layer and the three
// 256-channel biases, 15 KiB -- is copied into LDS once per workgroup, permuted so that a lane's read in the tile loop is one ds_read at
// an immediate offset from a per-lane base (lane * 4 for the A operands, 16 hh for the biases) instead of a global load behind 64-bit
// address arithmetic.  A operands: [block v][k-step][lane], 64 consecutive words per read; biases: channel order, so that the slot
// channels 32 v + 8 q + 4 hh .. + 3 is ONE 16-byte read with two distinct addresses per instruction (hh = 0, 1: broadcasts).
struct CvConsts {
    float wd[SPLIT_VB * 2 * 64];      // A[i = col][k = hh] of block v's two k-steps of [Wd | 0]: what ldc(wr + 16 (2 k + hh)) of cv_layer1_blocks reads
    float wc[SPLIT_VB * 4 * 64];      // ... of block v's four k-steps of Wc: WnBlock::w[st]
    float bc[256], bias2[256], bias3[256];
#if CV_LDS_HIDDEN
    float hid[128];                   // the WeightNet's hidden layers: [Wa | ba] as [k][o] (32), Wb as [o][c] (64), bb (8); every lane reads the same word
#endif
};
static_assert(sizeof(CvConsts) == 15 * 1024 + (CV_LDS_HIDDEN ? 512 : 0), "4 + 8 + 3 KiB (+ the hidden layers)");
// The fill in two halves: four 16-byte loads per thread (the biases by waves 0..2, one each), and the permuting stores.
struct CvConstsFill {
    f4 wd, wc[2], bias;
    float hid;
};
__device__ __forceinline__ CvConstsFill cv_consts_load(const float *wd, const WnSplit &W, const float *bias2, const float *bias3, int wave, int lane) {
    CvConstsFill k;
    const int t = wave * 64 + lane;
    k.wd = ldc4(wd + 4 * t);                                             // [g = channel / 16][m = 2 k + hh][channel % 16]: words 4 t .. 4 t + 3
#pragma unroll
    for (int n = 0; n < 2; ++n) {                                        // the live half of the image (k < 8): 512 slots (g, k / 4, channel % 16) of four k
        const int u = 256 * n + t;
        k.wc[n] = ldc4(W.wc + (u >> 5) * 256 + ((u >> 4) & 1) * 64 + (u & 15) * 4);
    }
    const float *bs = wave == 0 ? W.bc : wave == 1 ? bias2 : bias3;      // (wave-uniform; wave 3's copy is not stored)
    k.bias = ldc4(bs + 4 * lane);
#if CV_LDS_HIDDEN
    {
        const int u = t < 32 ? 0 : t - 32, o = u >> 3, c = u & 7;          // threads 0..31: wa, 32..95: wb, 96..103: bb (the others: a word nobody stores)
        const float *hs = t < 32 ? W.wa + 16 * (t >> 3) + (t & 7) : t < 96 ? W.wb + (16 * (c >> 2) + o) * 4 + (c & 3) : W.bb + (t < 104 ? t - 96 : 0);
        k.hid = ldc(hs);
    }
#endif
    return k;
}
__device__ __forceinline__ void cv_consts_store(CvConsts &C, const CvConstsFill &k, int wave, int lane) {
    const int t = wave * 64 + lane;
    {
        const int g = t >> 4, m = (t >> 2) & 3;                          // block g / 2, columns 16 (g % 2) + 4 (t % 4) .. + 3, k-step m / 2, hh = m % 2
        *reinterpret_cast<f4 *>(C.wd + ((g >> 1) * 2 + (m >> 1)) * 64 + (m & 1) * 32 + (g & 1) * 16 + 4 * (t & 3)) = k.wd;
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int u = 256 * n + t, g = u >> 5, kq = (u >> 4) & 1, c15 = u & 15;
#pragma unroll
        for (int k3 = 0; k3 < 4; ++k3)                                   // k = 4 kq + k3 = 2 st + hh
            C.wc[((g >> 1) * 4 + 2 * kq + (k3 >> 1)) * 64 + (k3 & 1) * 32 + (g & 1) * 16 + c15] = k.wc[n][k3];
    }
    if (wave < 3) *reinterpret_cast<f4 *>((wave == 0 ? C.bc : wave == 1 ? C.bias2 : C.bias3) + 4 * lane) = k.bias;
#if CV_LDS_HIDDEN
    if (t < 104) C.hid[t] = k.hid;
#endif
}
#if CV_LDS_HIDDEN
// wn_hidden (wn_tile.h, ascending order) on the LDS image: the same operations on the same values
__device__ __forceinline__ void wn_hidden_lds(const CvConsts &C, float dx, float dy, float dz, float (&t2)[8]) {
    float t1[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = __fmaf_rn(C.hid[o], dx, 0.f);
        a = __fmaf_rn(C.hid[8 + o], dy, a);
        a = __fmaf_rn(C.hid[16 + o], dz, a);
        t1[o] = fmaxf(__fadd_rn(a, C.hid[24 + o]), 0.f);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = C.hid[96 + o];
#pragma unroll
        for (int c = 0; c < 8; ++c) a = __fmaf_rn(C.hid[32 + 8 * o + c], t1[c], a);
        t2[o] = fmaxf(a, 0.f);
    }
}
#endif
// wn_block / split_bias from the LDS image: the same values into the same registers
__device__ __forceinline__ WnBlock wn_block_lds(const CvConsts &C, int v, int hh, int lane) {
    WnBlock k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f4 t = *reinterpret_cast<const f4 *>(C.bc + 32 * v + 8 * q + 4 * hh);
        k.bias[4 * q] = t.x; k.bias[4 * q + 1] = t.y; k.bias[4 * q + 2] = t.z; k.bias[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) k.w[st] = C.wc[(4 * v + st) * 64 + lane];
    return k;
}

// ---- layer 1's operands ---------------------------------------------------------------------------------------------------
// The tile layout gives a lane 32 bytes of a gathered p2 row per load instruction (its own position's row, two lanes per position):
// 32 partial cache lines per instruction, each fetched whole from L2 and -- four instructions in a row touching the same line
// while it is still in flight -- fetched again (tools/experiments/cv_ticks.py: 12 k of a tile's 86 k clocks went into layer 1, 6 k
// of them gone when every lane reads the same row).  So the rows come through LDS instead: one global_load_lds per two positions
// moves 2 x 512 contiguous bytes (channels 128 HALF .. 128 HALF + 127 of both rows) into the wave's own 16 KiB of LDS, every line
// fetched once, and the lanes read their slots from there.  Two rounds per tile (HALF = 0, 1: 64 KiB per workgroup next to the
// weight stream's 64 and the 15 KiB of constants); round 0 of the NEXT tile is requested right after layer 1 and lands under layers 2 and 3.
// Slot p of a position's 512 bytes holds source chunk p ^ (position & 15): the 16 lanes that read together (one hh, 16 positions)
// then hit 16 different bank groups.
constexpr int CV_ROWS_F4 = 32 * 32;      // f4 per wave: 32 positions x 32 slots of 16 bytes
struct CvRowsRequest {
    const char *p2;                // the p2 rows (wave-uniform; byte offsets are 32-bit: at most 2^22 rows)
    f4 *rows;                      // this wave's 16 KiB
    int nbrow;                     // this lane's gathered row (lane col and lane 32 + col hold the same)
    unsigned lanepart;             // 512 HALF + ((slot ^ sub) << 4): (slot ^ ((2 t + sub) & 15)) << 4 == lanepart ^ ((2 t & 15) << 4) below 512
    int sub;
    __device__ __forceinline__ CvRowsRequest(const float *p2_, f4 *rows_, int nbrow_, int half, int lane)
        : p2(reinterpret_cast<const char *>(p2_)), rows(rows_), nbrow(nbrow_), lanepart(512u * half + (unsigned)(((lane & 31) ^ (lane >> 5)) << 4)), sub(lane >> 5) {}
    // lanes 0..31: position 2 T, lanes 32..63: position 2 T + 1 (their row indices live in lanes 2 T, 2 T + 1)
    template <int T>
    __device__ __forceinline__ void one() const {
        const int r0 = __builtin_amdgcn_readlane(nbrow, 2 * T), r1 = __builtin_amdgcn_readlane(nbrow, 2 * T + 1);
        const unsigned off = ((unsigned)(sub ? r1 : r0) << 10) + (lanepart ^ (unsigned)(((2 * T) & 15) << 4));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(p2 + off),
                                         (__attribute__((address_space(3))) void *)(rows + T * 64), 16, 0, 0);
    }
    template <int... T>
    __device__ __forceinline__ void all(std::integer_sequence<int, T...>) const { (one<T>(), ...); }
};
template <int HALF>
__device__ __forceinline__ void cv_rows_request(const float *p2, int nbrow, f4 *rows, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the previous round's reads have returned before their slots are overwritten
    CvRowsRequest(p2, rows, nbrow, HALF, lane).all(std::make_integer_sequence<int, 16>{});
}
// Side job of layer 2 (split_mfma.h): the NEXT tile's round 0, three requests in each of the first group steps of the layer's first two
// chunks -- where the weight stream issues its own, so that they are as old as those at the chunk's closing vmcnt(0) -- and, in the
// training forward, the a1 stores.
template <bool SAVE>
struct CvLayer2Side {
    StoreRowsSide st;
    CvRowsRequest rq;
    template <int GI>
    __device__ __forceinline__ void at(const f4 (&h)[32]) const {
        if constexpr (SAVE) st.template at<GI>(h);
        constexpr int per_chunk = CV_F / SPLIT_GF, ig = split_issue_groups(CV_F), g = GI % per_chunk, n = (GI / per_chunk) * ig + g;
        if constexpr (g < ig && 3 * n < 16) {
            rq.template one<3 * n>();
            if constexpr (3 * n + 1 < 16) rq.template one<3 * n + 1>();
            if constexpr (3 * n + 2 < 16) rq.template one<3 * n + 2>();
        }
    }
};
// this lane's 16 slots of the round: channels 128 HALF + 8 e + 4 hh .. + 3, e = 0..15
template <int HALF>
__device__ __forceinline__ void cv_rows_read(const f4 *rows, int col, int hh, f4 (&h)[32]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) h[16 * HALF + e] = rows[col * 32 + ((2 * e + hh) ^ (col & 15))];
}
// r + q as held by lane K of this lane's row of 16 (the p1 row of a point is the same for its 16 neighbours: each of them loads
// two of its 32 slots and the additions pick the owner's copy -- 2 loads per lane instead of 32 returning the same bytes 16 times)
template <int K>
__device__ __forceinline__ f4 add_row_bcast(const f4 q, const f4 r) {
    f4 o;
    asm("s_nop 1\n"
        "v_add_f32_dpp %0, %4, %8 row_newbcast:%12 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %1, %5, %9 row_newbcast:%12 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %2, %6, %10 row_newbcast:%12 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %3, %7, %11 row_newbcast:%12 row_mask:0xf bank_mask:0xf"
        : "=&v"(o.x), "=&v"(o.y), "=&v"(o.z), "=&v"(o.w)
        : "v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w), "v"(r.x), "v"(r.y), "v"(r.z), "v"(r.w), "n"(K));
    return o;
}
// r * q as held by lane K of this lane's row of 16 (the backward's dout row: the same for a point's 16 neighbours)
template <int K>
__device__ __forceinline__ f4 mul_row_bcast(const f4 q, const f4 r) {
    f4 o;
    asm("s_nop 1\n"
        "v_mul_f32_dpp %0, %4, %8 row_newbcast:%12 row_mask:0xf bank_mask:0xf\n"
        "v_mul_f32_dpp %1, %5, %9 row_newbcast:%12 row_mask:0xf bank_mask:0xf\n"
        "v_mul_f32_dpp %2, %6, %10 row_newbcast:%12 row_mask:0xf bank_mask:0xf\n"
        "v_mul_f32_dpp %3, %7, %11 row_newbcast:%12 row_mask:0xf bank_mask:0xf"
        : "=&v"(o.x), "=&v"(o.y), "=&v"(o.z), "=&v"(o.w)
        : "v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w), "v"(r.x), "v"(r.y), "v"(r.z), "v"(r.w), "n"(K));
    return o;
}
__device__ __forceinline__ f4 add4_rn(const f4 a, const f4 b) {
    return (f4){__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w)};
}
template <int V0, int V1, bool LDSC>
__device__ __forceinline__ void cv_layer1_blocks(const CvSplitParams &P, const CvConsts &C, const f4 q0, const f4 q1, float b0, float b1, int hh, int col, float kinf, f4 (&h)[32]) {
    static_assert(V1 <= 8, "eight 32-channel blocks");
    auto block = [&](auto vc) {
        constexpr int v = decltype(vc)::value;
        f16v c;
        auto slot = [&](auto qc) {
            constexpr int q = decltype(qc)::value, e = 4 * v + q;
            const f4 t = add_row_bcast<e & 15>(e < 16 ? q0 : q1, h[e]);
            c[4 * q] = t.x; c[4 * q + 1] = t.y; c[4 * q + 2] = t.z; c[4 * q + 3] = t.w;
        };
        slot(std::integral_constant<int, 0>{}); slot(std::integral_constant<int, 1>{});
        slot(std::integral_constant<int, 2>{}); slot(std::integral_constant<int, 3>{});
        float a0, a1;                                        // A[i = col][k = hh] of the two k-steps
        if constexpr (LDSC) {
            a0 = C.wd[(2 * v) * 64 + 32 * hh + col]; a1 = C.wd[(2 * v + 1) * 64 + 32 * hh + col];
        } else {
            const int ch = 32 * v + col;
            const float *wr = P.wd + (ch >> 4) * 64 + (ch & 15);
            a0 = ldc(wr + 16 * hh); a1 = ldc(wr + 16 * (2 + hh));
        }
        c = mfma_f32x2(a0, b0, c);
        c = mfma_f32x2(a1, b1, c);
#pragma unroll
        for (int q = 0; q < 4; ++q) h[4 * v + q] = leaky_med4((f4){c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]}, kinf);
    };
    block(std::integral_constant<int, V0>{}); block(std::integral_constant<int, V0 + 1>{});
    block(std::integral_constant<int, V0 + 2>{}); block(std::integral_constant<int, V0 + 3>{});
}

// Register cap of the forward kernel.  Left alone (512) hipcc spreads the tile over 500 registers and nothing else fits on the SIMD;
// capped it allocates 404 without a spill, and the small-register geometry kernels of the other batches in flight (FPS 20, ball
// query 16, three-NN 12, kNN 40 registers) can share the SIMDs with it: +0.7 % frame-pairs/s, the kernel alone unchanged.
// (Round 6: with the hipcc of ROCm 7.2 the attribute no longer binds -- the code object reports .vgpr_count 496 (256 + 240 accumulation
// registers) for any cap from 320 to 512, with or without amdgpu_waves_per_eu: one wave owns the SIMD's register file.)
#ifndef CV_FWD_VGPRS
#define CV_FWD_VGPRS 448
#endif
// LDSC: the constants come from the LDS image (CvConsts); false: from global memory on every tile, the kernel as it was before the
// image existed -- kept as the comparison implementation (rtk_cost_volume_split_gconst), same arithmetic on the same values.
template <bool SAVE, bool LDSC = true>
__global__ __launch_bounds__(64 * SP_NW) __attribute__((amdgpu_waves_per_eu(1, 1), amdgpu_num_vgpr(CV_FWD_VGPRS)))
void cost_volume_split_kernel(const CvSplitParams P) {
    const float kinf = rtk_hidden_inf();
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * CV_F * 64];
    __shared__ __attribute__((aligned(16))) f4 s_rows[SP_NW * CV_ROWS_F4];
    __shared__ __attribute__((aligned(16))) CvConsts s_c;      // (LDSC; 64 + 64 + 15 KiB of the CU's 160: the registers give the workgroup the CU anyway)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5, col = lane & 31, pp = col >> 4,
              j = col & 15;      // wave index in an SGPR: the DMA's LDS destination (M0) is then scalar arithmetic
    f4 *rows = s_rows + wave * CV_ROWS_F4;
    constexpr int PPW = 2 * SP_NW;                                  // points per workgroup iteration
    const int groups = (P.n1 + PPW - 1) / PPW;
    // Tiles = (sample, group of eight points).  P.gx > 0 (samples % 8 == 0): a 1-D grid of P.gx workgroups, ALL tiles of sample s on
    // XCD s % 8 -- workgroup L serves XCD L % 8 and strides over that XCD's tiles (sample-major) with the XCD's P.gx / 8 workgroups,
    // so that the launcher can give the kernel any share of the CUs (cv_split_fill).  Else a plain 2-D grid, one sample per row.
    const bool flat = P.gx > 0;
    const int xcd = blockIdx.x & 7, t0 = flat ? (int)(blockIdx.x >> 3) : (int)blockIdx.x, tstep = flat ? P.gx >> 3 : (int)gridDim.x;
    const int ntiles = flat ? (P.samples >> 3) * groups : groups;
    auto locate = [&](int t, int &b_, int &G_) {
        if (flat) { const int sk = t / groups; b_ = sk * 8 + xcd; G_ = t - sk * groups; }
        else { b_ = blockIdx.y; G_ = t; }
    };
    int b, bx;
    locate(t0 < ntiles ? t0 : 0, b, bx);
    WStreamA<SP_NW, CV_F, 2 * SPLIT_NF> ws;
    // The constants' loads travel with the stream's first chunk; their stores and barrier come after start_parts' own, by every thread of
    // every workgroup (also one that has no tile).
    CvConstsFill cfill;
    if constexpr (LDSC) cfill = cv_consts_load(P.wd, P.wn, P.bias2, P.bias3, wave, lane);
    ws.start_parts(P.blob, s_w, wave, lane);
    if constexpr (LDSC) {
        cv_consts_store(s_c, cfill, wave, lane);
        __syncthreads();
    }
    const float *bias2 = (LDSC ? s_c.bias2 : P.bias2) + 4 * hh, *bias3 = (LDSC ? s_c.bias3 : P.bias3) + 4 * hh;
    auto wnb = [&](int v) {
        if constexpr (LDSC) return wn_block_lds(s_c, v, hh, lane);
        else return wn_block(P.wn, v, hh, col);
    };
    const float wi2 = ldc(P.wsc), wi3 = ldc(P.wsc + 1);
    // The tile loop is software-pipelined by one tile (round 4): the NEXT tile's neighbour index is requested at the top of the
    // CURRENT tile, the first half of its gathered rows (cv_rows_request<0>) right after layer 1, its direction and its two p1 slots
    // inside the epilogue, whose WeightNet / neighbour-sum arithmetic (VALU + DPP) runs while they arrive.
    int pt = bx * PPW + 2 * wave + pp;
    bool valid = pt < P.n1;
    long i = (long)b * P.n1 + (valid ? pt : P.n1 - 1);
    long nb = 0;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    f4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0;                          // p1 slots j and 16 + j of this lane's point
    if (t0 < ntiles) {
        nb = (long)b * P.n2 + (long)P.knn[i * 16 + j];
        cv_rows_request<0>(P.p2, (int)nb, rows, lane);
        q0 = ldc4(P.p1 + i * 256 + 4 * hh + 8 * j); q1 = ldc4(P.p1 + i * 256 + 4 * hh + 8 * (16 + j));
        if (P.st) { q0 = add4_rn(q0, ldc4(P.st + b * 256 + 4 * hh + 8 * j)); q1 = add4_rn(q1, ldc4(P.st + b * 256 + 4 * hh + 8 * (16 + j))); }
        dx = __fsub_rn(P.xyz2[nb * 3], P.xyz1[i * 3]); dy = __fsub_rn(P.xyz2[nb * 3 + 1], P.xyz1[i * 3 + 1]);
        dz = __fsub_rn(P.xyz2[nb * 3 + 2], P.xyz1[i * 3 + 2]);
    }
    for (int t = t0; t < ntiles; t += tstep) {
        asm volatile("" ::: "memory");
        // the next tile's neighbour index (wave-uniform condition)
        const bool more = t + tstep < ntiles;
        int bn, Gn;
        locate(more ? t + tstep : t, bn, Gn);
        const int ptn = Gn * PPW + 2 * wave + pp;
        const bool validn = ptn < P.n1;
        const long in_ = (long)bn * P.n1 + (validn ? ptn : P.n1 - 1);
        long knn_next = 0;
        if (more) knn_next = (long)P.knn[in_ * 16 + j];
        // layer 1: leaky(p1[i] + p2[nb] + Wd.d)     (bias folded into p1, or into the per-sample term: (p1[i] + st[b]) + p2[nb])
        f4 h[32];
        float t2[8];
        {
            const float b0 = hh ? dy : dx, b1 = hh ? 0.f : dz;      // B[k = hh][col] of the two k-steps (k = 3: the zero column)
            cv_rows_read<0>(rows, col, hh, h);
            cv_rows_request<1>(P.p2, (int)nb, rows, lane);
            cv_layer1_blocks<0, 4, LDSC>(P, s_c, q0, q1, b0, b1, hh, col, kinf, h);
            // the WeightNet's hidden layers (3 -> 8 -> 8: ~100 VALU instructions on the direction only) HERE, where the wave would
            // otherwise wait for round 1 of the rows -- they used to open the output epilogue, exposed (8 registers across the layers)
#if CV_LDS_HIDDEN
            if constexpr (LDSC && !SAVE) wn_hidden_lds(s_c, dx, dy, dz, t2);      // (the training forward with it: 25 registers spilled to scratch)
            else
#endif
                wn_hidden(P.wn, dx, dy, dz, t2);
            __builtin_amdgcn_sched_barrier(0);      // (round 1's reads wait for the DMA: hipcc would hoist them, and the wait, above the four blocks)
            cv_rows_read<1>(rows, col, hh, h);
            cv_layer1_blocks<4, 8, LDSC>(P, s_c, q0, q1, b0, b1, hh, col, kinf, h);
        }
        const long nbn = (long)bn * P.n2 + knn_next;      // (no next tile: row 0 of the sample, requested and never read)
        // byte offset of this lane's first 16-byte slot in a (position, 256) row (one 32-bit VGPR on uniform base pointers)
        const long pos = i * 16 + j;
        const unsigned ro = (unsigned)pos * 1024u + 16u * hh;
        if (SAVE && valid) {
            uint2 m[2];
            split_sign_masks(h, m);
            P.mk1[pos * 4 + hh] = m[0];
            P.mk1[pos * 4 + 2 + hh] = m[1];
        }
        f16v acc[SPLIT_VB];
        f4 bq[2][8];
        // a1 goes out while it is being consumed; the next tile's first round of rows is requested; the bias arrives during the last k-step
        LaneScale sc = lane_scale32(h);
        if (SAVE && P.amax) tensor_amax_update(P.amax, sc.mb);
        split_layer<0>(ws, h, sc.s, acc, SidePair<CvLayer2Side<SAVE>, BiasSide>{{StoreRowsSide{P.sv1, ro, valid}, CvRowsRequest(P.p2, rows, (int)nbn, 0, lane)},
                                                                              BiasSide{bias2, bq}});
        float c = sc.inv * wi2;
        split_epilogue(acc, bias2, bq, [&](int e, f4 a, f4 b) { h[e] = leaky_med4(scale_bias4(a, c, b), kinf); });
        if (SAVE && valid) {
            uint2 m[2];
            split_sign_masks(h, m);
            P.mk2[pos * 4 + hh] = m[0];
            P.mk2[pos * 4 + 2 + hh] = m[1];
        }
        sc = lane_scale32(h);
        if (SAVE && P.amax) tensor_amax_update(P.amax + 1, sc.mb);
        if (SAVE) split_layer<SPLIT_NF>(ws, h, sc.s, acc, SidePair<StoreRowsSide, BiasSide>{StoreRowsSide{P.sv2, ro, valid}, BiasSide{bias3, bq}});
        else split_layer<SPLIT_NF>(ws, h, sc.s, acc, BiasSide{bias3, bq});
        ws.sync();                                                   // wrap the stream to chunk 0
        c = sc.inv * wi3;
        split_epilogue(acc, bias3, bq, [&](int e, f4 a, f4 b) { h[e] = leaky_med4(scale_bias4(a, c, b), kinf); });      // a3
        if (SAVE && valid) {
#pragma unroll
            for (int e = 0; e < 32; ++e) *cv_at(P.sv3, ro + 32u * e) = h[e];
        }
        WnBlock wk = wnb(0);
        // out[i] = sum over the 16 neighbours of relu(Wc.t2 + bc) * a3, one 32-channel block at a time; block v + 1's four
        // dependent MFMAs (K = 8 in steps of 2) run under block v's VALU / DPP work, block v + 2's operands travel meanwhile
        float *o = P.out + i * P.out_pitch + 4 * hh;
        f16v wpre = wn_pre(wk, hh, t2);
        constexpr bool ahead1 = LDSC && CV_WN_AHEAD == 1;
        if constexpr (!ahead1) wk = wnb(1);
        auto out_block = [&](int v) {
            const f16v w = wpre;
            if constexpr (ahead1) {
                if (v + 1 < SPLIT_VB) wk = wnb(v + 1);
            }
            if (v + 1 < SPLIT_VB) wpre = wn_pre(wk, hh, t2);
            if constexpr (!ahead1) {
                if (v + 2 < SPLIT_VB) wk = wnb(v + 2);
            }
            f4 r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) r[q][e] = relu1(w[4 * q + e], kinf) * h[4 * v + q][e];
            // sum over the 16 neighbours by the transposing reduction (fused_common.h): lane j ends with slot q = 2 (bit 3 of j) + (bit 2
            // of j) of the block, the first lane of each quad stores -- 32 cross-lane operations and one store instead of 64 and four
            const f4 t = row_sum16_transpose4(r[0], r[1], r[2], r[3]);
            if (valid && (j & 3) == 0) *reinterpret_cast<f4 *>(o + 32 * v + 8 * (2 * ((j >> 3) & 1) + ((j >> 2) & 1))) = t;
        };
        out_block(0);
        out_block(1);
        // ---- next tile: its direction and its p1 slots -------------------------------------------------------------------------
        float cn[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};              // the six coordinates; subtracted after the last block (the
        f4 q0n = q0, q1n = q1, s0n = q0, s1n = q1;                    // subtraction is where the wave waits for them; so is the
        if (more) {                                                   // per-sample term's addition)
#pragma unroll
            for (int c = 0; c < 3; ++c) { cn[c] = ldc(P.xyz2 + nbn * 3 + c); cn[3 + c] = ldc(P.xyz1 + in_ * 3 + c); }
            q0n = ldc4(P.p1 + in_ * 256 + 4 * hh + 8 * j); q1n = ldc4(P.p1 + in_ * 256 + 4 * hh + 8 * (16 + j));
        }
        if (more && P.st) { s0n = ldc4(P.st + bn * 256 + 4 * hh + 8 * j); s1n = ldc4(P.st + bn * 256 + 4 * hh + 8 * (16 + j)); }
#pragma unroll
        for (int v = 2; v < SPLIT_VB; ++v) out_block(v);
        pt = ptn; valid = validn; i = in_; nb = nbn; q0 = q0n; q1 = q1n;
        if (P.st) { q0 = add4_rn(q0n, s0n); q1 = add4_rn(q1n, s1n); }
        dx = __fsub_rn(cn[0], cn[3]); dy = __fsub_rn(cn[1], cn[4]); dz = __fsub_rn(cn[2], cn[5]);
    }
    ws.finish();
}

// ---- the forward on the 16-position tile: two waves per SIMD ---------------------------------------------------------------------
// The same operator on the same arithmetic pieces (layer 1 and the WeightNet's output layer on the fp32-input MFMA, layers 2 and 3 as
// three fp16 products of two pieces under the position's power-of-two scale, fp32 accumulation), on the tile of fused_common.h: a
// wave owns ONE query point x its 16 neighbours, lane = 16 g + j holds channels 16 u + 4 g + r of position j, the layers run on
// v_mfma_f32_16x16x32_f16 over the image order of rtk_pack_split_layer16.  64 registers of activations and 64 accumulators instead of
// 128 + 128: a wave fits in half a SIMD's register file, the workgroup has eight waves (eight points per iteration, as the 32-position
// kernel) on one weight stream, and what one wave does outside the matrix pipe -- layer 1, the epilogues, the neighbour sum -- can run
// under the other wave's MFMAs.  The price: every streamed fragment is read from LDS by eight waves for 16 positions each instead of
// four waves for 32 (twice the fragment reads per MFMA).
constexpr int CV16_NW = 8;
constexpr int CV16_V = 16;                     // 16-channel blocks of 256 channels
constexpr int CV16_KS = 8;                     // k-steps (32 input channels) of a 256-channel contraction
constexpr int CV16_NF = CV16_KS * CV16_V * 2;  // fragments (KiB) of one 256 x 256 layer
constexpr int CV16_ROWS_F4 = 16 * 32;          // f4 per wave: 16 positions x 32 slots of 16 bytes (half a gathered row per round)
// Slot s of position p's 512 bytes holds source chunk s ^ p (CvRowsRequest); lane (g, j) reads chunk 4 u + g of position j.  The lanes a
// ds_read_b128 serves together ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) are 16 different positions at two values of g.
constexpr int cv16_rows_slot(int pos, int chunk) { return pos * 32 + (chunk ^ pos); }
constexpr bool cv16_rows_conflict_free() {
    constexpr int served[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    for (int u = 0; u < 8; ++u)
        for (int half = 0; half < 2; ++half)
            for (int grp = 0; grp < 2; ++grp) {
                unsigned seen = 0u;
                for (int k = 0; k < 16; ++k) {
                    const int lane = 32 * half + served[grp][k], g = lane >> 4, j = lane & 15;
                    const unsigned bankgroup = 1u << (cv16_rows_slot(j, 4 * u + g) & 15);
                    if (seen & bankgroup) return false;
                    seen |= bankgroup;
                }
            }
    return true;
}
static_assert(cv16_rows_conflict_free(), "a ds_read_b128 of the staged rows must touch 16 different bank groups per lane group");
static_assert(cv16_rows_slot(15, 31) < CV16_ROWS_F4, "a position's chunks stay inside its own 512 bytes");

// The constants in the tile's layout: a lane's read is one ds_read at an immediate offset from lane * 4 (the A operands) or 16 g (the biases).
struct CvConsts16 {
    float wd[CV16_V * 64];            // A[i][k = g] of block v of [Wd | 0]: the packed offset image as it is
    float wc[CV16_V * 2 * 64];        // ... of block v's two k-steps of Wc: k-slot g of step s is hidden channel 2 g + s (the eight live ones)
    float bc[256], bias2[256], bias3[256];
    float hid[128];                   // as CvConsts::hid
};
static_assert(sizeof(CvConsts16) == 15 * 1024 + 512, "4 + 8 + 3 KiB + the hidden layers");
__device__ __forceinline__ void cv16_consts_fill(CvConsts16 &C, const float *wd, const WnSplit &W, const float *bias2, const float *bias3, int t) {
    if (t < 256) *reinterpret_cast<f4 *>(C.wd + 4 * t) = ldc4(wd + 4 * t);
    else if (t < 256 + 192) {
        const int which = (t - 256) >> 6, l = t & 63;
        *reinterpret_cast<f4 *>((which == 0 ? C.bc : which == 1 ? C.bias2 : C.bias3) + 4 * l) = ldc4((which == 0 ? W.bc : which == 1 ? bias2 : bias3) + 4 * l);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int e = 512 * n + t, v = e >> 7, s = (e >> 6) & 1, l = e & 63, k = 2 * (l >> 4) + s;
        C.wc[e] = ldc(W.wc + ((v * 64 + 16 * (k >> 2) + (l & 15)) * 4 + (k & 3)));
    }
    if (t < 104) {
        const int u = t < 32 ? 0 : t - 32, o = u >> 3, c = u & 7;
        C.hid[t] = ldc(t < 32 ? W.wa + 16 * (t >> 3) + (t & 7) : t < 96 ? W.wb + (16 * (c >> 2) + o) * 4 + (c & 3) : W.bb + (t - 96));
    }
}

// wn_hidden_lds in pieces: the same operations on the same values, but no more than 40 of the image's 104 words in registers at a time
// (left to itself hipcc reads them all first -- next to the tile's 64 activations that is past the wave's half of the register file)
__device__ __forceinline__ void cv16_wn_hidden(const CvConsts16 &C, float dx, float dy, float dz, float (&t2)[8]) {
    float t1[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = __fmaf_rn(C.hid[o], dx, 0.f);
        a = __fmaf_rn(C.hid[8 + o], dy, a);
        a = __fmaf_rn(C.hid[16 + o], dz, a);
        t1[o] = fmaxf(__fadd_rn(a, C.hid[24 + o]), 0.f);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = C.hid[96 + o];
#pragma unroll
        for (int c = 0; c < 8; ++c) a = __fmaf_rn(C.hid[32 + 8 * o + c], t1[c], a);
        t2[o] = fmaxf(a, 0.f);
        asm volatile("" : "+v"(t2[o]));      // computed HERE: sunk to its use in the output epilogue, the 64 weights would live across the layers
        if (o % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// one round of the wave's 16 gathered rows: eight requests of two half rows each (CvRowsRequest: lanes 0..31 position 2 T, 32..63 position 2 T + 1)
template <int HALF>
__device__ __forceinline__ void cv16_rows_request(const float *p2, int nbrow, f4 *rows, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the previous round's reads have returned before their slots are overwritten
    CvRowsRequest(p2, rows, nbrow, HALF, lane).all(std::make_integer_sequence<int, 8>{});
}
// this lane's eight slots of the round: channels 128 HALF + 16 u + 4 g .. + 3, u = 0..7
template <int HALF>
__device__ __forceinline__ void cv16_rows_read(const f4 *rows, int j, int g, f4 (&h)[CV16_V]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) h[8 * HALF + u] = rows[j * 32 + ((4 * u + g) ^ j)];
}
// layer 1 of blocks U0 .. U0 + 7: leaky((q of block u + the gathered row) + Wd.d)
template <int U0>
__device__ __forceinline__ void cv16_layer1_blocks(const CvConsts16 &C, const f4 q, float bop, int lane, float kinf, f4 (&h)[CV16_V]) {
    auto block = [&](auto uc) {
        constexpr int u = decltype(uc)::value;
        h[u] = leaky_med4(mfma4(C.wd[u * 64 + lane], bop, add_row_bcast<u>(q, h[u])), kinf);
    };
    block(std::integral_constant<int, U0>{}); block(std::integral_constant<int, U0 + 1>{});
    block(std::integral_constant<int, U0 + 2>{}); block(std::integral_constant<int, U0 + 3>{});
    block(std::integral_constant<int, U0 + 4>{}); block(std::integral_constant<int, U0 + 5>{});
    block(std::integral_constant<int, U0 + 6>{}); block(std::integral_constant<int, U0 + 7>{});
}

// One group step of a layer on the 16-position tile: the four fragments (h and l piece) of two 16-row output blocks against the two B
// pieces of the k-step, six MFMAs, the two blocks interleaved, small terms first (LayerStepS::mm, fused_common.h); the reads of the next
// group and the splitting of the next k-step's activations sit between them (SplitStep, split_mfma.h).
template <int FBASE, int GI, class WS, int F, bool ZERO>
struct Split16Step {
    static constexpr int GV = CV16_V / 2, NG = CV16_KS * GV;
    template <int GJ, int PART>
    static __device__ __forceinline__ void load_part(WS &ws, f4 (&dst)[SPLIT_GF]) {
        constexpr int f0 = FBASE + GJ * SPLIT_GF;
        if constexpr (PART == 0) {
            if constexpr (f0 % F == 0 && f0 != 0) ws.sync();
            if constexpr ((f0 % F) / SPLIT_GF < split_issue_groups(F)) ws.template issue_part<(f0 % F) / SPLIT_GF, split_issue_groups(F)>();
        }
        dst[2 * PART] = ws.template frag_async<(f0 + 2 * PART) % F>();
        dst[2 * PART + 1] = ws.template frag_async<(f0 + 2 * PART + 1) % F>();
    }
    static __device__ __forceinline__ void run(WS &ws, const f4 (&h)[CV16_V], float scale, f4 (&acc)[CV16_V], f4 (&a)[2][SPLIT_GF], u4v (&b)[2][2]) {
        constexpr int up = GI / GV, v0 = (GI % GV) * 2;
        static_assert(F % SPLIT_GF == 0, "a group step reads four consecutive fragments of one chunk");
        lds_wait<0>(a[GI & 1]);
        const f4(&c)[SPLIT_GF] = a[GI & 1];
        const u4v(&B)[2] = b[up & 1];
        f4 z0, z1;
        if constexpr (ZERO && up == 0) z0 = z1 = f4_zero();
        else { z0 = acc[v0]; z1 = acc[v0 + 1]; }
        acc[v0] = mfma16_h(__builtin_bit_cast(u4v, c[1]), B[0], z0);                    // l . h
        acc[v0 + 1] = mfma16_h(__builtin_bit_cast(u4v, c[3]), B[0], z1);
        if constexpr (GI + 1 < NG) load_part<GI + 1, 0>(ws, a[(GI + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        acc[v0] = mfma16_h(__builtin_bit_cast(u4v, c[0]), B[1], acc[v0]);               // h . l
        acc[v0 + 1] = mfma16_h(__builtin_bit_cast(u4v, c[2]), B[1], acc[v0 + 1]);
        if constexpr (GI + 1 < NG) load_part<GI + 1, 1>(ws, a[(GI + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (up + 1 < CV16_KS && GI % GV < 4) split2_word_of<GI % GV>(h[2 * (up + 1)], h[2 * (up + 1) + 1], scale, b[(up + 1) & 1]);
        acc[v0] = mfma16_h(__builtin_bit_cast(u4v, c[0]), B[0], acc[v0]);               // h . h
        acc[v0 + 1] = mfma16_h(__builtin_bit_cast(u4v, c[2]), B[0], acc[v0 + 1]);
        __builtin_amdgcn_sched_barrier(0);
    }
};
template <int FBASE, class WS, int F, bool ZERO, int... GI>
__device__ __forceinline__ void split16_layer_impl(WS &ws, const f4 (&h)[CV16_V], float scale, f4 (&acc)[CV16_V], std::integer_sequence<int, GI...>) {
    f4 a[2][SPLIT_GF];
    u4v b[2][2];
    Split16Step<FBASE, 0, WS, F, ZERO>::template load_part<0, 0>(ws, a[0]);
    Split16Step<FBASE, 0, WS, F, ZERO>::template load_part<0, 1>(ws, a[0]);
    split2(h[0], h[1], scale, b[0]);
    __builtin_amdgcn_sched_barrier(0);
    (Split16Step<FBASE, GI, WS, F, ZERO>::run(ws, h, scale, acc, a, b), ...);
}
// acc = 2^(kw + kx) W . h for a 256 x 256 layer whose 16-position image starts at fragment FBASE of the stream; scale = this lane's 2^kx
// (lane_scale16).  All waves of the workgroup call this together (the stream has barriers).
template <int FBASE, int NW, int F, int NF>
__device__ __forceinline__ void split16_layer(WStreamA<NW, F, NF> &ws, const f4 (&h)[CV16_V], float scale, f4 (&acc)[CV16_V]) {
    split16_layer_impl<FBASE, WStreamA<NW, F, NF>, F, true>(ws, h, scale, acc, std::make_integer_sequence<int, CV16_KS * (CV16_V / 2)>{});
}

__global__ __launch_bounds__(64 * CV16_NW) __attribute__((amdgpu_waves_per_eu(2, 2)))
void cost_volume_split_kernel16(const CvSplitParams P) {
    const float kinf = rtk_hidden_inf();
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * CV_F * 64];
    __shared__ __attribute__((aligned(16))) f4 s_rows[CV16_NW * CV16_ROWS_F4];
    __shared__ __attribute__((aligned(16))) CvConsts16 s_c;      // 64 + 64 + 15.5 KiB
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, j = lane & 15;
    f4 *rows = s_rows + wave * CV16_ROWS_F4;
    constexpr int PPW = CV16_NW;                                    // points per workgroup iteration
    const int groups = (P.n1 + PPW - 1) / PPW;
    // tiles = (sample, group of eight points), dealt as in cost_volume_split_kernel: flat (P.gx > 0) or one sample per grid row
    const bool flat = P.gx > 0;
    const int xcd = blockIdx.x & 7, t0 = flat ? (int)(blockIdx.x >> 3) : (int)blockIdx.x, tstep = flat ? P.gx >> 3 : (int)gridDim.x;
    const int ntiles = flat ? (P.samples >> 3) * groups : groups;
    auto locate = [&](int t, int &b_, int &G_) {
        if (flat) { const int sk = t / groups; b_ = sk * 8 + xcd; G_ = t - sk * groups; }
        else { b_ = blockIdx.y; G_ = t; }
    };
    int b, bx;
    locate(t0 < ntiles ? t0 : 0, b, bx);
    cv16_consts_fill(s_c, P.wd, P.wn, P.bias2, P.bias3, (int)threadIdx.x);
    WStreamA<CV16_NW, CV_F, 2 * CV16_NF> ws;
    ws.start_parts(P.blob, s_w, wave, lane);                        // (its barrier publishes the constants too)
    const float wi2 = ldc(P.wsc), wi3 = ldc(P.wsc + 1);
    // Software-pipelined by one tile as the 32-position kernel: the next tile's neighbour index is requested at the top of the current
    // tile, the first half of its gathered rows after layer 1, its direction and its p1 slot in the output epilogue.
    bool valid = bx * PPW + wave < P.n1;
    long i = (long)b * P.n1 + (valid ? bx * PPW + wave : P.n1 - 1);
    long nb = 0;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    f4 q = {0.f, 0.f, 0.f, 0.f};                                    // p1 slot j of this wave's point: channels 16 j + 4 g .. + 3
    if (t0 < ntiles) {
        nb = (long)b * P.n2 + (long)P.knn[i * 16 + j];
        cv16_rows_request<0>(P.p2, (int)nb, rows, lane);
        q = ldc4(P.p1 + i * 256 + 16 * j + 4 * g);
        if (P.st) q = add4_rn(q, ldc4(P.st + b * 256 + 16 * j + 4 * g));
        dx = __fsub_rn(P.xyz2[nb * 3], P.xyz1[i * 3]); dy = __fsub_rn(P.xyz2[nb * 3 + 1], P.xyz1[i * 3 + 1]);
        dz = __fsub_rn(P.xyz2[nb * 3 + 2], P.xyz1[i * 3 + 2]);
    }
    for (int t = t0; t < ntiles; t += tstep) {
        asm volatile("" ::: "memory");
        // (the swizzled LDS addresses of the rows -- 16 reads, 16 request offsets -- are functions of the lane alone: computed from a
        // copy the optimiser cannot see through, one v_xor each per tile, they are not kept in 32 registers across the loop)
        int lv = lane;
        asm volatile("" : "+v"(lv));
        const int jv = lv & 15, gv = lv >> 4;
        const bool more = t + tstep < ntiles;                       // (wave-uniform)
        int bn, Gn;
        locate(more ? t + tstep : t, bn, Gn);
        const bool validn = Gn * PPW + wave < P.n1;
        const long in_ = (long)bn * P.n1 + (validn ? Gn * PPW + wave : P.n1 - 1);
        long knn_next = 0;
        if (more) knn_next = (long)P.knn[in_ * 16 + j];
        // layer 1: leaky(p1[i] + p2[nb] + Wd.d)     (bias folded into p1, or into the per-sample term)
        f4 h[CV16_V];
        float t2[8];
        {
            const float bop = g == 0 ? dx : g == 1 ? dy : g == 2 ? dz : 0.f;      // B[k = g][j]; k = 3 is the image's zero column
            cv16_rows_read<0>(rows, jv, gv, h);
            cv16_rows_request<1>(P.p2, (int)nb, rows, lv);
            cv16_layer1_blocks<0>(s_c, q, bop, lane, kinf, h);
            cv16_wn_hidden(s_c, dx, dy, dz, t2);      // the WeightNet's hidden layers while round 1 of the rows arrives
            __builtin_amdgcn_sched_barrier(0);
            cv16_rows_read<1>(rows, jv, gv, h);
            cv16_layer1_blocks<8>(s_c, q, bop, lane, kinf, h);
        }
        const long nbn = (long)bn * P.n2 + knn_next;
        if (more) cv16_rows_request<0>(P.p2, (int)nbn, rows, lv);      // lands under layers 2 and 3
        f4 acc[CV16_V];
        LaneScale sc = lane_scale16(h);
        split16_layer<0>(ws, h, sc.s, acc);
        float c = sc.inv * wi2;
#pragma unroll
        for (int v = 0; v < CV16_V; ++v) h[v] = leaky_med4(scale_bias4(acc[v], c, *reinterpret_cast<const f4 *>(s_c.bias2 + 16 * v + 4 * g)), kinf);
        sc = lane_scale16(h);
        split16_layer<CV16_NF>(ws, h, sc.s, acc);
        ws.sync();                                                   // wrap the stream to chunk 0
        c = sc.inv * wi3;
#pragma unroll
        for (int v = 0; v < CV16_V; ++v) h[v] = leaky_med4(scale_bias4(acc[v], c, *reinterpret_cast<const f4 *>(s_c.bias3 + 16 * v + 4 * g)), kinf);
        // ---- next tile: its direction and its p1 slot, under the output epilogue ------------------------------------------------
        float cn[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f4 qn = q, sn = q;
        if (more) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { cn[k] = ldc(P.xyz2 + nbn * 3 + k); cn[3 + k] = ldc(P.xyz1 + in_ * 3 + k); }
            qn = ldc4(P.p1 + in_ * 256 + 16 * j + 4 * g);
        }
        if (more && P.st) sn = ldc4(P.st + bn * 256 + 16 * j + 4 * g);
        // out[i] = sum over the 16 neighbours of relu(Wc.t2 + bc) * a3: K = 8 as two k-steps of the fp32-input MFMA (k-slot g of step s
        // = hidden channel 2 g + s), four 16-channel blocks per transposing reduction (lane j ends with block 4 m + 2 (bit 3) + (bit 2))
        const float tb0 = g == 0 ? t2[0] : g == 1 ? t2[2] : g == 2 ? t2[4] : t2[6], tb1 = g == 0 ? t2[1] : g == 1 ? t2[3] : g == 2 ? t2[5] : t2[7];
        float *o = P.out + i * P.out_pitch + 4 * g + 16 * (2 * ((j >> 3) & 1) + ((j >> 2) & 1));
#pragma unroll
        for (int m = 0; m < CV16_V / 4; ++m) {
            f4 r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = 4 * m + e;
                f4 w = *reinterpret_cast<const f4 *>(s_c.bc + 16 * v + 4 * g);
                w = mfma4(s_c.wc[(2 * v) * 64 + lane], tb0, w);
                w = mfma4(s_c.wc[(2 * v + 1) * 64 + lane], tb1, w);
                r[e] = relu_med4(w, kinf) * h[v];
            }
            const f4 s = row_sum16_transpose4(r[0], r[1], r[2], r[3]);
            if (valid && (j & 3) == 0) *reinterpret_cast<f4 *>(o + 64 * m) = s;
        }
        valid = validn; i = in_; nb = nbn; q = qn;
        if (P.st) q = add4_rn(qn, sn);
        dx = __fsub_rn(cn[0], cn[3]); dy = __fsub_rn(cn[1], cn[4]); dz = __fsub_rn(cn[2], cn[5]);
    }
    ws.finish();
}

// ---- rtk_cost_volume_bwd on the split path ------------------------------------------------------------------------------
// Same outputs as cost_volume_bwd_kernel (fused_group.hip) from the same saved tensors; the tile of the split forward.  The two
// transposed 256 x 256 products (W3^T dz3, W2^T dz2) run split; the WeightNet's hidden gradient dt2 = Wc^T dq3 (8 x 256 per
// position) runs on the fp32-input MFMA against an LDS image of Wc^T built once per workgroup.
struct CvSplitBwdParams {
    CvSplitParams f;              // geometry, WeightNet, blob = split images of W3^T, W2^T
    const float *dout;
    int dout_pitch;
    const float *a3;
    const uint2 *mk1, *mk2;
    float *dz1, *dz2, *dz3, *dq3, *d4, *dp1, *dpd, *dt2, *dbrows;
};

__device__ __forceinline__ f4 leaky_grad_bits4(f4 d, unsigned bits) {     // d * leaky'(z), [z > 0] in the low four bits
    return (f4){(bits & 1u) ? d.x : 0.1f * d.x, (bits & 2u) ? d.y : 0.1f * d.y, (bits & 4u) ? d.z : 0.1f * d.z, (bits & 8u) ? d.w : 0.1f * d.w};
}

__global__ __launch_bounds__(64 * SP_NW) __attribute__((amdgpu_waves_per_eu(1, 1))) void cost_volume_bwd_split_kernel(const CvSplitBwdParams Q) {
    const float kinf = rtk_hidden_inf();
    __shared__ __attribute__((aligned(16))) f4 s_w[2 * SP_F * 64];
    __shared__ float s_wct[128 * 64];                                    // [(v, q, r)][lane = 32 hh + o]: Wc[32 v + 8 q + 4 hh + r][o] (o < 8, else 0)
    const CvSplitParams &P = Q.f;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5, col = lane & 31, pp = col >> 4,
              j = col & 15;
    const int jq = 2 * ((j >> 3) & 1) + ((j >> 2) & 1);               // the slot a lane holds after a transposing reduction of four
    for (int e = threadIdx.x; e < 128 * 64; e += 64 * SP_NW) {
        const int l = e & 63, st = e >> 6, o = l & 31, ch = 32 * (st >> 4) + 8 * ((st >> 2) & 3) + 4 * (l >> 5) + (st & 3);
        s_wct[e] = o < 8 ? P.wn.wc[((ch >> 4) * 64 + (o >> 2) * 16 + (ch & 15)) * 4 + (o & 3)] : 0.f;
    }
    int b, bx, nbx;
    rtk_decode_block(P.gx, b, bx, nbx);
    constexpr int PPW = 2 * SP_NW;
    const int groups = (P.n1 + PPW - 1) / PPW;
    WStreamA<SP_NW, SP_F, 2 * SPLIT_NF> ws;
    ws.start_parts(P.blob, s_w, wave, lane);                             // (its barrier also publishes s_wct)
    const float wi3 = ldc(P.wsc), wi2 = ldc(P.wsc + 1);                  // images: W3^T, W2^T
    // software-pipelined by one tile like the forward kernel: the next tile's neighbour index and direction are requested in this
    // tile's epilogue (the dz1 / neighbour-sum phase), not in front of its own first loads
    int pt = bx * PPW + 2 * wave + pp;
    bool valid = pt < P.n1;
    long i = (long)b * P.n1 + (valid ? pt : P.n1 - 1);
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (bx < groups) {
        const long nb = (long)b * P.n2 + (long)P.knn[i * 16 + j];
        dx = __fsub_rn(P.xyz2[nb * 3], P.xyz1[i * 3]); dy = __fsub_rn(P.xyz2[nb * 3 + 1], P.xyz1[i * 3 + 1]);
        dz = __fsub_rn(P.xyz2[nb * 3 + 2], P.xyz1[i * 3 + 2]);
    }
    for (int G = bx; G < groups; G += nbx) {
        asm volatile("" ::: "memory");
        const long pos = i * 16 + j;
        const unsigned ro = (unsigned)pos * 1024u + 16u * hh;
        if (valid && hh == 0) *reinterpret_cast<f4 *>(Q.d4 + pos * 4) = (f4){dx, dy, dz, 1.0f};
        uint2 m2[2] = {Q.mk2[pos * 4 + hh], Q.mk2[pos * 4 + 2 + hh]}, m1[2] = {Q.mk1[pos * 4 + hh], Q.mk1[pos * 4 + 2 + hh]};
        // a3 = leaky(z3).  (Through LDS as the forward's p2 rows -- whole lines, once -- the phase gains 3.6 k clocks per tile and the
        // two layers lose 6 k: next to this kernel's 32 KiB Wc^T image the rows only fit with 24 KiB halves of the weight buffer,
        // whose twice as many chunk boundaries each wait for the dz stores in flight; and the next tile's rows come from HBM, not L2:
        // requested as a layer's side job they are too young at three boundaries in a row: +9 k.  Not kept.)
        f4 h[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) h[e] = *cv_at(Q.a3, ro + 32u * e);
        // ---- out = sum_k wn * a3:  dz3 = dout wn leaky'(z3),  dq3 = dout a3 [wn > 0],  dt2 = Wc^T dq3 -------------------------
        float t2[8];
        WnBlock wk = wn_block(P.wn, 0, hh, col);
        // the dout row of a point is the same for its 16 neighbours: each of them loads two of its 32 slots, the products take the
        // owner's copy through DPP (mul_row_bcast)
        const float *dor = Q.dout + i * Q.dout_pitch + 4 * hh;
        const f4 dq0 = ldc4(dor + 8 * j), dq1 = ldc4(dor + 8 * (16 + j));
        wn_hidden(P.wn, dx, dy, dz, t2);
        f16v dt2;
#pragma unroll
        for (int e = 0; e < 16; ++e) dt2[e] = 0.f;
        f16v wpre = wn_pre(wk, hh, t2);
        wk = wn_block(P.wn, 1, hh, col);
        auto block_a = [&](auto vc) {
            constexpr int v = decltype(vc)::value;
            const f16v w = wpre;                                     // block v + 1's four MFMAs and block v + 2's operands travel under block v
            if constexpr (v + 1 < SPLIT_VB) wpre = wn_pre(wk, hh, t2);
            if constexpr (v + 2 < SPLIT_VB) wk = wn_block(P.wn, v + 2, hh, col);
            f4 zs[4];
            auto slot = [&](auto qc) {
                constexpr int q = decltype(qc)::value, e = 4 * v + q;
                const f4 a = h[e];
                f4 wv;
#pragma unroll
                for (int r = 0; r < 4; ++r) wv[r] = relu1(w[4 * q + r], kinf);
                const f4 da = mul_row_bcast<e & 15>(e < 16 ? dq0 : dq1, a);       // d * a
                const f4 t = mul_row_bcast<e & 15>(e < 16 ? dq0 : dq1, wv);       // d * relu(w)   (== d * w wherever w > 0, +-0 elsewhere)
                f4 qq, z;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    qq[r] = wv[r] > 0.f ? da[r] : 0.f;
                    z[r] = a[r] > 0.f ? t[r] : 0.1f * t[r];
                    dt2 = mfma_f32x2(s_wct[(16 * v + 4 * q + r) * 64 + lane], qq[r], dt2);
                }
                h[e] = z;
                zs[q] = z;
                if (valid) *cv_at(Q.dq3, ro + 32u * e) = qq;       // (dz3 goes out during the product that consumes it)
            };
            slot(std::integral_constant<int, 0>{}); slot(std::integral_constant<int, 1>{});
            slot(std::integral_constant<int, 2>{}); slot(std::integral_constant<int, 3>{});
            if (Q.dbrows) {                          // (uniform) per-query neighbour sums of the block's four slots by ONE transposing reduction
                const f4 r = row_sum16_transpose4(zs[0], zs[1], zs[2], zs[3]);      // (fused_common.h: lane j ends with slot jq; the host's bias sum shrinks 16x)
                if (valid && (j & 3) == 0) *reinterpret_cast<f4 *>(Q.dbrows + i * 512 + 32 * v + 8 * jq + 4 * hh) = r;
            }
        };
        block_a(std::integral_constant<int, 0>{}); block_a(std::integral_constant<int, 1>{}); block_a(std::integral_constant<int, 2>{});
        block_a(std::integral_constant<int, 3>{}); block_a(std::integral_constant<int, 4>{}); block_a(std::integral_constant<int, 5>{});
        block_a(std::integral_constant<int, 6>{}); block_a(std::integral_constant<int, 7>{});
        if (valid) *reinterpret_cast<f4 *>(Q.dt2 + pos * 8 + 4 * hh) = (f4){dt2[0], dt2[1], dt2[2], dt2[3]};      // rows 4 hh .. + 3 of the 8 hidden units
        // ---- da2 = W3^T dz3;  dz2 = da2 leaky'(z2) ----------------------------------------------------------------------------
        f16v acc[SPLIT_VB];
        LaneScale sc = lane_scale32(h);          // gradients span many orders of magnitude: the position's own scale is what keeps 22 bits
        if (P.amax) tensor_amax_update(P.amax, sc.mb);
        split_layer<0>(ws, h, sc.s, acc, StoreRowsSide{Q.dz3, ro, valid});
        float c = sc.inv * wi3;
#pragma unroll
        for (int v = 0; v < SPLIT_VB; ++v) {
#pragma unroll
            for (int q = 0; q < 4; ++q) h[4 * v + q] = leaky_grad_bits4(acc_slot(acc, 4 * v + q) * c, split_mask_bits(m2, v, q));
            if (Q.dbrows) {
                const f4 r = row_sum16_transpose4(h[4 * v], h[4 * v + 1], h[4 * v + 2], h[4 * v + 3]);
                if (valid && (j & 3) == 0) *reinterpret_cast<f4 *>(Q.dbrows + i * 512 + 256 + 32 * v + 8 * jq + 4 * hh) = r;
            }
        }
        // ---- da1 = W2^T dz2;  dz1 = da1 leaky'(z1);  dp1 = sum over the 16 neighbours; per-query partials of dWd = dz1^T d -----
        sc = lane_scale32(h);
        if (P.amax) tensor_amax_update(P.amax + 1, sc.mb);
        split_layer<SPLIT_NF>(ws, h, sc.s, acc, StoreRowsSide{Q.dz2, ro, valid});
        ws.sync();                                                   // wrap the stream to chunk 0
        c = sc.inv * wi2;
        // ---- next tile: neighbour index now, direction half way through the epilogue ---------------------------------------
        const int Gn = G + nbx;
        const bool more = Gn < groups;
        const int ptn = Gn * PPW + 2 * wave + pp;
        const bool validn = ptn < P.n1;
        const long in_ = (long)b * P.n1 + (validn ? ptn : P.n1 - 1);
        long knn_next = 0;
        if (more) knn_next = (long)P.knn[in_ * 16 + j];
        float dxn = 0.f, dyn = 0.f, dzn = 0.f;
        float *dpr = Q.dp1 + i * 256 + 4 * hh;
        float *dpd = Q.dpd + i * 768 + 4 * hh;
#pragma unroll
        for (int v = 0; v < SPLIT_VB; ++v) {
            if (v == 2 && more) {
                const long nbn = (long)b * P.n2 + knn_next;
                dxn = __fsub_rn(P.xyz2[nbn * 3], P.xyz1[in_ * 3]); dyn = __fsub_rn(P.xyz2[nbn * 3 + 1], P.xyz1[in_ * 3 + 1]);
                dzn = __fsub_rn(P.xyz2[nbn * 3 + 2], P.xyz1[in_ * 3 + 2]);
            }
            // the block's four slots: dz1 out, then the neighbour sums of dz1 and of dz1 (x) d, each by ONE transposing reduction of the
            // four slots (32 cross-lane operations instead of 64; lane j ends with slot jq and the first lane of each quad stores)
            f4 r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                r[q] = leaky_grad_bits4(acc_slot(acc, 4 * v + q) * c, split_mask_bits(m1, v, q));
                if (valid) *cv_at(Q.dz1, ro + 32u * (4 * v + q)) = r[q];
            }
            const f4 s0 = row_sum16_transpose4(r[0], r[1], r[2], r[3]);
            const f4 sx = row_sum16_transpose4(r[0] * dx, r[1] * dx, r[2] * dx, r[3] * dx);
            const f4 sy = row_sum16_transpose4(r[0] * dy, r[1] * dy, r[2] * dy, r[3] * dy);
            const f4 sz = row_sum16_transpose4(r[0] * dz, r[1] * dz, r[2] * dz, r[3] * dz);
            if (valid && (j & 3) == 0) {
                *reinterpret_cast<f4 *>(dpr + 32 * v + 8 * jq) = s0;
                *reinterpret_cast<f4 *>(dpd + 32 * v + 8 * jq) = sx;
                *reinterpret_cast<f4 *>(dpd + 256 + 32 * v + 8 * jq) = sy;
                *reinterpret_cast<f4 *>(dpd + 512 + 32 * v + 8 * jq) = sz;
            }
        }
        pt = ptn; valid = validn; i = in_; dx = dxn; dy = dyn; dz = dzn;
    }
    ws.finish();
}

// ---- rtk_sa_scale on the split path: the two-layer scales with 64 output channels (sa2 scale 1, sa3 scales 0 and 1) -------------
// A wave owns 32 (centroid, neighbour) positions: one centroid of 32 neighbours or two of 16.  The offset layer (K = 4 with the
// bias column) runs on the fp32-input MFMA, the C1 -> 64 layer split with its image RESIDENT in LDS (6 C1 x 64 bytes: no stream,
// no barriers after the fill), the max over the neighbours in registers.
struct SaSplitParams {
    int samples, n, npoint, gx;
    const float *xyz, *new_xyz;
    const int *idx;
    const float *q;
    int q_pitch;
    const float *w1;        // offset layer image [C1 / 16][64] of [Wx | b1]
    const f4 *image;        // split image of the C1 -> 64 layer ...
    const float *wsc;       // ... and the inverse of its power-of-two weight scale
    const float *bias2;
    float *out;
    int out_pitch, out_offset;
    const int *src_nuniq, *dst_nuniq;
};

// Register budget: four waves per SIMD (<= 128 registers), which is what the launcher's grid gives anyway (SA_WGS_TARGET workgroups of
// four waves on 1024 SIMDs).  The pipelined loop held the next unit's q rows (32 registers at C1 = 64) and coordinates next to the
// tile in work: 122 / 127 / 116 registers, no scratch; with the rows staged in LDS (SaRows) one 32-channel block of them is in registers
// under the epilogue only: 106 / 108 / 98.  (Five waves, <= 96 registers, held the serial loop -- 94 / 94 / 76 -- and was
// chosen when an SA wave fitted on a SIMD next to a 404-register forward cost volume; that kernel now allocates CV_FWD_VGPRS and shares
// its SIMDs with nothing.  Under that cap the pipelined loop spills 45 / 71 / 10 registers.  The first capped build computed wrong
// maxima: see the epilogue.)
#ifndef SA_SPLIT_WAVES
#define SA_SPLIT_WAVES 4
#endif
#ifndef SA_WGS_TARGET
#define SA_WGS_TARGET 1024
#endif
// The k-step of layer 2 behind which the pipelined loop requests the next unit's rows at C1 = 64 (four k-steps; at C1 = 32 they go
// out in front of layer 2).  Behind step 1 a quarter of the tile's activations is dead and the rows fit: in front of layer 2 the
// 64-channel shapes spilled 2 / 11 registers when the rows went into registers.  (Through LDS step 0 fits as well and measures the
// same.)  <16, 64> also needs its epilogue fenced off from layer 2 (else the scheduler hoists the eight bias reads and the first
// block's maximum over the last MFMAs: 6 - 11 registers spilled); SA_EPI_FENCE_ALL fences every shape.
#ifndef SA_GATHER_STEP
#define SA_GATHER_STEP 1
#endif
// C1 = 64, rows through LDS: the k-step behind which round 0 of the next unit's rows is read and round 1 requested (3: the last MFMA;
// 2, with SA_GATHER_STEP 0 or 1, measures the same: tools/experiments/sa_ablate.py, profiles/sa_rows_lds_schedules.txt).
#ifndef SA_ROWS_READ_STEP
#define SA_ROWS_READ_STEP 3
#endif
#ifndef SA_EPI_FENCE_ALL
#define SA_EPI_FENCE_ALL 0
#endif
// How many units ahead of its use the pipelined loops request a unit's centroid and ball index (the gathers stay one unit ahead).
// 1: at the top of the unit before, needed behind that unit's layer 1 -- one dependent round trip per tile.  2: a whole tile earlier,
// five more registers of state and a third copy of the loop body.  An instance may take 2 only where its code object keeps 0 scratch, 0
// spills and <= 128 registers with it (sa_split_index_ahead, the place for an exception: today all three fit, 128 / 128 / 120; the
// same macro and rule in fused_group.hip).  Measured slower than 1 at every configuration: the default is 1.
#ifndef SA_INDEX_AHEAD
#define SA_INDEX_AHEAD 1
#endif
constexpr int sa_split_index_ahead(int ns, int c1) { return SA_INDEX_AHEAD == 2 ? 2 : 1; }

// ---- the q rows of the pipelined loop through LDS -----------------------------------------------------------------------------------
// The tile layout gives a lane 32 bytes of its own position's q row per load instruction: 32 partial cache lines per instruction, the
// four instructions of a 32-channel block sweeping the same 32 lines while they are in flight (the pattern layer 1 of the cost volume
// and the patch kernel had: CvRowsRequest above, pt_rows_request in fused_patch.hip).  Here a 32-channel block of the 32 rows of a unit
// -- 128 contiguous bytes per position -- is one ROUND: four global_load_lds of 16 bytes per lane into the wave's own 4 KiB slab,
// instruction T serving positions 8 T .. 8 T + 7, lane L chunk L & 7 of position 8 T + (L >> 3): eight lines per instruction, each
// fetched once.  C1 / 32 rounds per unit share the slab, one after the other.  Slot s of a position's 128 bytes holds source chunk
// s ^ sa_rows_swz(position), so that the 16 lanes a ds_read_b128 serves together hit 16 different 16-byte bank groups.
constexpr int SA_ROWS_F4 = 32 * 8;                                 // f4 per wave: 32 positions x 8 slots of 16 bytes
constexpr int sa_rows_swz(int pos) { return (pos >> 1) & 7; }
constexpr int sa_rows_slot(int pos, int chunk) { return pos * 8 + (chunk ^ sa_rows_swz(pos)); }      // f4 index in the slab
// Every chunk, both halves of the columns, for the two ways the 32 columns of one hh may be cut into groups of 16: consecutive columns,
// and the lane groups ds_read_b128 is served in on gfx950 ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}).  64 banks of four bytes are
// 16 groups of 16 bytes.
constexpr bool sa_rows_conflict_free() {
    constexpr int served[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    for (int chunk = 0; chunk < 8; ++chunk)
        for (int g = 0; g < 2; ++g) {
            unsigned seen_a = 0u, seen_b = 0u;
            for (int k = 0; k < 16; ++k) {
                const unsigned a = 1u << (sa_rows_slot(16 * g + k, chunk) & 15), bgrp = 1u << (sa_rows_slot(served[g][k], chunk) & 15);
                if ((seen_a & a) || (seen_b & bgrp)) return false;
                seen_a |= a; seen_b |= bgrp;
            }
        }
    return true;
}
static_assert(sa_rows_conflict_free(), "a ds_read_b128 of the staged rows must touch 16 different bank groups per lane group");
static_assert(sa_rows_swz(31) < 8 && sa_rows_slot(31, 7) < SA_ROWS_F4, "a position's chunks stay inside its own 128 bytes of the slab");
// Which instances take their rows through LDS (the others keep the direct gather): the place for an exception.
constexpr bool sa_split_rows_lds(int ns, int c1) { return true; }
struct SaRows {
    const char *q;                 // row 0, first column, of this workgroup's sample (uniform; byte offsets from here are 32-bit)
    f4 *slab;                      // this wave's 4 KiB
    unsigned ro[4];                // instruction T: byte offset of position 8 T + (lane >> 3)'s row plus this lane's (swizzled) source chunk
    // rowoff: byte offset of the row of this lane's position (lane col and lane 32 + col hold the same)
    __device__ __forceinline__ void offsets(unsigned rowoff, int lane) {
#pragma unroll
        for (int T = 0; T < 4; ++T)
            ro[T] = (unsigned)__shfl((int)rowoff, 8 * T + (lane >> 3), 64) + ((unsigned)((lane & 7) ^ ((4 * T + (lane >> 4)) & 7)) << 4);
    }
    // round R of the unit whose offsets are held.  DRAIN: reads of the slab may still be in flight (the round before was read just now).
    template <int R, bool DRAIN>
    __device__ __forceinline__ void request() const {
        if constexpr (DRAIN) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // (uniform 64-bit base) + (32-bit per-lane offset), the round's 128 bytes in the offset: it stays below n * q_pitch * 4 < 2^32
#pragma unroll
        for (int T = 0; T < 4; ++T)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(q + (ro[T] + 128u * R)),
                                             (__attribute__((address_space(3))) void *)(slab + T * 64), 16, 0, 0);
    }
    // this lane's four slots of the round that was requested last: channels 32 R + 8 q + 4 hh .. + 3 at r[4 q ..]
    __device__ __forceinline__ void read(int col, int hh, f16v &r) const {
        // The round has landed.  vmcnt(0) waits for every load outstanding, so nothing younger than the round may be in flight that the
        // wave does not need here anyway: the coordinates that travel with round 0 are as old as it; the next unit's centroid and ball
        // index (requested at the top of a tile, two units ahead with SA_INDEX_AHEAD 2) are consumed at SA_GATHER_STEP, before any
        // read, or older than the round; the epilogue's stores come behind the last read.  A request moved between a round and its read
        // would be waited for here.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const f4 t = slab[sa_rows_slot(col, 2 * q4 + hh)];
            r[4 * q4] = t.x; r[4 * q4 + 1] = t.y; r[4 * q4 + 2] = t.z; r[4 * q4 + 3] = t.w;
        }
    }
};
// PIPE: the tile loop software-pipelined by one unit with its constants out of the loop (the first of the two loops below); false: the
// loop as it was before (rtk_sa_scale_split_serial, the comparison implementation).  The two compute the same bits.
template <int NS, int C1, bool PIPE>
__global__ __launch_bounds__(256, SA_SPLIT_WAVES) void sa_scale_split_kernel(const SaSplitParams P) {
    constexpr int KS = C1 / 16, VB1 = C1 / 32, NFR = KS * 2 * 2, CPT = 32 / NS;      // k-steps, 32-blocks of layer 1, fragments, centroids per tile
    // (as in sa_scale_kernel, fused_group.hip: the lanes of the last tile past live_c are redirected to centroid live_c - 1 before the
    // index load; the whole tile lies inside the zero tail ball_query_pair_body writes)
    static_assert(RTK_BALL_TAIL_ROWS % CPT == 0, "a tile of CPT centroids must not reach past the ball tables' zero tail");
    const float kinf = rtk_hidden_inf();
    __shared__ __attribute__((aligned(16))) f4 s_img[NFR * 64];
    const int lane = threadIdx.x & 63, hh = lane >> 5, col = lane & 31, pp = col / NS, slot = col % NS;
    int b, bx, nbx;
    rtk_decode_block(P.gx, b, bx, nbx);
    __shared__ __attribute__((aligned(16))) float s_bias2[PIPE ? 64 : 4];     // PIPE: bias2 and the offset image [KS][64] behind the image
    __shared__ float s_w1[PIPE ? KS * 64 : 1];
    constexpr bool ROWS = PIPE && sa_split_rows_lds(NS, C1);                  // the q rows through LDS (SaRows): a slab per wave
    __shared__ __attribute__((aligned(16))) f4 s_rows[ROWS ? 4 * SA_ROWS_F4 : 1];
    static_assert(VB1 <= 2, "the schedule below: the last round is read behind the epilogue, the one before it behind layer 2");
    if constexpr (PIPE) {
        // The serial loop below reloads the 2 VB1 offset weights of a lane and its eight bias2 fragments on every tile (the latter
        // only after the last layer-2 MFMA, waited for one by one) and makes three dependent round trips per tile: ball index ->
        // coordinates and q rows -> bias.  Here the offset image and bias2 live in LDS behind the split image (filled with it), and the
        // gathers of unit u + 1 are in flight under unit u's layer 2: its ball index and centroid are requested at the top of u, its
        // neighbour coordinates and q rows -- into registers of their own, which become layer 1's accumulators at the top of the next
        // trip -- under u's layer-2 MFMAs (SA_GATHER_STEP).  ROWS: the q rows are requested there as DMA into the wave's slab (SaRows),
        // one 32-channel block per round; the last round is read into those registers inside the epilogue, in front of its stores, the
        // one before it (C1 = 64) behind layer 2's last MFMAs, where the next round is requested.  Every round requested is read in the
        // same unit: a wave never exits with a DMA outstanding.  Whether a next unit exists is wave-uniform; without one nothing is
        // requested.  Lanes past live_c are redirected before every index load as in the serial loop.
        //
        // Prologue in two round trips (the serial one makes four: dst_nuniq -> fill and barrier -> src_nuniq, centroid, ball index ->
        // gathers).  Trip 1 is everything whose address depends on no loaded value: both counters, this thread's words of the image, the
        // offset image and bias2 (into registers; stored to LDS behind the exit test), the weight scale, and -- speculatively -- the
        // UN-redirected centroid and ball index of the wave's first unit, the centroid clamped below npoint so that the address stays
        // inside the tables whatever dst_nuniq holds.  A first unit wholly below live_c (wave-uniform) keeps them: they are what the
        // redirected loads return.  Any other first unit discards them and loads again behind the redirection, so the kernel may READ
        // ball and new_xyz rows of centroids in [live_c, npoint) but forms no address and no value from them.  Trip 2 is the gathers.
        // A null counter reads a word that is always there (idx[0]) and is not used: no branch around a load.
        constexpr int AH = sa_split_index_ahead(NS, C1);
        const int stride = nbx * 4;
        int unit = bx * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (an SGPR: the loop's branches are scalar)
        const int dst_w = *(P.dst_nuniq ? P.dst_nuniq + b : P.idx), src_w = *(P.src_nuniq ? P.src_nuniq + b : P.idx);
        static_assert(NFR * 64 == KS * 256 && KS * 64 <= 256, "the fill below: KS words of the image and one of w1 per thread");
        f4 img_w[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) img_w[k] = P.image[k * 256 + threadIdx.x];
        const float w1_w = P.w1[threadIdx.x & (KS * 64 - 1)], bias_w = P.bias2[threadIdx.x & 63];
        const float winv = ldc(P.wsc);
        const int c_s = b * P.npoint + min(unit * CPT + pp, P.npoint - 1);
        const int id_s = P.idx[(long)c_s * NS + slot];
        const float ca_s = P.new_xyz[(long)c_s * 3 + hh], cb_s = P.new_xyz[(long)c_s * 3 + 2];
        __builtin_amdgcn_sched_barrier(0);      // (everything above is in flight before the first wait)
        const int live_c = min(P.dst_nuniq ? __builtin_amdgcn_readfirstlane(dst_w) : P.npoint, P.npoint);
        const int live_units = (live_c + CPT - 1) / CPT;
        if (bx * 4 >= live_units) return;                     // (loads into registers may be outstanding, nothing else)
        const int src_e = P.src_nuniq ? src_w : 0x7fffffff;
#pragma unroll
        for (int k = 0; k < KS; ++k) s_img[k * 256 + threadIdx.x] = img_w[k];
        if (threadIdx.x < KS * 64) s_w1[threadIdx.x] = w1_w;
        if (threadIdx.x < 64) s_bias2[threadIdx.x] = bias_w;
        __syncthreads();
        if (unit >= live_units) return;                       // (no barrier follows)
        // A lane's two operands of the offset layer are (dx, dz) (hh = 0) or (dy, 1) (hh = 1): it loads component hh and component 2 of
        // the neighbour and of the centroid -- every lane both, the lanes hh = 1 select their constant afterwards.
        // State of the unit in work (c, valid, ca, cb and -- requested, not waited for -- na, nb, a), of the one after it (*_n) and,
        // where the index is requested two units ahead (AH == 2), of the one after that (*_2: centroid and ball index only).
        int c, c_n = 0, id_n = 0, c_2 = 0, id_2 = 0;
        bool valid, valid_n = false, valid_2 = false;
        float ca, cb, na, nb, ca_n = 0.f, cb_n = 0.f, na_n = 0.f, nb_n = 0.f, ca_2 = 0.f, cb_2 = 0.f;
        f16v a[VB1], an[VB1];
        auto centroid_of = [&](int u, int &cc, bool &vv) {        // global centroid index of this lane in unit u, redirected past live_c
            int cl = u * CPT + pp;
            vv = cl < live_c;
            if (!vv) cl = live_c - 1;
            cc = b * P.npoint + cl;
        };
        auto gather = [&](int id, float &xa, float &xb, f16v (&r)[VB1]) {     // neighbour coordinates and q rows (duplicate source rows alias row 0)
            const long src = (long)b * P.n + id;
            xa = P.xyz[src * 3 + hh]; xb = P.xyz[src * 3 + 2];
            const float *qrow = P.q + ((long)b * P.n + (id < src_e ? id : 0)) * P.q_pitch + 4 * hh;
#pragma unroll
            for (int v = 0; v < VB1; ++v)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f4 t = *reinterpret_cast<const f4 *>(qrow + 32 * v + 8 * q);
                    r[v][4 * q] = t.x; r[v][4 * q + 1] = t.y; r[v][4 * q + 2] = t.z; r[v][4 * q + 3] = t.w;
                }
        };
        // ROWS: the coordinates as plain loads, the rows as DMA requests (duplicate source rows alias row 0 before the offset is formed)
        SaRows rw;
        rw.q = reinterpret_cast<const char *>(P.q + (long)b * P.n * P.q_pitch);
        rw.slab = s_rows + (ROWS ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * SA_ROWS_F4 : 0);      // (an SGPR: the DMA's LDS base is scalar)
        auto gather_xyz = [&](int id, float &xa, float &xb) {
            const long src = (long)b * P.n + id;
            xa = P.xyz[src * 3 + hh]; xb = P.xyz[src * 3 + 2];
        };
        auto row_offset = [&](int id) { return (unsigned)(id < src_e ? id : 0) * ((unsigned)P.q_pitch * 4u); };
        auto request = [&](int u, int &cc, bool &vv, int &id, float &xa, float &xb) {      // centroid and ball index of unit u
            centroid_of(u, cc, vv);
            id = P.idx[(long)cc * NS + slot];
            xa = P.new_xyz[(long)cc * 3 + hh]; xb = P.new_xyz[(long)cc * 3 + 2];
        };
        // one unit; MORE: another one follows, whose gathers go out here; REQ: the centroid and ball index of the unit AH units ahead go
        // out at the top (AH == 1: MORE's own, used behind layer 1 -- the one dependent round trip per tile; AH == 2: the unit after
        // MORE's, a whole tile before its gathers need it).  (A copy of the body per combination -- the steady state, at AH == 2 the
        // unit with one left, and the last unit -- instead of a test inside one: behind a branch around a load the compiler has to
        // wait as if the load had not been issued.)
        auto tile = [&](auto req, auto more) {
            constexpr bool REQ = decltype(req)::value, MORE = decltype(more)::value;
            constexpr int GS = KS == 4 ? SA_GATHER_STEP : 0;
            if constexpr (REQ) {
                if constexpr (AH == 2) request(unit + 2 * stride, c_2, valid_2, id_2, ca_2, cb_2);
                else request(unit + stride, c_n, valid_n, id_n, ca_n, cb_n);
            }
            __builtin_amdgcn_sched_barrier(0);      // (the requests stay here: the scheduler otherwise moves them down to their first use)
            const float b0 = __fsub_rn(na, ca), dz = __fsub_rn(nb, cb);
            const float b1 = hh ? 1.0f : dz;
            f4 h[4 * VB1];
#pragma unroll
            for (int v = 0; v < VB1; ++v) {
                const int ch = 32 * v + col;
                const float *wr = s_w1 + (ch >> 4) * 64 + (ch & 15);
                a[v] = mfma_f32x2(wr[16 * hh], b0, a[v]);
                a[v] = mfma_f32x2(wr[16 * (2 + hh)], b1, a[v]);
#pragma unroll
                for (int q = 0; q < 4; ++q) h[4 * v + q] = relu_med4((f4){a[v][4 * q], a[v][4 * q + 1], a[v][4 * q + 2], a[v][4 * q + 3]}, kinf);
            }
            const LaneScale sc = lane_scale32(h);
            const float cs = sc.inv * winv;
            f16v acc[2];
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[v][e] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                u4v bp[2];
                split2(h[2 * s], h[2 * s + 1], sc.s, bp);
                u4v fr[2][2];
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int p = 0; p < 2; ++p) fr[v][p] = __builtin_bit_cast(u4v, s_img[((s * 2 + v) * 2 + p) * 64 + lane]);
#define RTK_SA_MM(pa, pb) acc[0] = mfma_h(fr[0][pa], bp[pb], acc[0]); acc[1] = mfma_h(fr[1][pa], bp[pb], acc[1]);
                RTK_SA_MM(1, 0) RTK_SA_MM(0, 1) RTK_SA_MM(0, 0)
#undef RTK_SA_MM
                if (MORE && s == GS) {
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (ROWS) {
                        gather_xyz(id_n, na_n, nb_n);
                        rw.offsets(row_offset(id_n), lane);
                        rw.template request<0, false>();      // (the slab's last reads were layer 1's operands: returned long ago)
                    } else gather(id_n, na_n, nb_n, an);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (ROWS && MORE && VB1 == 2 && s == SA_ROWS_READ_STEP) {      // round 0 into registers h has left, round 1 out
                    __builtin_amdgcn_sched_barrier(0);
                    rw.read(col, hh, an[0]);
                    rw.template request<1, true>();
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // epilogue: as in the serial loop, the bias from LDS
            if constexpr (SA_EPI_FENCE_ALL || (NS == 16 && C1 == 64)) __builtin_amdgcn_sched_barrier(0);
            f4 m[2][4];
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    m[v][q] = scale_bias4((f4){acc[v][4 * q], acc[v][4 * q + 1], acc[v][4 * q + 2], acc[v][4 * q + 3]}, cs,
                                          *reinterpret_cast<const f4 *>(s_bias2 + 32 * v + 8 * q + 4 * hh));
            const int qo = 2 * ((col >> 3) & 1) + ((col >> 2) & 1);
            float *o = P.out + (long)c * P.out_pitch + P.out_offset + 4 * hh + 8 * qo;
            // the next unit's last round, covered by the reductions; in front of the stores, whose return its wait would otherwise include
            auto rows_last = [&]() {
                if constexpr (ROWS && MORE) {
                    __builtin_amdgcn_sched_barrier(0);
                    rw.read(col, hh, an[VB1 - 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if constexpr (NS == 32) {
                f4 t[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] = wave_max_pair16(m[0][q], m[1][q], kinf);
                const f4 r = relu_med4(row_max16_transpose4(t[0], t[1], t[2], t[3]), kinf);
                rows_last();
                if (valid && (col & 3) == 0) *reinterpret_cast<f4 *>(o + 32 * ((col >> 4) & 1)) = r;
            } else {
                f4 r[2];
#pragma unroll
                for (int v = 0; v < 2; ++v) r[v] = relu_med4(row_max16_transpose4(m[v][0], m[v][1], m[v][2], m[v][3]), kinf);
                rows_last();
#pragma unroll
                for (int v = 0; v < 2; ++v)
                    if (valid && (col & 3) == 0) *reinterpret_cast<f4 *>(o + 32 * v) = r[v];
            }
        };
        int id = id_s;
        c = c_s; valid = true; ca = ca_s; cb = cb_s;
        if ((unit + 1) * CPT > live_c) request(unit, c, valid, id, ca, cb);      // (wave-uniform) a partial first unit: the dependent path
        if constexpr (ROWS) {
            // the first unit's rows: round 0 through the slab; at C1 = 64 the second block travels beside it as plain loads (the slab holds
            // one round, and a second round behind the first would be a third round trip)
            gather_xyz(id, na, nb);
            rw.offsets(row_offset(id), lane);
            rw.template request<0, false>();
            if constexpr (VB1 == 2) {
                const float *qrow = reinterpret_cast<const float *>(rw.q + row_offset(id)) + 32 + 4 * hh;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f4 t = *reinterpret_cast<const f4 *>(qrow + 8 * q);
                    a[1][4 * q] = t.x; a[1][4 * q + 1] = t.y; a[1][4 * q + 2] = t.z; a[1][4 * q + 3] = t.w;
                }
            }
            rw.read(col, hh, a[0]);
        } else gather(id, na, nb, a);
        auto advance = [&]() {
            unit += stride; c = c_n; valid = valid_n; ca = ca_n; cb = cb_n; na = na_n; nb = nb_n;
            for (int v = 0; v < VB1; ++v) a[v] = an[v];       // (a rotation of registers; the trip count is a constant)
        };
        if constexpr (AH == 2) {
            // the second unit's centroid and index travel with the first unit's gathers (no second unit: the first one's again, unused)
            request(unit + stride < live_units ? unit + stride : unit, c_n, valid_n, id_n, ca_n, cb_n);
            while (unit + 2 * stride < live_units) {
                tile(std::true_type{}, std::true_type{});
                advance();
                c_n = c_2; valid_n = valid_2; id_n = id_2; ca_n = ca_2; cb_n = cb_2;
            }
            if (unit + stride < live_units) {
                tile(std::false_type{}, std::true_type{});
                advance();
            }
        } else {
            while (unit + stride < live_units) {
                tile(std::true_type{}, std::true_type{});
                advance();
            }
        }
        tile(std::false_type{}, std::false_type{});
        return;
    }
    // ---- the serial comparison kernel (rtk_sa_scale_split_serial): prologue and loop as they were before the pipelined one ----
    const int dst_e = P.dst_nuniq ? __builtin_amdgcn_readfirstlane(P.dst_nuniq[b]) : P.npoint;
    const int live_c = min(dst_e, P.npoint);                      // centroids >= live_c are duplicates of centroid 0: neither computed nor written
    const int live_units = (live_c + CPT - 1) / CPT;
    if (bx * 4 >= live_units) return;
    for (int i = threadIdx.x; i < NFR * 64; i += blockDim.x) s_img[i] = P.image[i];
    __syncthreads();
    const int src_e = P.src_nuniq ? P.src_nuniq[b] : 0x7fffffff;
    const float winv = ldc(P.wsc);
    for (int unit = bx * 4 + (threadIdx.x >> 6); unit < live_units; unit += nbx * 4) {
        int cl = unit * CPT + pp;                                  // centroid of this lane within the sample
        const bool valid = cl < live_c;
        if (!valid) cl = live_c - 1;
        const int c = b * P.npoint + cl;
        const int id = P.idx[(long)c * NS + slot];
        const long src = (long)b * P.n + id;
        const float dx = __fsub_rn(P.xyz[src * 3], P.new_xyz[(long)c * 3]), dy = __fsub_rn(P.xyz[src * 3 + 1], P.new_xyz[(long)c * 3 + 1]),
                    dz = __fsub_rn(P.xyz[src * 3 + 2], P.new_xyz[(long)c * 3 + 2]);
        // layer 1: relu(q[id] + Wx.d + b1)      (duplicate source rows alias row 0)
        const float *qrow = P.q + ((long)b * P.n + (id < src_e ? id : 0)) * P.q_pitch + 4 * hh;
        const float b0 = hh ? dy : dx, b1 = hh ? 1.0f : dz;
        f4 h[4 * VB1];
#pragma unroll
        for (int v = 0; v < VB1; ++v) {
            f16v a;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f4 t = *reinterpret_cast<const f4 *>(qrow + 32 * v + 8 * q);
                a[4 * q] = t.x; a[4 * q + 1] = t.y; a[4 * q + 2] = t.z; a[4 * q + 3] = t.w;
            }
            const int ch = 32 * v + col;
            const float *wr = P.w1 + (ch >> 4) * 64 + (ch & 15);
            a = mfma_f32x2(wr[16 * hh], b0, a);
            a = mfma_f32x2(wr[16 * (2 + hh)], b1, a);
#pragma unroll
            for (int q = 0; q < 4; ++q) h[4 * v + q] = relu_med4((f4){a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]}, kinf);
        }
        // layer 2 (C1 -> 64) on the split path, the position's activations scaled by its own power of two; ReLU after the max
        const LaneScale sc = lane_scale32(h);
        const float cs = sc.inv * winv;
        f16v acc[2];
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[v][e] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            u4v bp[2];
            split2(h[2 * s], h[2 * s + 1], sc.s, bp);
            u4v fr[2][2];
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int p = 0; p < 2; ++p) fr[v][p] = __builtin_bit_cast(u4v, s_img[((s * 2 + v) * 2 + p) * 64 + lane]);
#define RTK_SA_MM(pa, pb) acc[0] = mfma_h(fr[0][pa], bp[pb], acc[0]); acc[1] = mfma_h(fr[1][pa], bp[pb], acc[1]);
            RTK_SA_MM(1, 0) RTK_SA_MM(0, 1) RTK_SA_MM(0, 0)
#undef RTK_SA_MM
        }
        // The maximum over the neighbours by a transposing reduction (fused_common.h): the eight f4 of a lane (v, q) end as ONE (32
        // neighbours: the two v through v_permlane16_swap) or two (16 neighbours); lane (hh, col) then holds q = 2 (bit 3 of col) +
        // (bit 2 of col) and -- 32 neighbours -- v = bit 4 of col, and the first lane of each quad stores.  Bias and scale BEFORE the
        // maximum (an fma the compiler knows: it places the wait states an MFMA result needs; the position's scale differs lane by lane).
        f4 m[2][4];
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                m[v][q] = scale_bias4((f4){acc[v][4 * q], acc[v][4 * q + 1], acc[v][4 * q + 2], acc[v][4 * q + 3]}, cs,
                                      *reinterpret_cast<const f4 *>(P.bias2 + 32 * v + 8 * q + 4 * hh));
        const int qo = 2 * ((col >> 3) & 1) + ((col >> 2) & 1);
        float *o = P.out + (long)c * P.out_pitch + P.out_offset + 4 * hh + 8 * qo;
        if constexpr (NS == 32) {
            f4 t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = wave_max_pair16(m[0][q], m[1][q], kinf);
            const f4 r = relu_med4(row_max16_transpose4(t[0], t[1], t[2], t[3]), kinf);
            if (valid && (col & 3) == 0) *reinterpret_cast<f4 *>(o + 32 * ((col >> 4) & 1)) = r;
        } else {
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const f4 r = relu_med4(row_max16_transpose4(m[v][0], m[v][1], m[v][2], m[v][3]), kinf);
                if (valid && (col & 3) == 0) *reinterpret_cast<f4 *>(o + 32 * v) = r;
            }
        }
    }
}

}  // namespace

extern "C" int rtk_pack_split_layer(int cout, int cin, const float *w, int transposed, void *image, float *inv_scale, rtk_stream_t stream) {
    RTK_REQUIRE(cout > 0 && cin > 0 && cout % 32 == 0 && cin % 32 == 0 && w && image && inv_scale, "pack_split_layer: bad arguments");
    RTK_REQUIRE((long)cout * cin <= (1L << 22), "pack_split_layer: more than 2^22 weights (every workgroup scans the matrix for its scale)");
    const int slots = (cin / 16) * (cout / 32) * 64;
    pack_split_kernel<false><<<(slots + 255) / 256, 256, 0, (hipStream_t)stream>>>(cout, cin, w, transposed, (u4v *)image, inv_scale);
    RTK_CHECK_LAUNCH("pack_split_layer");
    return RTK_OK;
}

extern "C" int rtk_pack_split_layer16(int cout, int cin, const float *w, int transposed, void *image, float *inv_scale, rtk_stream_t stream) {
    RTK_REQUIRE(cout > 0 && cin > 0 && cout % 32 == 0 && cin % 32 == 0 && w && image && inv_scale, "pack_split_layer16: bad arguments");
    RTK_REQUIRE((long)cout * cin <= (1L << 22), "pack_split_layer16: more than 2^22 weights (every workgroup scans the matrix for its scale)");
    const int slots = (cin / 32) * (cout / 16) * 64;
    pack_split_kernel<true><<<(slots + 255) / 256, 256, 0, (hipStream_t)stream>>>(cout, cin, w, transposed, (u4v *)image, inv_scale);
    RTK_CHECK_LAUNCH("pack_split_layer16");
    return RTK_OK;
}

extern "C" int rtk_split_mlp2(int positions, const float *x, const void *images, const float *image_scales, const float *bias1,
                              const float *bias2, float *y, rtk_stream_t stream) {
    RTK_REQUIRE(positions > 0 && x && images && image_scales && bias1 && bias2 && y, "split_mlp2: bad arguments");
    const int tiles = (positions + 32 * SP_NW - 1) / (32 * SP_NW);
    split_mlp2_kernel<<<tiles < 256 ? tiles : 256, 64 * SP_NW, 0, (hipStream_t)stream>>>(positions, x, (const f4 *)images, image_scales, bias1, bias2, y);
    RTK_CHECK_LAUNCH("split_mlp2");
    return RTK_OK;
}

static int cv_split_fill(const char *who, CvSplitParams &P, int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                         const int64_t *knn_idx, const void *split_images, const float *image_scales, const rtk_layer_t *wn, dim3 &grid) {
    RTK_REQUIRE(samples > 0 && samples <= 65535 && n1 > 0 && n2 >= 16 && xyz1 && xyz2 && knn_idx && split_images && image_scales,
                "%s: bad arguments", who);
    RTK_REQUIRE(wn && wn[0].w_packed && wn[1].w_packed && wn[2].w_packed && wn[1].bias && wn[2].bias && wn[1].cin16 == 1 &&
                wn[1].cout16 == 1 && wn[2].cin16 == 1 && wn[2].cout16 == 16, "%s: bad WeightNet layers", who);
    P.samples = samples; P.n1 = n1; P.n2 = n2;
    P.xyz1 = xyz1; P.xyz2 = xyz2; P.knn = knn_idx;
    P.blob = reinterpret_cast<const f4 *>(split_images);
    P.wsc = image_scales;
    P.wn.wa = wn[0].w_packed; P.wn.wb = wn[1].w_packed; P.wn.wc = wn[2].w_packed; P.wn.bb = wn[1].bias; P.wn.bc = wn[2].bias;
    P.p1 = P.p2 = P.st = P.wd = P.bias2 = P.bias3 = nullptr;
    P.out = nullptr; P.out_pitch = 0; P.sv1 = P.sv2 = P.sv3 = nullptr; P.mk1 = P.mk2 = nullptr; P.amax = nullptr;
    const int groups = (n1 + 2 * SP_NW - 1) / (2 * SP_NW);
    // one workgroup per CU (the tile keeps the whole register file); the rest is looped.  (Measured and rejected: 2 or 4 queued
    // workgroups per CU to shorten the tail when other kernels of the pipelined batches hold CUs -- 1 to 1.5 % slower.)
    int gx = 256 / samples;
    if (gx < 1) gx = 1;
    if (gx > groups) gx = groups;
    grid = rtk_xcd_grid(samples, gx, P.gx);
    return RTK_OK;
}

// compute units of the current device (one workgroup of the cost-volume kernels per CU); 256 if the runtime does not say
static int cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) return 256;
    return n;
}

static int cv_split_forward(const char *who, int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                            const float *p1, const float *p2, const float *wd_packed, const void *split_images, const float *image_scales,
                            const float *bias2, const float *bias3, const rtk_layer_t *wn, float *out, int out_pitch, float *a1, float *a2,
                            float *a3, void *mask1, void *mask2, float *amax, int workgroups, rtk_stream_t stream,
                            const float *sample_term = nullptr, bool global_consts = false, bool tile16 = false) {
    CvSplitParams P;
    dim3 grid;
    if (cv_split_fill(who, P, samples, n1, n2, xyz1, xyz2, knn_idx, split_images, image_scales, wn, grid) != RTK_OK) return RTK_ERR_INVALID;
    RTK_REQUIRE(p1 && p2 && wd_packed && bias2 && bias3 && out, "%s: bad arguments", who);
    RTK_REQUIRE((double)samples * n2 <= 4194304.0, "%s: more than 2^22 rows in p2 (32-bit byte offsets of the row requests): split the batch", who);
    RTK_REQUIRE(out_pitch % 4 == 0 && out_pitch >= 256, "%s: bad out_pitch", who);
    const bool save = a1 != nullptr;
    RTK_REQUIRE(!save || ((double)samples * n1 * 16.0 * 1024.0 < 4294967296.0), "%s: more than 4 GiB per saved activation (32-bit row "
                "offsets): split the batch", who);
    P.p1 = p1; P.p2 = p2; P.st = sample_term; P.wd = wd_packed; P.bias2 = bias2; P.bias3 = bias3; P.out = out; P.out_pitch = out_pitch;
    P.sv1 = a1; P.sv2 = a2; P.sv3 = a3; P.mk1 = (uint2 *)mask1; P.mk2 = (uint2 *)mask2; P.amax = amax;
    if (samples % 8 == 0) {      // flattened tiles (see the kernel): `workgroups` of them, a multiple of 8, at most one per tile
        const int tiles_x = (samples / 8) * ((n1 + 2 * SP_NW - 1) / (2 * SP_NW));
        int per_xcd = (workgroups > 0 ? workgroups : cu_count()) / 8;
        if (per_xcd < 1) per_xcd = 1;
        if (per_xcd > tiles_x) per_xcd = tiles_x;
        P.gx = 8 * per_xcd;
        grid = dim3(P.gx);
    }
    static_assert(2 * SP_NW == CV16_NW, "both tiles take eight points per workgroup iteration: one grid rule");
    if (tile16) cost_volume_split_kernel16<<<grid, 64 * CV16_NW, 0, (hipStream_t)stream>>>(P);
    else if (save) cost_volume_split_kernel<true><<<grid, 64 * SP_NW, 0, (hipStream_t)stream>>>(P);
    else if (global_consts) cost_volume_split_kernel<false, false><<<grid, 64 * SP_NW, 0, (hipStream_t)stream>>>(P);
    else cost_volume_split_kernel<false><<<grid, 64 * SP_NW, 0, (hipStream_t)stream>>>(P);
    RTK_CHECK_LAUNCH(who);
    return RTK_OK;
}

extern "C" int rtk_cost_volume_split(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                     const float *p1, const float *p2, const float *wd_packed, const void *split_images,
                                     const float *image_scales, const float *bias2, const float *bias3, const rtk_layer_t *wn, float *out,
                                     int out_pitch, rtk_stream_t stream) {
    return cv_split_forward("cost_volume_split", samples, n1, n2, xyz1, xyz2, knn_idx, p1, p2, wd_packed, split_images, image_scales, bias2, bias3,
                            wn, out, out_pitch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int rtk_cost_volume_split_shared(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                            const float *p1, const float *p2, const float *wd_packed, const void *split_images,
                                            const float *image_scales, const float *bias2, const float *bias3, const rtk_layer_t *wn,
                                            float *out, int out_pitch, int workgroups, rtk_stream_t stream) {
    RTK_REQUIRE(workgroups >= 0, "cost_volume_split_shared: workgroups = %d", workgroups);
    return cv_split_forward("cost_volume_split_shared", samples, n1, n2, xyz1, xyz2, knn_idx, p1, p2, wd_packed, split_images, image_scales,
                            bias2, bias3, wn, out, out_pitch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, workgroups, stream);
}

extern "C" int rtk_cost_volume_split_gconst(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                            const float *p1, const float *p2, const float *wd_packed, const void *split_images,
                                            const float *image_scales, const float *bias2, const float *bias3, const rtk_layer_t *wn,
                                            float *out, int out_pitch, int workgroups, rtk_stream_t stream) {
    RTK_REQUIRE(workgroups >= 0, "cost_volume_split_gconst: workgroups = %d", workgroups);
    return cv_split_forward("cost_volume_split_gconst", samples, n1, n2, xyz1, xyz2, knn_idx, p1, p2, wd_packed, split_images, image_scales,
                            bias2, bias3, wn, out, out_pitch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, workgroups, stream, nullptr, true);
}

extern "C" int rtk_cost_volume_split_term(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                          const float *p1, const float *p2, const float *sample_term, const float *wd_packed,
                                          const void *split_images, const float *image_scales, const float *bias2, const float *bias3,
                                          const rtk_layer_t *wn, float *out, int out_pitch, int workgroups, rtk_stream_t stream) {
    RTK_REQUIRE(workgroups >= 0 && sample_term, "cost_volume_split_term: workgroups = %d, sample_term = %p", workgroups, (const void *)sample_term);
    return cv_split_forward("cost_volume_split_term", samples, n1, n2, xyz1, xyz2, knn_idx, p1, p2, wd_packed, split_images, image_scales,
                            bias2, bias3, wn, out, out_pitch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, workgroups, stream, sample_term);
}

extern "C" int rtk_cost_volume_split16_shared(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                              const float *p1, const float *p2, const float *wd_packed, const void *split_images16,
                                              const float *image_scales, const float *bias2, const float *bias3, const rtk_layer_t *wn,
                                              float *out, int out_pitch, int workgroups, rtk_stream_t stream) {
    RTK_REQUIRE(workgroups >= 0, "cost_volume_split16_shared: workgroups = %d", workgroups);
    return cv_split_forward("cost_volume_split16_shared", samples, n1, n2, xyz1, xyz2, knn_idx, p1, p2, wd_packed, split_images16, image_scales,
                            bias2, bias3, wn, out, out_pitch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, workgroups, stream, nullptr, false,
                            true);
}

extern "C" int rtk_cost_volume_split16_term(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                            const float *p1, const float *p2, const float *sample_term, const float *wd_packed,
                                            const void *split_images16, const float *image_scales, const float *bias2, const float *bias3,
                                            const rtk_layer_t *wn, float *out, int out_pitch, int workgroups, rtk_stream_t stream) {
    RTK_REQUIRE(workgroups >= 0 && sample_term, "cost_volume_split16_term: workgroups = %d, sample_term = %p", workgroups, (const void *)sample_term);
    return cv_split_forward("cost_volume_split16_term", samples, n1, n2, xyz1, xyz2, knn_idx, p1, p2, wd_packed, split_images16, image_scales,
                            bias2, bias3, wn, out, out_pitch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, workgroups, stream, sample_term,
                            false, true);
}

extern "C" int rtk_cost_volume_split_train(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                           const float *p1, const float *p2, const float *wd_packed, const void *split_images,
                                           const float *image_scales, const float *bias2, const float *bias3, const rtk_layer_t *wn,
                                           float *out, int out_pitch, float *a1, float *a2, float *a3, void *mask1, void *mask2,
                                           float *act_amax, rtk_stream_t stream) {
    RTK_REQUIRE(a1 && a2 && a3 && mask1 && mask2, "cost_volume_split_train: null activation buffer");
    return cv_split_forward("cost_volume_split_train", samples, n1, n2, xyz1, xyz2, knn_idx, p1, p2, wd_packed, split_images, image_scales,
                            bias2, bias3, wn, out, out_pitch, a1, a2, a3, mask1, mask2, act_amax, 0, stream);
}

extern "C" int rtk_cost_volume_bwd_split(int samples, int n1, int n2, const float *xyz1, const float *xyz2, const int64_t *knn_idx,
                                         const void *split_images_t, const float *image_scales_t, const rtk_layer_t *wn, const float *dout,
                                         int dout_pitch,
                                         const float *a3, const void *mask1, const void *mask2, float *dz1, float *dz2, float *dz3,
                                         float *dq3, float *d4, float *dp1, float *dpd, float *dt2, float *dbias_rows,
                                         float *dz_amax, rtk_stream_t stream) {
    CvSplitBwdParams Q;
    dim3 grid;
    if (cv_split_fill("cost_volume_bwd_split", Q.f, samples, n1, n2, xyz1, xyz2, knn_idx, split_images_t, image_scales_t, wn, grid) != RTK_OK)
        return RTK_ERR_INVALID;
    RTK_REQUIRE(dout && mask1 && mask2 && a3 && dz1 && dz2 && dz3 && dq3 && d4 && dp1 && dpd && dt2, "cost_volume_bwd_split: bad arguments");
    RTK_REQUIRE((double)samples * n1 * 16.0 * 1024.0 < 4294967296.0, "cost_volume_bwd_split: more than 4 GiB per (position, 256) tensor "
                "(32-bit row offsets): split the batch");
    RTK_REQUIRE(dout_pitch % 4 == 0 && dout_pitch >= 256, "cost_volume_bwd_split: bad dout_pitch");
    Q.dout = dout; Q.dout_pitch = dout_pitch; Q.a3 = a3; Q.mk1 = (const uint2 *)mask1; Q.mk2 = (const uint2 *)mask2;
    Q.dz1 = dz1; Q.dz2 = dz2; Q.dz3 = dz3; Q.dq3 = dq3; Q.d4 = d4; Q.dp1 = dp1; Q.dpd = dpd; Q.dt2 = dt2; Q.dbrows = dbias_rows;
    Q.f.amax = dz_amax;
    cost_volume_bwd_split_kernel<<<grid, 64 * SP_NW, 0, (hipStream_t)stream>>>(Q);
    RTK_CHECK_LAUNCH("cost_volume_bwd_split");
    return RTK_OK;
}

template <bool PIPE>
static int sa_scale_split_launch(int samples, int n, int npoint, int nsample, const float *xyz, const float *new_xyz, const int *idx,
                                 const float *q, int q_pitch, int c1, const float *w1xyz_packed, const void *split_image,
                                 const float *image_scale, const float *bias2, float *out, int out_pitch, int out_offset,
                                 const int *src_nuniq, const int *dst_nuniq, rtk_stream_t stream) {
    RTK_REQUIRE(samples > 0 && n > 0 && npoint > 0 && xyz && new_xyz && idx && q && w1xyz_packed && split_image && image_scale && bias2 && out,
                "sa_scale_split: bad arguments");
    RTK_REQUIRE(q_pitch % 4 == 0 && out_pitch % 4 == 0 && out_offset % 4 == 0, "sa_scale_split: pitches/offset must be multiples of 4");
    RTK_REQUIRE((long)samples * npoint * nsample < 0x7fffffffL && (long)samples * n < 0x7fffffffL && samples <= 65535,
                "sa_scale_split: problem too large for 32-bit indexing");
    RTK_REQUIRE(q_pitch >= c1, "sa_scale_split: q_pitch is smaller than the row's %d channels", c1);
    // the pipelined loop addresses a sample's q rows by 32-bit byte offsets (SaRows); the serial one serves whatever they cannot reach
    if constexpr (PIPE) {
        if ((double)n * q_pitch * 4.0 >= 4294967296.0)
            return sa_scale_split_launch<false>(samples, n, npoint, nsample, xyz, new_xyz, idx, q, q_pitch, c1, w1xyz_packed, split_image, image_scale,
                                                bias2, out, out_pitch, out_offset, src_nuniq, dst_nuniq, stream);
    }
    SaSplitParams P;
    P.samples = samples; P.n = n; P.npoint = npoint;
    P.xyz = xyz; P.new_xyz = new_xyz; P.idx = idx; P.q = q; P.q_pitch = q_pitch; P.w1 = w1xyz_packed;
    P.image = reinterpret_cast<const f4 *>(split_image); P.wsc = image_scale; P.bias2 = bias2;
    P.out = out; P.out_pitch = out_pitch; P.out_offset = out_offset; P.src_nuniq = src_nuniq; P.dst_nuniq = dst_nuniq;
    const int units = (npoint + 32 / nsample - 1) / (32 / nsample);
    int bx = (units + 3) / 4;
    while ((long)bx * samples > SA_WGS_TARGET && bx > 1) bx = (bx + 1) / 2;      // few, fat workgroups: the LDS image fill is paid per workgroup
    const dim3 blocks = rtk_xcd_grid(samples, bx, P.gx);
    hipStream_t s = (hipStream_t)stream;
    if (nsample == 32 && c1 == 64) sa_scale_split_kernel<32, 64, PIPE><<<blocks, 256, 0, s>>>(P);
    else if (nsample == 16 && c1 == 64) sa_scale_split_kernel<16, 64, PIPE><<<blocks, 256, 0, s>>>(P);
    else if (nsample == 16 && c1 == 32) sa_scale_split_kernel<16, 32, PIPE><<<blocks, 256, 0, s>>>(P);
    else {
        rtk_set_error("sa_scale_split: no kernel instance for nsample=%d, %d -> 64 channels", nsample, c1);
        return RTK_ERR_UNSUPPORTED;
    }
    RTK_CHECK_LAUNCH("sa_scale_split");
    return RTK_OK;
}

extern "C" int rtk_sa_scale_split(int samples, int n, int npoint, int nsample, const float *xyz, const float *new_xyz, const int *idx,
                                  const float *q, int q_pitch, int c1, const float *w1xyz_packed, const void *split_image,
                                  const float *image_scale, const float *bias2, float *out, int out_pitch, int out_offset,
                                  const int *src_nuniq, const int *dst_nuniq, rtk_stream_t stream) {
    return sa_scale_split_launch<true>(samples, n, npoint, nsample, xyz, new_xyz, idx, q, q_pitch, c1, w1xyz_packed, split_image, image_scale,
                                       bias2, out, out_pitch, out_offset, src_nuniq, dst_nuniq, stream);
}

extern "C" int rtk_sa_scale_split_serial(int samples, int n, int npoint, int nsample, const float *xyz, const float *new_xyz, const int *idx,
                                         const float *q, int q_pitch, int c1, const float *w1xyz_packed, const void *split_image,
                                         const float *image_scale, const float *bias2, float *out, int out_pitch, int out_offset,
                                         const int *src_nuniq, const int *dst_nuniq, rtk_stream_t stream) {
    return sa_scale_split_launch<false>(samples, n, npoint, nsample, xyz, new_xyz, idx, q, q_pitch, c1, w1xyz_packed, split_image, image_scale,
                                        bias2, out, out_pitch, out_offset, src_nuniq, dst_nuniq, stream);
}
