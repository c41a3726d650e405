// fused_patch.hip -- rtk_patch_cost on the 32-position tile (model_utils.py:238-248):
//
//     out[i] = sum over the 16 neighbours k of  relu(Wc.t2(d_ik) + bc) * feat[idx[i, k]],   t2 = the WeightNet's hidden layers on d_ik
//
// A wave owns TWO points x their 16 neighbours: the 32 columns of v_mfma_f32_32x32x2_f32, lane = 32 hh + col, a lane holds channels
// 32 v + 8 q + 4 hh + r of position col (the layout of the cost volume's output epilogue, fused_split.hip, with the gathered feature
// row in place of a3).  A workgroup of four waves takes eight points per iteration and strides over its sample's groups of eight.
//
//   * Constants.  The last WeightNet layer (K = 8 and the bias) of ALL eight 32-channel blocks lives in 40 registers per lane,
//     loaded once per wave: the bias enters as a k-slot of its own (operand 1), so a block is FIVE k-steps of two on a zero
//     accumulator -- (bias, 0) (4, 1) (5, 2) (6, 3) (7, -) -- and the tile loop reads no constant from memory but the hidden layers'
//     wave-uniform weights (scalar loads).  The k-slots are assigned so that every channel accumulates in the order of the 16-position
//     kernel (patch_cost_kernel, fused_group.hip: bias, 0, 4, 1, 5, 2, 6, 3, 7): the two kernels return the same bits.
//   * Rows.  A feature row is fetched exactly once, as contiguous runs: one global_load_lds per four positions moves 4 x 256 bytes (a
//     QUARTER row: two 32-channel blocks) into the wave's own 8 KiB of LDS; four rounds per tile, round r + 1 requested as soon as
//     round r's slots have been read into registers, the next tile's round 0 during the last two blocks of this one (its kNN
//     indices are requested behind round 0's wait, its coordinates before that round).  Slot p of a position's 256 bytes holds source
//     chunk p ^ (position & 15): the 16 lanes that read together hit 16 different bank groups.  Rows are addressed by 32-bit byte
//     offsets on a uniform base (the launcher checks the size) and only their first 1024 bytes are ever touched.
//   * The neighbour sum is the transposing reduction of fused_common.h over the 16 lanes of a DPP row, as in the 16-position kernel.
#include "rtk_common.h"
#include "rtk_fused.h"
#include "wn_tile.h"

namespace {

constexpr int PT_NW = 4;                     // waves per workgroup
constexpr int PT_PPW = 2 * PT_NW;            // points per workgroup iteration
constexpr int PT_SLAB_F4 = 32 * 16;          // f4 per wave: 32 positions x 16 slots of 16 bytes
#ifndef PT_WGS_TARGET
#define PT_WGS_TARGET 1024                   // workgroups per launch: the constants are loaded once per wave, the first round of a wave's
#endif                                       // first tile is exposed -- a workgroup should see several tiles

struct PtParams {
    int samples, n;
    const float *xyz;
    const int64_t *knn;
    const float *feat;
    unsigned row_bytes;     // feat_pitch * 4
    WnSplit wn;
    float *out;
    int out_pitch;
    int gx;                 // > 0: XCD-aware 1-D grid (rtk_decode_block)
};

// One round of row requests: instruction T serves positions 4 T .. 4 T + 3, lane L the 16-byte slot L & 15 of position 4 T + (L >> 4).
// ro[T]: byte offset of that position's row plus the (swizzled) source chunk of the lane's slot.
template <int R, int... T>
__device__ __forceinline__ void pt_rows_request(const char *feat, const unsigned (&ro)[8], f4 *rows, std::integer_sequence<int, T...>) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the previous round's reads have returned before their slots are overwritten
    // (uniform 64-bit base) + (32-bit per-lane offset): the SGPR-base form of the instruction, no 64-bit address arithmetic per lane
    const char *base = feat + 256 * R;
    (__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(base + ro[T]),
                                      (__attribute__((address_space(3))) void *)(rows + T * 64), 16, 0, 0), ...);
}
// this lane's eight slots of a round: channels 64 R + 32 vv + 8 q + 4 hh .. + 3 at h[4 vv + q]
__device__ __forceinline__ void pt_rows_read(const f4 *rows, int col, int hh, f4 (&h)[8]) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the round has landed
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = rows[col * 16 + ((2 * e + hh) ^ (col & 15))];
}
// row offsets of a tile's requests from the lanes that hold them (lane col and lane 32 + col: the row of position col)
__device__ __forceinline__ void pt_row_offsets(unsigned rowoff, int lane, unsigned (&ro)[8]) {
    const unsigned chunk = (unsigned)((lane & 15) ^ (lane >> 4));
#pragma unroll
    for (int T = 0; T < 8; ++T) ro[T] = (unsigned)__shfl((int)rowoff, 4 * T + (lane >> 4), 64) + ((chunk ^ (unsigned)((4 * T) & 15)) << 4);
}

__global__ __launch_bounds__(64 * PT_NW, 2) void patch_cost_tile_kernel(const PtParams P) {
    const float kinf = rtk_hidden_inf();
    __shared__ __attribute__((aligned(16))) f4 s_rows[PT_NW * PT_SLAB_F4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5, col = lane & 31, pp = col >> 4,
              j = col & 15;
    f4 *rows = s_rows + wave * PT_SLAB_F4;
    const char *featb = reinterpret_cast<const char *>(P.feat);
    int b, bx, nbx;
    rtk_decode_block(P.gx, b, bx, nbx);
    const int groups = (P.n + PT_PPW - 1) / PT_PPW;
    if (bx >= groups) return;
    // A operands of the eight blocks: A[i = col][k = hh] of the five k-steps, channel ch = 32 v + col
    //   hh = 0: bc[ch], Wc[ch][4], Wc[ch][5], Wc[ch][6], Wc[ch][7]        hh = 1: Wc[ch][0], Wc[ch][1], Wc[ch][2], Wc[ch][3], 0
    float wa[8][5];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int ch = 32 * v + col;
        const f4 w = ldc4(P.wn.wc + ((ch >> 4) * 64 + 16 * (1 - hh) + (ch & 15)) * 4);      // Wc[ch][4 (1 - hh) .. + 3]
        const float bias = ldc(P.wn.bc + ch);
        wa[v][0] = hh ? w.x : bias; wa[v][1] = hh ? w.y : w.x; wa[v][2] = hh ? w.z : w.y; wa[v][3] = hh ? w.w : w.z; wa[v][4] = hh ? 0.f : w.w;
    }
    // tile state: this lane's point (clamped: a point that does not exist is computed as the sample's last and not stored)
    const int pt = bx * PT_PPW + 2 * wave + pp;
    bool valid = pt < P.n;
    long i = (long)b * P.n + (valid ? pt : P.n - 1);
    const long nb = (long)b * P.n + (long)P.knn[i * 16 + j];
    unsigned ro[8];
    pt_row_offsets((unsigned)nb * P.row_bytes, lane, ro);
    pt_rows_request<0>(featb, ro, rows, std::make_integer_sequence<int, 8>{});
    float dx = __fsub_rn(P.xyz[nb * 3], P.xyz[i * 3]), dy = __fsub_rn(P.xyz[nb * 3 + 1], P.xyz[i * 3 + 1]),
          dz = __fsub_rn(P.xyz[nb * 3 + 2], P.xyz[i * 3 + 2]);
    for (int G = bx; G < groups; G += nbx) {
        asm volatile("" ::: "memory");
        // the next tile's neighbour index (wave-uniform condition); without a next tile everything below re-requests this tile's rows
        const bool more = G + nbx < groups;
        const int ptn = (more ? G + nbx : G) * PT_PPW + 2 * wave + pp;
        const bool validn = ptn < P.n;
        const long in_ = (long)b * P.n + (validn ? ptn : P.n - 1);
        float t2[8];
        wn_hidden<true>(P.wn, dx, dy, dz, t2);
        // B[k = hh][col] of the five k-steps
        const float bk[5] = {hh ? t2[0] : 1.0f, hh ? t2[1] : t2[4], hh ? t2[2] : t2[5], hh ? t2[3] : t2[6], hh ? 0.f : t2[7]};
        float *o = P.out + i * P.out_pitch + 4 * hh;
        f4 h[8];
        auto block = [&](int v) {
            f16v w = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 5; ++st) w = mfma_f32x2(wa[v][st], bk[st], w);
            f4 r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) r[q][e] = relu1(w[4 * q + e], kinf) * h[4 * (v & 1) + q][e];
            // sum over the 16 neighbours by the transposing reduction (fused_common.h): lane j ends with slot q = 2 (bit 3 of j) + (bit 2
            // of j) of the block, the first lane of each quad stores
            const f4 t = row_sum16_transpose4(r[0], r[1], r[2], r[3]);
            if (valid && (j & 3) == 0) *reinterpret_cast<f4 *>(o + 32 * v + 8 * (2 * ((j >> 3) & 1) + ((j >> 2) & 1))) = t;
        };
        constexpr auto seq8 = std::make_integer_sequence<int, 8>{};
        pt_rows_read(rows, col, hh, h);
        pt_rows_request<1>(featb, ro, rows, seq8);
        const long knn_next = (long)P.knn[in_ * 16 + j];      // (behind round 0's wait, which would otherwise wait for it as well)
        block(0); block(1);
        pt_rows_read(rows, col, hh, h);
        pt_rows_request<2>(featb, ro, rows, seq8);
        block(2); block(3);
        pt_rows_read(rows, col, hh, h);
        pt_rows_request<3>(featb, ro, rows, seq8);
        block(4); block(5);
        pt_rows_read(rows, col, hh, h);
        // ---- next tile: its coordinates, then round 0 of its rows, under the last two blocks ------------------------------------
        const long nbn = (long)b * P.n + knn_next;
        float cn[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) { cn[c] = P.xyz[nbn * 3 + c]; cn[3 + c] = P.xyz[in_ * 3 + c]; }
        pt_row_offsets((unsigned)nbn * P.row_bytes, lane, ro);
        pt_rows_request<0>(featb, ro, rows, seq8);
        block(6); block(7);
        valid = validn; i = in_;
        dx = __fsub_rn(cn[0], cn[3]); dy = __fsub_rn(cn[1], cn[4]); dz = __fsub_rn(cn[2], cn[5]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the last (unused) round has landed before the wave's LDS is released
}

}  // namespace

// The 16-position kernel (fused_group.hip) serves the channel-major output and whatever the tile's 32-bit row offsets cannot address.
extern "C" int rtk_patch_cost(int samples, int n, const float *xyz, const int64_t *knn_idx, const float *feat, int feat_pitch,
                              const rtk_layer_t *wn, float *out, int out_pitch, int out_channel_major, rtk_stream_t stream) {
    if (out_channel_major || samples <= 0 || n <= 0 || feat_pitch <= 0 || (double)samples * n * feat_pitch * 4.0 >= 4294967296.0)
        return rtk_patch_cost_wave16(samples, n, xyz, knn_idx, feat, feat_pitch, wn, out, out_pitch, out_channel_major, stream);
    RTK_REQUIRE(samples <= 65535 && n >= 16 && xyz && knn_idx && feat && out && feat_pitch % 4 == 0 && feat_pitch >= 256,
                "patch_cost: bad arguments");
    RTK_REQUIRE(out_pitch % 4 == 0 && out_pitch >= 256, "patch_cost: bad out_pitch");
    RTK_REQUIRE(wn && wn[0].w_packed && wn[1].w_packed && wn[2].w_packed && wn[1].bias && wn[2].bias && wn[1].cin16 == 1 &&
                wn[1].cout16 == 1 && wn[2].cin16 == 1, "patch_cost: bad WeightNet layers");
    RTK_REQUIRE(wn[2].cout16 == 16, "patch_cost: WeightNet must produce 256 channels");
    PtParams P;
    P.samples = samples; P.n = n; P.xyz = xyz; P.knn = knn_idx; P.feat = feat; P.row_bytes = (unsigned)feat_pitch * 4u;
    P.wn.wa = wn[0].w_packed; P.wn.wb = wn[1].w_packed; P.wn.wc = wn[2].w_packed; P.wn.bb = wn[1].bias; P.wn.bc = wn[2].bias;
    P.out = out; P.out_pitch = out_pitch;
    int gx = (n + PT_PPW - 1) / PT_PPW;                                       // one tile per wave ...
    while ((long)gx * samples > PT_WGS_TARGET && gx > 1) gx = (gx + 1) / 2;   // ... halved until the launch has at most PT_WGS_TARGET workgroups
    const dim3 grid = rtk_xcd_grid(samples, gx, P.gx);
    patch_cost_tile_kernel<<<grid, 64 * PT_NW, 0, (hipStream_t)stream>>>(P);
    RTK_CHECK_LAUNCH("patch_cost");
    return RTK_OK;
}
