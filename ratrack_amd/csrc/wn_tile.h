// wn_tile.h -- what the kernels on the 32-position tile share besides the split layers (split_mfma.h): the fp32-input 32x32 matrix
// instruction, loads of kernel-lifetime constants, the WeightNet's hidden layers on wave-uniform weights and the one-instruction
// ReLU / maximum.  Tile layout (split_mfma.h): lane = 32 hh + col, a lane holds channels 32 v + 8 q + 4 hh + r of position col.
#pragma once
#include "fused_common.h"

typedef float f16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f16v mfma_f32x2(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// Loads of kernel-lifetime constants (weights, biases) through the constant address space: the compiler may move them over the
// kernel's stores (a plain global load stays behind every store it might alias -- in the cost volume's epilogue that put one exposed
// L2 round trip in front of each of the eight output blocks) and turns the wave-uniform ones into scalar loads.
__device__ __forceinline__ float ldc(const float *p) { return *(const __attribute__((address_space(4))) float *)p; }
__device__ __forceinline__ f4 ldc4(const float *p) { return *(const __attribute__((address_space(4))) f4 *)p; }

struct WnSplit {                  // WeightNet images as packed for the 16x16 kernels (fused_group.hip)
    const float *wa;              // [Wa | ba]: Wa[o][k] = wa[16 k + o], ba[o] = wa[48 + o]
    const float *wb, *wc;         // Wb[o][c] = wb[(16 (c / 4) + o) 4 + c % 4];  Wc[ch][k] = wc[((ch / 16) 64 + 16 (k / 4) + ch % 16) 4 + k % 4]
    const float *bb, *bc;
};

// WeightNet hidden layers (3 -> 8 -> 8, ReLU) of this lane's position: uniform weights, every lane its own direction.
// KSLOT_ORDER: the second layer accumulates its eight inputs in the order the k-slots of the 16x16x4 kernels imply (weightnet_hidden,
// fused_group.hip: slot g of step r holds channel 4 g + r, the 8 live channels come as 0, 4, 1, 5, 2, 6, 3, 7) instead of ascending
// -- the same bits as those kernels.  (The first layer's order is the same in both: x, y, z, bias.)
template <bool KSLOT_ORDER = false>
__device__ __forceinline__ void wn_hidden(const WnSplit &W, float dx, float dy, float dz, float (&t2)[8]) {
    float t1[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = __fmaf_rn(ldc(W.wa + o), dx, 0.f);
        a = __fmaf_rn(ldc(W.wa + 16 + o), dy, a);
        a = __fmaf_rn(ldc(W.wa + 32 + o), dz, a);
        t1[o] = fmaxf(__fadd_rn(a, ldc(W.wa + 48 + o)), 0.f);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = ldc(W.bb + o);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int c = KSLOT_ORDER ? 4 * (s & 1) + (s >> 1) : s;
            a = __fmaf_rn(ldc(W.wb + (16 * (c >> 2) + o) * 4 + (c & 3)), t1[c], a);
        }
        t2[o] = fmaxf(a, 0.f);
    }
}

// max(x, 0.1 x), max(x, 0) and max(x, y) in ONE instruction each.  fmaxf() costs two under IEEE mode -- hipcc first quiets a possible
// signalling NaN in every operand it did not compute itself (v_max_f32 x, x, x on each accumulator read): 32 extra VALU instructions
// per 32-channel block of the epilogue, 256 per layer boundary -- and a median with a literal +inf (v_med3_f32) is folded back into
// exactly that maxnum.  All are the median with a +inf the optimiser cannot see (an SGPR written by a volatile asm, once per
// kernel: rtk_hidden_inf): ReLU = med3(x, 0, inf), LeakyReLU = med3(x, 0.1 x, inf) (leaky_med4, fused_split.hip), max = med3(x, y, inf)
// -- instructions the compiler knows, so it places the wait states a matrix-core result needs itself (round 4's LeakyReLU was a
// written-out v_max_f32 that relied on the product in front of it for that).  Same bits as fmaxf for every input but a signalling
// NaN's payload: with a NaN operand v_med3 returns the minimum of the others, which is fmaxf's answer (0, or y) here.
__device__ __forceinline__ float rtk_hidden_inf() {
    float v;
    asm volatile("s_mov_b32 %0, 0x7f800000" : "=s"(v));
    return v;
}
__device__ __forceinline__ float relu1(float x, float inf) { return __builtin_amdgcn_fmed3f(x, 0.f, inf); }
__device__ __forceinline__ f4 relu_med4(f4 t, float inf) { return (f4){relu1(t.x, inf), relu1(t.y, inf), relu1(t.z, inf), relu1(t.w, inf)}; }
__device__ __forceinline__ float max1(float x, float y, float inf) { return __builtin_amdgcn_fmed3f(x, y, inf); }
__device__ __forceinline__ f4 max_med4(f4 a, f4 b, float inf) {
    return (f4){max1(a.x, b.x, inf), max1(a.y, b.y, inf), max1(a.z, b.z, inf), max1(a.w, b.w, inf)};
}
