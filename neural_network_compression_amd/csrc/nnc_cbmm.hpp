// nnc_cbmm.hpp -- what the codebook matmul (nnc_cbmm.hip) and its bitmap-sparse sibling (nnc_cbsp.hip) share: the launch
// constants, the per-bank LDS codebook layout and the register-blocked FMA step of the tiled kernels.
#pragma once
#include "nnc_common.hpp"

#define CB_WAVES 4
#define CB_THREADS (CB_WAVES * WAVE)
#define CB_UNROLL 8               // label rows in flight per wave
#define CB_SKINNY_M 16
#define CB_U8_COPIES 32           // K <= 256 (uint8): 32 copies of a 256-entry table (zero-padded: no bounds test) = 32 KiB
#define CB_U16_WORDS 8448         // K > 256 (uint16): copies = the largest power of two with (K + 1) * copies <= this (33 KiB)
#define CB_PLAN_CUS 256           // the workspace query plans for this many CUs (the plan's splits never shrink with more)
#define TB_M 128
#define TB_N 128
#define TB_K 8

static inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// the per-bank table: entry j of lane l at word j * copies + (l mod copies), copies = 1 << cshift
template <typename LT> struct CbTable;
template <> struct CbTable<uint8_t> {
    __device__ static __forceinline__ int index(uint32_t l, int, int cshift, int lane) { return (int)((l << cshift) | (lane & ((1 << cshift) - 1))); }
};
template <> struct CbTable<uint16_t> {
    __device__ static __forceinline__ int index(uint32_t l, int k, int cshift, int lane)
    {
        return (int)((std::min(l, (uint32_t)k) << cshift) | (lane & ((1 << cshift) - 1)));   // entry k holds the out-of-range value
    }
};

// one TB_K step of the 128 x 128 tile: thread (tx, ty) adds xs[kk][ty*8 + a] * ws[kk][tx*8 + b] into acc[a][b], kk in order
__device__ __forceinline__ void tb_tile_fma(const float *xs, const float *ws, int tx, int ty, float (&acc)[8][8])
{
#pragma unroll
    for (int kk = 0; kk < TB_K; ++kk) {
        const float4 a0 = *reinterpret_cast<const float4 *>(xs + kk * TB_M + ty * 8);
        const float4 a1 = *reinterpret_cast<const float4 *>(xs + kk * TB_M + ty * 8 + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(ws + kk * TB_N + tx * 8);
        const float4 b1 = *reinterpret_cast<const float4 *>(ws + kk * TB_N + tx * 8 + 4);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = __builtin_fmaf(av[a], bv[b], acc[a][b]);
    }
}
