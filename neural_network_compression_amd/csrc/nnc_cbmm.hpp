// nnc_cbmm.hpp -- what the codebook matmul (nnc_cbmm.hip), its bitmap-sparse sibling (nnc_cbsp.hip) and its backward pass
// (nnc_cbgrad.hip) share: the launch constants, the per-bank LDS codebook layout, the label-row loads of the stream kernels and the
// register-blocked FMA step of the tiled kernels.  The 2- and 4-bit packed form (nnc_cbpk.hip) takes cb_fill, tb_tile_fma and
// the split-K combine from here.
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

// y[idx] = the split-K partials part[s][idx], s < splits, summed in an order that depends on `splits` alone, + bias[idx % ncols],
// ReLU (k_cbmm_reduce, nnc_cbmm.hip; splits = 0: y = bias or 0), launched on `s`: NNC_OK or the launch error
int cbmm_reduce(const float *part, long long splits, long long mn, long long ncols, const float *bias, int relu, float *y, hipStream_t s);

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

// ------------------------------------------------------------------ device helpers
// the table: `entries` values (centers, then zeros), `1 << cshift` copies of each, copy c of entry j at j * copies + c.  The
// centres come from global memory once per workgroup into `stage`; the copies are made from LDS (a loop of global loads per copy
// was a chain of L2 round trips in front of every workgroup).
__device__ __forceinline__ void cb_fill(float *cb, float *stage, const float *__restrict__ centers, int k, int entries, int cshift)
{
    for (int j = threadIdx.x; j < entries; j += blockDim.x) stage[j] = j < k ? centers[j] : 0.0f;
    __syncthreads();
    const int words = entries << cshift;
#pragma unroll 8
    for (int w = threadIdx.x; w < words; w += blockDim.x) cb[w] = stage[w >> cshift];
}

template <int VB> struct Chunk;
template <> struct Chunk<4> { using T = uint32_t; };
template <> struct Chunk<8> { using T = uint2; };
template <> struct Chunk<16> { using T = uint4; };

template <int VB>
__device__ __forceinline__ void load_chunk(const unsigned char *p, uint32_t *w)
{
    const typename Chunk<VB>::T v = *reinterpret_cast<const typename Chunk<VB>::T *>(p);
    __builtin_memcpy(w, &v, VB);
}

// o[d] = bytes [s + 4d, s + 4d + 4) of the 2N-dword window w (s < 4N, uniform over the wave)
template <int N>
__device__ __forceinline__ void funnel(const uint32_t *w, uint32_t s, uint32_t *o)
{
    const uint32_t q = s >> 2, r = s & 3;
    uint32_t v[N + 1];
#pragma unroll
    for (int d = 0; d <= N; ++d) {
        uint32_t t = w[d];
#pragma unroll
        for (int qq = 1; qq < N; ++qq) t = q == (uint32_t)qq ? w[d + qq] : t;
        v[d] = t;
    }
#pragma unroll
    for (int d = 0; d < N; ++d) o[d] = __builtin_amdgcn_alignbyte(v[d + 1], v[d], r);
}
