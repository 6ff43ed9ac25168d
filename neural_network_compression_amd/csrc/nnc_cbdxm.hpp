// nnc_cbdxm.hpp -- the label load of the dx MFMA kernels of the two byte forms (k_cbdx_mfma, k_cbdx_mfma_grouped) on bf16 / fp16
// activations.  The main loop of all five dx kernels is the tile's own, hm_accumulate (nnc_cbmfma.hpp), which
// the forward kernels run too (section 31); a dx kernel keeps its signature, its LDS carve-up, its table fill, the decode of its
// index form and hm_store_y.
#pragma once
#include "nnc_cbmfma.hpp"

// The byte forms: a thread owns one index row and 16 consecutive o of a step, which lie one after the other in memory.
// The n (<= 16) labels p[0 .. n), packed as they lie in memory (little endian) into 4 * sizeof(LT) words; the absent ones 0.  p is
// dereferenced only where n > 0.
template <typename LT>
__device__ __forceinline__ void dxm_load_labels(const LT *p, int n, uint32_t (&w)[4 * sizeof(LT)])
{
    constexpr int LB = sizeof(LT), NW = 4 * LB, PER = 4 / LB;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (n == 16 && a % 16 == 0) {
#pragma unroll
        for (int q = 0; q < LB; ++q) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
            w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
        }
    } else if (n == 16 && a % 4 == 0) {
#pragma unroll
        for (int d = 0; d < NW; ++d) w[d] = reinterpret_cast<const uint32_t *>(p)[d];
    } else {
#pragma unroll
        for (int d = 0; d < NW; ++d) w[d] = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < n) w[j / PER] |= (uint32_t)p[j] << (8 * LB * (j % PER));
    }
}
