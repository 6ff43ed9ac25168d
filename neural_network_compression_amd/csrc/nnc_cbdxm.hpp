// nnc_cbdxm.hpp -- what the dx MFMA kernels on bf16 / fp16 activations share: their main loop, run by all five
// (k_cbdx_mfma, k_cbspdx_mfma, k_cbpkdx_mfma, k_cbdx_mfma_grouped, k_cbpkdx_mfma_grouped), and the label load of the two byte forms.
// A kernel keeps its signature, its LDS carve-up, its table fill, the decode of its index form and hm_store_y.
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

// acc = the 128 (r) x 128 (i) tile of dx = g W^T over the columns [T.k_lo, T.k_hi) of the split, in steps of HM_BK: T.m0 is the first
// row of g, T.n0 the first index row.  gs [HM_BM][HM_LD] is the g image, row-major in o (hm_load_x / hm_store_x with ncols as the
// row length); ws [HM_BN][HM_LD] the W^T image [i][o], which the kernel's two callables fill: load_w(ob) fetches what the thread
// needs of its index row for the step at ob, one step ahead of the MFMAs that consume it, and store_w(ob) looks it up and writes
// the thread's 16 values with hm_store_w.  ahead(ob), behind the loads of g, is for a form that requests something for the step
// after ob there (the bitmap word of k_cbspdx_mfma).  The first barrier of the loop also orders what the caller wrote to LDS before
// it (the table).
struct DxmNothing {
    __device__ __forceinline__ void operator()(long long) const {}
};

template <typename XT, bool XVEC, typename LoadW, typename StoreW, typename Ahead = DxmNothing>
__device__ __forceinline__ void dxm_accumulate(const XT *g, long long m, long long ncols, const HmTile T, XT *gs, const XT *ws,
                                               typename HFrag<XT>::C (&acc)[2][2], LoadW load_w, StoreW store_w, Ahead ahead = Ahead())
{
    uint4 gf[2];
    auto load = [&](long long ob) {
        load_w(ob);
#pragma unroll
        for (int i = 0; i < 2; ++i) gf[i] = hm_load_x<XT, XVEC>(g, m, ncols, T.m0, ob, T.k_hi, T.t + i * HM_THREADS);
        ahead(ob);
    };

    hm_clear<XT>(acc);
    load(T.k_lo);
    for (long long ob = T.k_lo; ob < T.k_hi; ob += HM_BK) {
        __syncthreads();   // the table is filled (first step); the images of the step before have been read
        store_w(ob);
#pragma unroll
        for (int i = 0; i < 2; ++i) hm_store_x(gs, T.t + i * HM_THREADS, gf[i]);
        __syncthreads();
        if (ob + HM_BK < T.k_hi) load(ob + HM_BK);
        hm_step(gs, ws, T.wm, T.wn, T.fr, T.fh, acc);
    }
}
