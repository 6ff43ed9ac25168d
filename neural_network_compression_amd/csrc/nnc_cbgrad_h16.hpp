// nnc_cbgrad_h16.hpp -- the main loop of the dc MFMA kernels on bf16 / fp16 activations, written once: the
// 128 (i) x 128 (o) tile of dW = x^T g from two transposed LDS images.  All five kernels run it (k_cbdc_mfma, k_cbspdc_mfma,
// k_cbpkdc_mfma, k_cbdc_mfma_grouped, k_cbpkdc_mfma_grouped), so they hold the same accumulators and differ only in where the
// label of an accumulator comes from.  A kernel keeps its signature, its LDS carve-up, cbdc_begin and the epilogue; dcm_scales and
// dcm_accumulate are the rest.
#pragma once
#include "nnc_cbmfma.hpp"
#include "nnc_cbtile.hpp"

// the value of the 16 bits `h` as XT, scaled by 2^sc (bf16; fp16 is staged as it is: sc = 0), as the float32 hm_store_w rounds back
template <typename XT> __device__ __forceinline__ float dcm_staged(uint32_t h, int sc)
{
    const float v = (float)__builtin_bit_cast(XT, (unsigned short)h);
    return std::is_same<XT, bf16_t>::value ? ldexpf(v, sc) : v;
}

// 8 values of consecutive r into column `col` of an image [128][HM_LD] at r offset k0 (a multiple of 8): one 16-byte store
template <typename XT> __device__ __forceinline__ void dcm_store8(XT *img, int col, int k0, const float (&w)[8])
{
    typename HFrag<XT>::V v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (XT)w[j];
    *reinterpret_cast<typename HFrag<XT>::V *>(img + col * HM_LD + k0) = v;
}

// fp16 operands are staged unscaled: every product and sum is a normal float32 as it is, so the shift takes the two scales back
template <typename XT> __device__ __forceinline__ void dcm_scales(int &scx, int &scg, int &Sw)
{
    if (!std::is_same<XT, bf16_t>::value) {
        Sw += scx + scg;
        scx = scg = 0;
    }
}

// acc += the tile of dW' = (x 2^scx)^T (g 2^scg) over the rows [T.k_lo, T.k_hi) of the split, in steps of HM_BK: T.m0 is the first
// index row i, T.n0 the first column o.  xs [HM_BM][HM_LD] is the x^T image [i][r], gs [HM_BN][HM_LD] the g^T image [o][r].  Both
// operands arrive row-major in the wrong index, so both go through a transposing LDS store: the element arm owns column wc of both
// tiles and rows wk0 .. wk0 + 15, two values per word; XVEC (x and g 4-byte aligned, kdim and ncols even) columns 2 pc, 2 pc + 1
// and rows pk0 .. pk0 + 7, a word per row (the two columns).  Everything past kdim, ncols and k_hi is zero in the images, never
// memory.  The first barrier of the loop also orders what the caller wrote to LDS before it (the cleared bins).
template <typename XT, bool XVEC>
__device__ __forceinline__ void dcm_accumulate(const XT *x, const XT *g, long long kdim, long long ncols, const HmTile T, int scx,
                                               int scg, XT *xs, XT *gs, typename HFrag<XT>::C (&acc)[2][2])
{
    const unsigned short *x16 = reinterpret_cast<const unsigned short *>(x), *g16 = reinterpret_cast<const unsigned short *>(g);
    const int pc = T.t & 63, pk0 = (T.t >> 6) * 8;
    uint32_t xw[8], gw[8];

    auto load = [&](long long rb) {
        if constexpr (XVEC) {
            const long long ii = T.m0 + 2 * pc, oo = T.n0 + 2 * pc;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long r = rb + pk0 + j;
                xw[j] = (r < T.k_hi && ii < kdim) ? *reinterpret_cast<const uint32_t *>(x16 + r * kdim + ii) : 0u;
                gw[j] = (r < T.k_hi && oo < ncols) ? *reinterpret_cast<const uint32_t *>(g16 + r * ncols + oo) : 0u;
            }
        } else {
            const long long ii = T.m0 + T.wc, oo = T.n0 + T.wc;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long r = rb + T.wk0 + 2 * j;
                const uint32_t x0 = (r < T.k_hi && ii < kdim) ? x16[r * kdim + ii] : 0u, x1 = (r + 1 < T.k_hi && ii < kdim) ? x16[(r + 1) * kdim + ii] : 0u;
                const uint32_t g0 = (r < T.k_hi && oo < ncols) ? g16[r * ncols + oo] : 0u, g1 = (r + 1 < T.k_hi && oo < ncols) ? g16[(r + 1) * ncols + oo] : 0u;
                xw[j] = x0 | x1 << 16;
                gw[j] = g0 | g1 << 16;
            }
        }
    };
    auto store = [&]() {
        if constexpr (XVEC) {
            float a0[8], a1[8], b0[8], b1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a0[j] = dcm_staged<XT>(xw[j] & 0xFFFFu, scx), a1[j] = dcm_staged<XT>(xw[j] >> 16, scx);
                b0[j] = dcm_staged<XT>(gw[j] & 0xFFFFu, scg), b1[j] = dcm_staged<XT>(gw[j] >> 16, scg);
            }
            dcm_store8(xs, 2 * pc, pk0, a0);
            dcm_store8(xs, 2 * pc + 1, pk0, a1);
            dcm_store8(gs, 2 * pc, pk0, b0);
            dcm_store8(gs, 2 * pc + 1, pk0, b1);
        } else {
            float a[16], b[16];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a[2 * j] = dcm_staged<XT>(xw[j] & 0xFFFFu, scx), a[2 * j + 1] = dcm_staged<XT>(xw[j] >> 16, scx);
                b[2 * j] = dcm_staged<XT>(gw[j] & 0xFFFFu, scg), b[2 * j + 1] = dcm_staged<XT>(gw[j] >> 16, scg);
            }
            hm_store_w(xs, T.wc, T.wk0, a);
            hm_store_w(gs, T.wc, T.wk0, b);
        }
    };

    hm_clear<XT>(acc);
    load(T.k_lo);
    for (long long rb = T.k_lo; rb < T.k_hi; rb += HM_BK) {
        __syncthreads();   // the bins are cleared (first step); the images of the step before have been read
        store();
        __syncthreads();
        if (rb + HM_BK < T.k_hi) load(rb + HM_BK);
        hm_step(xs, gs, T.wm, T.wn, T.fr, T.fh, acc);
    }
}

// the two arms of a dc MFMA kernel's XVEC: x and g on 4-byte addresses, kdim and ncols even
static inline bool dcm_xvec(const void *x, const void *g, long long kdim, long long ncols)
{
    return reinterpret_cast<uintptr_t>(x) % 4 == 0 && reinterpret_cast<uintptr_t>(g) % 4 == 0 && kdim % 2 == 0 && ncols % 2 == 0;
}
