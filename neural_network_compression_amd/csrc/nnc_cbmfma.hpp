// nnc_cbmfma.hpp -- the 128 x 128 MFMA tile of the bf16 / fp16 codebook kernels at m > 16, written once: k_cbmm_mfma
// (nnc_cbmm_h16.hip), k_cbmm_mfma_grouped (nnc_cbmm_grouped.hip) and k_cbpk_mfma_grouped (nnc_cbpk_grouped.hip).  HM_THREADS
// threads, 4 waves, each a 64 x 64 quarter as 2 x 2 v_mfma_f32_32x32x16 accumulators; grid (column tiles * row tiles, splits).  A
// kernel keeps its signature, its LDS carve-up, its table (cb_fill, and cb_refill on the walk through the groups), its label load
// (a byte, two bytes, a packed field) and its table lookup, and calls these for the rest: the tile coordinates, the x fragments,
// the two LDS images, the k step and the C / D epilogue.  The barriers, the load-next-before-MFMA order and the loop over the
// k steps stay in these forward kernels, as the decode of the tiled float32 kernels does around nnc_cbtile.hpp; the backward kernels
// on the same tile share theirs (dxm_accumulate of nnc_cbdxm.hpp, dcm_accumulate of nnc_cbgrad_h16.hpp).
#pragma once
#include "nnc_cbmm.hpp"

// Thread t of the tile at (m0, n0), split [k_lo, k_hi).  W image: t owns column wc and the 16 rows wk0 .. wk0 + 15 of a k step.
// MFMA: lane l of a 32x32x16 holds A[row l & 31][k = 8 (l >> 5) + e] and B[k = 8 (l >> 5) + e][col l & 31], e = 0..7, so the
// wave's quarter starts at (wm, wn) and the lane reads row / column fr at k offset fh.
struct HmTile {
    int t, lane, wc, wk0, wm, wn, fr, fh;
    long long n0, m0, k_lo, k_hi;
};

__device__ __forceinline__ HmTile hm_tile(long long col_tiles, long long rows_per_split, long long kdim)
{
    HmTile T;
    T.t = threadIdx.x;
    T.lane = T.t & 63;
    const int wave = T.t >> 6;
    T.n0 = (blockIdx.x % col_tiles) * HM_BN;
    T.m0 = (blockIdx.x / col_tiles) * HM_BM;
    T.k_lo = (long long)blockIdx.y * rows_per_split;
    T.k_hi = std::min(kdim, T.k_lo + rows_per_split);
    T.wc = T.t & (HM_BN - 1);
    T.wk0 = (T.t >> 7) * 16;
    T.wm = (wave >> 1) * 64;
    T.wn = (wave & 1) * 64;
    T.fr = T.lane & 31;
    T.fh = (T.lane >> 5) * 8;
    return T;
}

// C / D: register r of lane l of a 32 x 32 accumulator is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31, and accumulator
// (a, b) of a wave starts at (wm + 32 a, wn + 32 b).  The row and the column of the matrix, from those of the wave's quarter
// (row0 = m0 + wm, col0 = n0 + wn):
__device__ __forceinline__ long long hm_acc_row(long long row0, int a, int r, int lane) { return row0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ long long hm_acc_col(long long col0, int b, int lane) { return col0 + b * 32 + (lane & 31); }

// Fragment f (of the 128 rows x 4 fragments of 8; a thread loads f = t and t + HM_THREADS) of the x image of the step at kb: x[m0 +
// f / 4, kb + 8 (f % 4) .. + 7], zero past m and past k_hi, never memory: a NaN there would reach valid outputs as NaN * 0.  XVEC:
// x is 16-byte aligned and kdim a multiple of 8 (one 16-byte load); else element by element.
template <typename XT, bool XVEC>
__device__ __forceinline__ uint4 hm_load_x(const XT *__restrict__ x, long long m, long long kdim, long long m0, long long kb, long long k_hi, int f)
{
    const long long gr = m0 + (f >> 2), gk = kb + (f & 3) * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (gr < m) {
        if constexpr (XVEC) {   // kdim, k_lo and gk are multiples of 8: the fragment lies wholly before k_hi or wholly past it
            if (gk < k_hi) v = *reinterpret_cast<const uint4 *>(x + gr * kdim + gk);
        } else {
            const unsigned short *xr = reinterpret_cast<const unsigned short *>(x + gr * kdim);
            uint32_t h[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = gk + e < k_hi ? (uint32_t)xr[gk + e] : 0u;
            v = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
        }
    }
    return v;
}

// fragment f into the x image xs[HM_BM][HM_LD] (row-major in k)
template <typename XT> __device__ __forceinline__ void hm_store_x(XT *xs, int f, uint4 v)
{
    *reinterpret_cast<uint4 *>(xs + (f >> 2) * HM_LD + (f & 3) * 8) = v;
}

// the thread's 16 looked-up values (exact in XT: the table holds values of XT) into the W image ws[HM_BN][HM_LD] (column-major, k
// contiguous) as two 16-byte runs of k
template <typename XT> __device__ __forceinline__ void hm_store_w(XT *ws, int wc, int wk0, const float (&w)[16])
{
    typename HFrag<XT>::V w0, w1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        w0[j] = (XT)w[j];
        w1[j] = (XT)w[j + 8];
    }
    *reinterpret_cast<typename HFrag<XT>::V *>(ws + wc * HM_LD + wk0) = w0;
    *reinterpret_cast<typename HFrag<XT>::V *>(ws + wc * HM_LD + wk0 + 8) = w1;
}

template <typename XT> __device__ __forceinline__ void hm_clear(typename HFrag<XT>::C (&acc)[2][2])
{
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
}

// one k step of HM_BK from the two images: two sub-steps of 16, each 2 x 2 MFMAs, acc[i][j] += A_i B_j
template <typename XT>
__device__ __forceinline__ void hm_step(const XT *xs, const XT *ws, int wm, int wn, int fr, int fh, typename HFrag<XT>::C (&acc)[2][2])
{
    using F = HFrag<XT>;
    using V = typename F::V;
#pragma unroll
    for (int s = 0; s < HM_BK; s += 16) {
        V a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = *reinterpret_cast<const V *>(xs + (wm + i * 32 + fr) * HM_LD + s + fh);
            b[i] = *reinterpret_cast<const V *>(ws + (wn + i * 32 + fr) * HM_LD + s + fh);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = F::mfma(a[i], b[j], acc[i][j]);
    }
}

// C / D (hm_acc_row, hm_acc_col).  `out` is y (direct 1: float32, 2: XT; + bias, ReLU here) or the float32 partials
// [split][m][ncols] (direct 0).
template <typename XT>
__device__ __forceinline__ void hm_store_y(const typename HFrag<XT>::C (&acc)[2][2], long long n0, long long m0, int wm, int wn, int lane, long long m,
                                           long long ncols, const float *__restrict__ bias, int relu, int direct, void *__restrict__ out_)
{
    float *outf = reinterpret_cast<float *>(out_);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long c = hm_acc_col(n0 + wn, j, lane);
            if (c >= ncols) continue;
            const float bv = (direct && bias) ? bias[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long row = hm_acc_row(m0 + wm, i, r, lane);
                if (row >= m) continue;
                float v = acc[i][j][r];
                if (direct) {
                    if (bias) v += bv;
                    if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
                    if (direct == 2)
                        reinterpret_cast<XT *>(out_)[row * ncols + c] = (XT)v;
                    else
                        outf[row * ncols + c] = v;
                } else {
                    outf[((long long)blockIdx.y * m + row) * ncols + c] = v;
                }
            }
        }
    }
}

// the launch of a kernel instantiated for both arms of XVEC (x 16-byte aligned and kdim a multiple of 8, or not): HM_THREADS threads
template <typename... P, typename... A>
static inline void hm_launch(const void *x, long long kdim, void (*vec)(P...), void (*elem)(P...), dim3 grid, size_t lds, hipStream_t s, A... args)
{
    const bool xvec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && kdim % 8 == 0;
    hipLaunchKernelGGL(xvec ? vec : elem, grid, dim3(HM_THREADS), lds, s, args...);
}
