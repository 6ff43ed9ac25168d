// nnc_cbmfma.hpp -- the 128 x 128 MFMA tile of the bf16 / fp16 codebook kernels at m > 16, written once.
// HM_THREADS threads, 4 waves, each a 64 x 64 quarter as 2 x 2 v_mfma_f32_32x32x16 accumulators; grid (column tiles * row tiles,
// splits).  Nine kernels run its k loop, hm_accumulate: four forward kernels (k_cbmm_mfma_grouped, k_cbpk_mfma_grouped, k_cbsp_mfma,
// k_cbspg_mfma) and the five dx kernels (k_cbdx_mfma, k_cbspdx_mfma, k_cbpkdx_mfma, k_cbdx_mfma_grouped, k_cbpkdx_mfma_grouped);
// k_cbmm_mfma keeps the same loop written out, because through the callables it compiled to a slower instruction stream (section
// 31).  The dc kernels run dcm_accumulate (nnc_cbgrad_h16.hpp) on the same fragments.  A
// kernel keeps its signature, its table (cb_fill; cb_refill on the walk through the groups, as the loop's `open`) and the load of
// its index form (a byte, two bytes, a packed field, the bitmap-sparse decode of nnc_cbsp.hpp), and takes the rest from here: the
// LDS carve-up, the tile coordinates, the x fragments, the two LDS images, the lookup into the W image, the barriers and the
// load-next-before-MFMA order of the k loop, the k step and the C / D epilogue.
#pragma once
#include "nnc_cbmm.hpp"

// the dynamic LDS of a forward kernel: the per-bank table (entries << cshift words), the stage cb_fill copies from (entries
// words), then the two images
template <typename XT> struct HmLds {
    float *cb, *stage;
    XT *xs, *ws;   // [HM_BM][HM_LD]: x tile, row-major in k; [HM_BN][HM_LD]: W tile, column-major (k contiguous)
};

template <typename XT> __device__ __forceinline__ HmLds<XT> hm_lds(float *smem, int entries, int cshift)
{
    HmLds<XT> L;
    L.cb = smem;
    L.stage = smem + (entries << cshift);
    L.xs = reinterpret_cast<XT *>(smem + hm_table_words(entries, cshift));
    L.ws = L.xs + HM_BM * HM_LD;
    return L;
}

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

// The W image of the step at kb from the thread's 16 labels: cb[index(lab[j])] for its rows kb + wk0 + j, and zero past k_hi and
// where the thread's column does not exist (col_ok false), never the table: a label there is no label, and a NaN centre would reach
// valid outputs as NaN * 0.  `index` is the kernel's table lookup (CbTable<LT>::index, or the packed form's fixed shift).
template <typename XT, typename Index>
__device__ __forceinline__ void hm_lookup_w(XT *ws, const float *cb, const HmTile &T, bool col_ok, long long kb, const uint32_t (&lab)[16], Index index)
{
    float w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = (col_ok && kb + T.wk0 + j < T.k_hi) ? cb[index(lab[j])] : 0.0f;
    hm_store_w(ws, T.wc, T.wk0, w);
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

// The k loop of the tile: acc = the 128 x 128 tile of x W over the k range [T.k_lo, T.k_hi) of the split, in steps of HM_BK.  x has
// m rows of length kdim and T.m0 is the tile's first; xs [HM_BM][HM_LD] is its image, row-major in k (hm_load_x / hm_store_x).
// ws [HM_BN][HM_LD] is the W image [column][k], which the kernel's callables fill: load_w(kb) fetches what the thread needs of its
// index form for the step at kb, one step ahead of the MFMAs that consume it, and store_w(kb) looks it up and writes the thread's 16
// values (hm_lookup_w, hm_store_w).  ahead(kb), behind the loads of x, is for a form that requests something for the step after
// kb there (the bitmap words of the sparse forms, which their kernels request for T.k_lo themselves in front of the call).
// open(kb) runs at the top of every step in front of its first barrier, when the lookups of the step before have ended (at that
// step's second barrier): the grouped kernels refill the table there when the step opens a group.  Whatever steers a callable
// must be uniform over the workgroup: every wave reaches both barriers of every step.  The first barrier also orders what the
// caller wrote to LDS before the call (the table).  A forward kernel passes (x, m, kdim); a dx kernel passes (g, m, ncols), its
// tile being dx = g W^T over the columns of the split, T.n0 its first index row and ws the W^T image [i][o].
struct HmNothing {
    __device__ __forceinline__ void operator()(long long) const {}
};

template <typename XT, bool XVEC, typename LoadW, typename StoreW, typename Ahead = HmNothing, typename Open = HmNothing>
__device__ __forceinline__ void hm_accumulate(const XT *x, long long m, long long kdim, const HmTile T, XT *xs, const XT *ws,
                                              typename HFrag<XT>::C (&acc)[2][2], LoadW load_w, StoreW store_w, Ahead ahead = Ahead(), Open open = Open())
{
    uint4 xf[2];
    auto load = [&](long long kb) {
        load_w(kb);
#pragma unroll
        for (int i = 0; i < 2; ++i) xf[i] = hm_load_x<XT, XVEC>(x, m, kdim, T.m0, kb, T.k_hi, T.t + i * HM_THREADS);
        ahead(kb);
    };

    hm_clear<XT>(acc);
    load(T.k_lo);
    for (long long kb = T.k_lo; kb < T.k_hi; kb += HM_BK) {
        open(kb);
        __syncthreads();   // the table is filled (first step, or refilled); the images of the step before have been read
        store_w(kb);
#pragma unroll
        for (int i = 0; i < 2; ++i) hm_store_x(xs, T.t + i * HM_THREADS, xf[i]);
        __syncthreads();
        if (kb + HM_BK < T.k_hi) load(kb + HM_BK);
        hm_step(xs, ws, T.wm, T.wn, T.fr, T.fh, acc);
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
