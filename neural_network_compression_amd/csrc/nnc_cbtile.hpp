// nnc_cbtile.hpp -- what every tiled (m > 16) float32 codebook kernel repeats, written once: the byte form (k_cbmm_tiled,
// k_cbdx_tiled, k_cbdc_tiled), the packed form (k_cbpk_tiled, k_cbpkdx_tiled, k_cbpkdc_tiled), the bitmap-sparse form
// (k_cbsp_tiled, k_cbspdx_tiled, k_cbspdc_tiled), the group-wise forward pass (k_cbmm_tiled_grouped) and the group-wise backward
// passes (k_cbdx_tiled_grouped, k_cbdc_tiled_grouped; k_cbpkdx_tiled_grouped, k_cbpkdc_tiled_grouped).  A kernel keeps its
// LDS layout, its table and the decode of its W tile (where a weight's label comes from) and calls these for the rest: the
// tile coordinates, the x / g tile loads, the dc prologue and scaled tile fill, the stores and the dc binning loop.  The FMA
// step itself is tb_tile_fma (nnc_cbmm.hpp).  256 threads; grid (column tiles * row tiles, splits).  The sparse kernels keep
// their kept mask, the masked FMA step, the sp_epilogue store and the binning of k_cbspdc_tiled (a running symbol position and
// a register for the skipped weights: more than a label per (i, o)).  What the stream (m <= 16) kernels share is elsewhere: the
// label row loads, the forward x load and the group step in nnc_cbmm.hpp, the dc x load in nnc_cbgrad.hpp.
// cbdc_begin stays the tiled kernels' alone: the dc stream kernels compile to other instructions around it (same section).
#pragma once
#include "nnc_cbgrad.hpp"

// thread (tx, ty) = (t % 16, t / 16) owns rows ty*8.. and columns tx*8.. of the 128 x 128 tile at (m0, n0); the workgroup's
// split is [lo, hi) of the reduced dimension
struct TbTile {
    int tx, ty;
    long long n0, m0, lo, hi;
};

__device__ __forceinline__ TbTile tb_tile(long long col_tiles, long long per_split, long long extent)
{
    TbTile T;
    T.tx = threadIdx.x & 15;
    T.ty = threadIdx.x >> 4;
    T.n0 = (blockIdx.x % col_tiles) * TB_N;
    T.m0 = (blockIdx.x / col_tiles) * TB_M;
    T.lo = (long long)blockIdx.y * per_split;
    T.hi = std::min(extent, T.lo + per_split);
    return T;
}

__device__ __forceinline__ void tb_clear(float (&acc)[8][8])
{
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.0f;
}

// The x tile of the forward pass and the g tile of dx: a[m0 + r, kb + j] of a row-major a[m][stride] into as[j][r], r < TB_M,
// j < TB_K, 0 past m or `hi`.  Thread t loads row t / 2, columns (t % 2) * 4 .. + 3.  Returns non-zero if one of the thread's
// values is Inf or NaN (the sparse kernels take their masked step then; the others drop it).
__device__ __forceinline__ int tb_load_rows(float *as, const float *a, long long m, long long stride, long long m0, long long kb, long long hi)
{
    const int lr = threadIdx.x >> 1, lk = (threadIdx.x & 1) * 4;
    const long long gr = m0 + lr;
    int nonfinite = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long gk = kb + lk + j;
        const float v = (gr < m && gk < hi) ? a[gr * stride + gk] : 0.0f;
        nonfinite |= !__builtin_isfinite(v);
        as[(lk + j) * TB_M + lr] = v;
    }
    return nonfinite;
}

// The forward store of one output: y[r, c] = v + bias, then ReLU (direct), or the partial of this split at [blockIdx.y][r][c].
// The loop over a thread's 8 x 8 outputs stays in the kernels: compiled inside a helper, the 64 stores come out as another
// instruction sequence whose registers change the budget of the FMA loop (k_cbmm_tiled 96 -> 118 VGPRs, k_cbmm_tiled_grouped
// 122 -> 182 and half the occupancy; k_cbdx_tiled<uint16_t> 98 -> 110 with the dx store).
__device__ __forceinline__ void tb_store_y(float v, long long r, long long c, long long m, long long ncols, const float *bias, int relu, int direct, float *out)
{
    if (r >= m || c >= ncols) return;
    if (direct) {
        if (bias) v += bias[c];
        if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
        out[r * ncols + c] = v;
    } else {
        out[((long long)blockIdx.y * m + r) * ncols + c] = v;
    }
}

// the dx store of one output: dx[r, c] (direct) or the partial of this split at [blockIdx.y][r][c]; the loop stays in the kernels too
__device__ __forceinline__ void tb_store_dx(float v, long long r, long long c, long long m, long long kdim, int direct, float *out)
{
    float *dst = direct ? out : out + (long long)blockIdx.y * m * kdim;
    if (r < m && c < kdim) dst[r * kdim + c] = v;
}

// The head of a dc kernel: S and the flag from the maxima in hdr[0..1], written to hdr[2..3] by one thread of the launch; false
// (uniform over the launch) when there is nothing to bin.  Else the scales of x and g, the shift Sw of dW' = dW * 2^(scx + scg)
// and the workgroup's `nbins` LDS bins cleared (the caller's first barrier comes before any of them is used).
__device__ __forceinline__ bool cbdc_begin(uint32_t *hdr, long long m, int terms_log2, unsigned long long *bins, int nbins, int &scx, int &scg,
                                           int &Sw)
{
    int flag;
    const int S = cbdc_shift(hdr, m, terms_log2, flag);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        hdr[2] = (uint32_t)S;
        hdr[3] = (uint32_t)flag;
    }
    if (flag != CBG_FLAG_OK) return false;
    cbdc_scales(hdr, scx, scg);
    Sw = S - scx - scg;
    for (int j = threadIdx.x; j < nbins; j += 256) bins[j] = 0ull;
    return true;
}

// The two tiles of a dc step: x[rb + r, i0 + i] * 2^scx into xs[r][i] and g[rb + r, o0 + o] * 2^scg into gs[r][o], r < TB_K,
// +-0 past r_hi, kdim or ncols.  Thread t loads row t / 32, columns (t % 32) * 4 .. + 3 of both (coalesced).  All eight loads,
// then the sched_barrier, then the scaling: see cbdc_scaled (nnc_cbgrad.hpp).
__device__ __forceinline__ void cbdc_load_tiles(float *xs, float *gs, const float *x, const float *g, long long kdim, long long ncols,
                                                long long i0, long long o0, long long rb, long long r_hi, int scx, int scg)
{
    const int lk = threadIdx.x >> 5, lc = (threadIdx.x & 31) * 4;
    const long long r = rb + lk;
    const bool in_r = r < r_hi;
    float xv[4], gv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long ii = i0 + lc + j, oo = o0 + lc + j;
        xv[j] = x[cbdc_idx(r * kdim + ii, in_r && ii < kdim)];
        gv[j] = g[cbdc_idx(r * ncols + oo, in_r && oo < ncols)];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long ii = i0 + lc + j, oo = o0 + lc + j;
        xs[lk * TB_M + lc + j] = cbdc_scaled(xv[j], in_r && ii < kdim, scx);
        gs[lk * TB_N + lc + j] = cbdc_scaled(gv[j], in_r && oo < ncols, scg);
    }
}

// The thread's 64 values of dW' binned: the image of acc[a][b] into copy `rep` of bin label(i, o), i = m0 + ty*8 + a < kdim,
// o = n0 + tx*8 + b < ncols; a label >= k falls into no bin.  A row's 8 columns are asked for in order behind one guard, so a
// label() that reads them from one word (the packed form) loads it once.
template <typename Label>
__device__ __forceinline__ void cbdc_bin_tile(const float (&acc)[8][8], const TbTile &T, long long kdim, long long ncols, int k, int Sw,
                                              unsigned long long *bins, int rlog2, int rep, Label label)
{
    const long long o0 = T.n0 + T.tx * 8;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const long long i = T.m0 + T.ty * 8 + a;
        if (i >= kdim || o0 >= ncols) continue;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (o0 + b >= ncols) continue;
            const uint32_t l = label(i, o0 + b);
            if (l < (uint32_t)k) atomicAdd(&bins[(l << rlog2) + rep], cbdc_fix(acc[a][b], Sw));
        }
    }
}
