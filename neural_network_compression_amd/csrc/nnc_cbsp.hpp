// nnc_cbsp.hpp -- what the bitmap-sparse codebook matmul (nnc_cbsp.hip) shares with its backward pass (nnc_cbspgrad.hip): the
// layout and the limits of the packed form, the count and rank of a stored symbol, the d table, the masked FMA step of the tiled
// kernels and the row-sum launch.
#pragma once
#include "nnc_cbmm.hpp"

// ------------------------------------------------------------------ the layout (host and device)
struct SpLayout {
    long long segs, g;            // segments per row, kdim * segs
    long long off_lo, off_hi, off_sym, bytes;
};

static SpLayout sp_layout(long long kdim, long long ncols, int lb, long long nnz)
{
    SpLayout L{};
    L.segs = cdiv(ncols, 64);
    L.g = kdim * L.segs;
    L.off_lo = 8 * L.g;
    L.off_hi = L.off_lo + 4 * L.g;
    L.off_sym = (L.off_hi + 4 * kdim + 255) / 256 * 256;
    L.bytes = L.off_sym + nnz * lb;
    return L;
}

static bool sp_size_ok(int64_t kdim, int64_t ncols)
{
    return kdim <= (1LL << 40) && ncols < (1LL << 32) && (ncols == 0 || kdim <= (1LL << 40) / cdiv(ncols, 64));
}

static int sp_check_z(const char *fn, int32_t z, int label_bytes)
{
    if (z < 0 || z >= (label_bytes == 1 ? 256 : 65536)) return fail(NNC_EINVAL, std::string(fn) + ": zero_symbol outside the label range");
    return NNC_OK;
}

// the exclusive count of stored symbols at segment g of row i (lo0 = lo[i * segs], h = hi[i])
__device__ __forceinline__ long long sp_count(uint32_t lo, uint32_t lo0, uint32_t h)
{
    return (long long)(((uint64_t)h << 32) | lo) + (lo < lo0 ? (1LL << 32) : 0LL);
}

// bits of `word` below this lane (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ uint32_t sp_rank(uint64_t word)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(word >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)word, 0u));
}

// ------------------------------------------------------------------ the d table
// stage[j] = c[j] - c_z (j < k), -c_z past k; then `1 << cshift` copies of each entry as in k_cbmm_stream
__device__ __forceinline__ float sp_cz(const float *__restrict__ centers, int k, int z) { return z < k ? centers[z] : 0.0f; }

__device__ __forceinline__ void sp_fill(float *tab, float *stage, const float *__restrict__ centers, int k, float cz, int entries, int cshift)
{
    for (int j = threadIdx.x; j < entries; j += blockDim.x) stage[j] = (j < k ? centers[j] : 0.0f) - cz;
    __syncthreads();
    const int words = entries << cshift;
#pragma unroll 8
    for (int w = threadIdx.x; w < words; w += blockDim.x) tab[w] = stage[w >> cshift];
}

// tb_tile_fma with the products of skipped weights (kept[kk][n] == 0) left out
__device__ __forceinline__ void tb_tile_fma_masked(const float *xs, const float *ws, const unsigned char *kept, int tx, int ty, float (&acc)[8][8])
{
    for (int kk = 0; kk < TB_K; ++kk) {
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const float av = xs[kk * TB_M + ty * 8 + a];
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (kept[kk * TB_N + tx * 8 + b]) acc[a][b] = __builtin_fmaf(av, ws[kk * TB_N + tx * 8 + b], acc[a][b]);
        }
    }
}

// rs[r] = sum_i x[r, i] for r < m in a fixed order (k_cbsp_rowsum, nnc_cbsp.hip), launched on `s`: NNC_OK or the launch error
int cbsp_rowsum(const float *x, long long m, long long kdim, float *rs, hipStream_t s);
