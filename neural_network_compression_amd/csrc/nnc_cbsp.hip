// nnc_cbsp.hip -- the pruned quantized layer run from a bitmap-sparse form of its centroid indices (include/nnc.h, nnc_cbsp_*;
// DESIGN.md section 11).
//
// The form of a (kdim, ncols) index matrix with a skipped symbol z, S = ceil(ncols / 64) segments per row, G = kdim * S, all in
// one buffer (nnc_cbsp_pack_bytes):
//   bitmap  uint64[G]      bit b of segment (i, s) set iff labels[i, 64 s + b] != z (bits past ncols are 0)
//   lo      uint32[G]      the low word of the exclusive prefix count of stored symbols at the start of the segment
//   hi      uint32[kdim]   the high word of that count at the start of row i
//   symbols 1 or 2 bytes   the labels != z in row-major order (256-byte aligned)
// The count at segment (i, s) is (hi[i] << 32 | lo[i, s]) + 2^32 if lo[i, s] < lo[i, 0] (the low word wrapped inside the row;
// a row holds fewer than 2^32 symbols since ncols < 2^32).  Structure: 96 bits per segment + 32 per row <= 2 bits per weight
// slot of the padded (kdim, 64 S) matrix.
//
// The product: y = c_z * sum_i x[r, i] + sum over stored (i, o) of x[r, i] * d[labels[i, o]] (+ bias, ReLU), d[s] = c[s] - c_z
// in float32, d[s >= K] = -c_z; with c_z == 0 exactly the rank-1 term is dropped, so a skipped weight is absent (Inf * 0 is not
// formed).  Kernels:
//   k_cbsp_bits / k_cbsp_rowscan / k_cbsp_basescan / k_cbsp_emit   the pack: ballot + popcount per segment, a scan of the
//                  counts in each row, a scan of the row totals, the symbols emitted at count + v_mbcnt.  No per-weight temporary.
//   k_cbsp_unpack  the inverse.
//   k_cbsp_stream  (nnc_cbsp.hpp, with the plan and k_cbsp_reduce: nnc_cbsp_h16.hip instantiates them for bf16 / fp16 x; here x is
//                  float32)  m <= 16: a wave owns one 64-column segment (a lane a column) over a range of rows.  The bitmap words and
//                  offsets of 64 rows come in one vector load per lane and are broadcast by v_readlane; a lane's symbol is at
//                  count + v_mbcnt(word); the d table sits in LDS with one copy per bank (CbTable); x[r, i] is broadcast by
//                  v_readlane; the symbol loads of CB_UNROLL rows are in flight together.  The row sums of x are kept on the
//                  side (one add per lane per CB_UNROLL rows) and combined in a fixed order.
//   k_cbsp_tiled   m > 16: the W tile decoded from bitmap and symbols into LDS, then the FMA step of k_cbmm_tiled; the tile
//                  coordinates and the x tile load are nnc_cbtile.hpp's, the kept mask, the masked step and the store its own.
//   k_cbsp_rowsum  m > 16: sum_i x[r, i], one workgroup per row, in a fixed order.
//   k_cbsp_reduce  the split-K partials in split order, + c_z * row sum, + bias, ReLU.  No float atomics anywhere.
#include "nnc_cbsp.hpp"
#include "nnc_cbtile.hpp"

#define SP_PLAN_LEN NNC_CBSP_PLAN_LEN

__device__ __forceinline__ uint32_t sp_label(const unsigned char *labels, int lb, long long idx)
{
    return lb == 1 ? (uint32_t)labels[idx] : (uint32_t)reinterpret_cast<const uint16_t *>(labels)[idx];
}

// ------------------------------------------------------------------ pack / unpack
// one wave per segment (grid-stride): bitmap word by ballot, its popcount into lo
__global__ __launch_bounds__(256) void k_cbsp_bits(const unsigned char *__restrict__ labels, int lb, long long ncols, long long segs, long long g,
                                                   uint32_t z, uint64_t *__restrict__ bitmap, uint32_t *__restrict__ lo)
{
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * 4;
    for (long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); seg < g; seg += waves) {
        const long long i = seg / segs, c = (seg - i * segs) * 64 + lane;
        const bool keep = c < ncols && sp_label(labels, lb, i * ncols + c) != z;
        const uint64_t word = __ballot(keep);
        if (lane == 0) {
            bitmap[seg] = word;
            lo[seg] = (uint32_t)__popcll(word);
        }
    }
}

// one workgroup per row: the exclusive scan of the row's segment counts in place, the row total into hi[i]
__global__ __launch_bounds__(256) void k_cbsp_rowscan(long long kdim, long long segs, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi)
{
    __shared__ uint32_t part[256];
    for (long long i = blockIdx.x; i < kdim; i += gridDim.x) {
        uint32_t *row = lo + i * segs;
        uint32_t carry = 0;
        for (long long s0 = 0; s0 < segs; s0 += 256) {
            const long long s = s0 + threadIdx.x;
            const uint32_t v = s < segs ? row[s] : 0u;
            part[threadIdx.x] = v;
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {   // Hillis-Steele inclusive scan
                const uint32_t t = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
                __syncthreads();
                part[threadIdx.x] += t;
                __syncthreads();
            }
            if (s < segs) row[s] = carry + part[threadIdx.x] - v;
            carry += part[255];
            __syncthreads();
        }
        if (threadIdx.x == 0) hi[i] = carry;
    }
}

// one workgroup: the exclusive scan of the row totals (int64); hi[i] = its high word, lo[i * segs] = its low word (the in-row
// count of segment 0 is 0); *nnz = the total
__global__ __launch_bounds__(256) void k_cbsp_basescan(long long kdim, long long segs, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi,
                                                       long long *__restrict__ nnz)
{
    __shared__ long long part[256];
    long long carry = 0;
    for (long long i0 = 0; i0 < kdim; i0 += 256) {
        const long long i = i0 + threadIdx.x;
        const long long v = i < kdim ? (long long)hi[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const long long t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < kdim) {
            const long long base = carry + part[threadIdx.x] - v;
            hi[i] = (uint32_t)((uint64_t)base >> 32);
            if (segs > 0) lo[i * segs] = (uint32_t)base;
        }
        carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0 && nnz) *nnz = carry;
}

// one wave per segment: lo[g] becomes the low word of the global count; the symbols go to count + rank (only below `cap`)
__global__ __launch_bounds__(256) void k_cbsp_emit(const unsigned char *__restrict__ labels, int lb, long long ncols, long long segs, long long g,
                                                   const uint64_t *__restrict__ bitmap, uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                   unsigned char *__restrict__ sym, long long cap)
{
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * 4;
    for (long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); seg < g; seg += waves) {
        const long long i = seg / segs, s = seg - i * segs, c = s * 64 + lane;
        const uint64_t word = bitmap[seg];
        const uint32_t lo0 = lo[i * segs];
        const long long base = (long long)(((uint64_t)hi[i] << 32) | lo0) + (s > 0 ? (long long)lo[seg] : 0LL);
        if (s > 0 && lane == 0) lo[seg] = (uint32_t)base;   // segment 0 already holds it (read above by every wave of the row)
        if ((word >> lane) & 1) {
            const long long pos = base + sp_rank(word);
            if (pos < cap) {
                const uint32_t v = sp_label(labels, lb, i * ncols + c);
                if (lb == 1) sym[pos] = (unsigned char)v;
                else reinterpret_cast<uint16_t *>(sym)[pos] = (uint16_t)v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_cbsp_unpack(const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                     const unsigned char *__restrict__ sym, long long nnz, int lb, long long ncols, long long segs,
                                                     long long g, uint32_t z, unsigned char *__restrict__ labels)
{
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * 4;
    for (long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); seg < g; seg += waves) {
        const long long i = seg / segs, c = (seg - i * segs) * 64 + lane;
        if (c >= ncols) continue;
        const uint64_t word = bitmap[seg];
        uint32_t v = z;
        if ((word >> lane) & 1) {
            const long long pos = sp_count(lo[seg], lo[i * segs], hi[i]) + sp_rank(word);
            v = pos < nnz ? sp_label(sym, lb, pos) : z;
        }
        if (lb == 1) labels[i * ncols + c] = (unsigned char)v;
        else reinterpret_cast<uint16_t *>(labels)[i * ncols + c] = (uint16_t)v;
    }
}

// ------------------------------------------------------------------ tiled: m > 16
// grid (col_tiles * row_tiles, splits), 256 threads, as k_cbmm_tiled; the W tile is decoded from bitmap and symbols: thread t
// decodes row t / 32 of the tile, columns (t % 32) * 4 .. + 3 (one segment, one word, one count + popcount).
template <typename LT>
__global__ __launch_bounds__(256) void k_cbsp_tiled(const float *__restrict__ x, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                    const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const LT *__restrict__ sym,
                                                    long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k, int z,
                                                    long long col_tiles, long long rows_per_split, const float *__restrict__ rowsum,
                                                    const float *__restrict__ bias, int relu, int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *tab = ws + TB_K * TB_N;         // k + 1 entries: d, then -c_z
    unsigned char *kept = reinterpret_cast<unsigned char *>(tab + k + 1);   // [TB_K][TB_N]: 1 where the weight is stored
    const float cz = sp_cz(centers, k, z);
    for (int j = threadIdx.x; j <= k; j += 256) tab[j] = (j < k ? centers[j] : 0.0f) - cz;

    const TbTile T = tb_tile(col_tiles, rows_per_split, kdim);
    float acc[8][8];
    tb_clear(acc);

    const int wk = threadIdx.x >> 5, wc = (threadIdx.x & 31) * 4;
    const long long gc = T.n0 + wc, gs = gc >> 6;
    const int b0 = (int)(gc & 63);
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        __syncthreads();
        const int nonfinite = tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t keep = 0;
        if (gk < T.hi && gc < ncols) {
            const long long gi = gk * segs;
            const uint64_t word = bitmap[gi + gs];
            long long pos = sp_count(lo[gi + gs], lo[gi], hi[gk]) + __popcll(word & ((1ULL << b0) - 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((word >> (b0 + j)) & 1) {
                    const uint32_t l = pos < nnz ? (uint32_t)sym[pos] : (uint32_t)k;
                    v[j] = tab[std::min(l, (uint32_t)k)];
                    keep |= 1u << j;
                    ++pos;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[wk * TB_N + wc + j] = v[j];
            kept[wk * TB_N + wc + j] = (unsigned char)((keep >> j) & 1);
        }
        // a skipped weight is absent: where the x tile holds an Inf or NaN the FMA must not form x * 0 at a skipped position
        // (rare, so the whole workgroup takes the masked step for that tile only)
        if (__syncthreads_or(nonfinite)) tb_tile_fma_masked(xs, ws, kept, T.tx, T.ty, acc);
        else tb_tile_fma(xs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const long long r = T.m0 + T.ty * 8 + a;
        if (r >= m) continue;
        const float rs = direct ? rowsum[r] : 0.0f;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const long long c = T.n0 + T.tx * 8 + b;
            if (c >= ncols) continue;
            if (direct) out[r * ncols + c] = sp_epilogue(acc[a][b], cz, rs, bias, c, relu);
            else out[((long long)blockIdx.y * m + r) * ncols + c] = acc[a][b];
        }
    }
}

// sum_i x[r, i]: one workgroup per row, each thread a strided sum, then a fixed tree
// (XT = bf16_t / f16_t, the g of nnc_cbsp_dx_h16: every element widened, the same float32 sums)
template <typename XT>
__global__ __launch_bounds__(256) void k_cbsp_rowsum(const XT *__restrict__ x, long long m, long long kdim, float *__restrict__ rs)
{
    __shared__ float part[256];
    for (long long r = blockIdx.x; r < m; r += gridDim.x) {
        float v = 0.0f;
        for (long long i = threadIdx.x; i < kdim; i += 256) v += (float)x[r * kdim + i];
        part[threadIdx.x] = v;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) rs[r] = part[0];
        __syncthreads();
    }
}

// ------------------------------------------------------------------ C ABI
int cbsp_rowsum_dt(const void *x, int dtype, long long m, long long kdim, float *rs, hipStream_t s)
{
    const dim3 grid((unsigned)std::min<long long>(m, 65536));
    if (dtype == NNC_DT_F32)
        hipLaunchKernelGGL(k_cbsp_rowsum<float>, grid, dim3(256), 0, s, reinterpret_cast<const float *>(x), m, kdim, rs);
    else if (dtype == NNC_DT_BF16)
        hipLaunchKernelGGL(k_cbsp_rowsum<bf16_t>, grid, dim3(256), 0, s, reinterpret_cast<const bf16_t *>(x), m, kdim, rs);
    else
        hipLaunchKernelGGL(k_cbsp_rowsum<f16_t>, grid, dim3(256), 0, s, reinterpret_cast<const f16_t *>(x), m, kdim, rs);
    LAUNCHCHK("k_cbsp_rowsum");
    return NNC_OK;
}

int cbsp_pack_scans(long long kdim, long long segs, uint32_t *lo, uint32_t *hi, long long *nnz, hipStream_t s)
{
    if (kdim > 0 && segs > 0) {
        hipLaunchKernelGGL(k_cbsp_rowscan, dim3((unsigned)std::min<long long>(kdim, 65536)), dim3(256), 0, s, kdim, segs, lo, hi);
        LAUNCHCHK("k_cbsp_rowscan");
    }
    if (kdim > 0 || nnz) {
        hipLaunchKernelGGL(k_cbsp_basescan, dim3(1), dim3(256), 0, s, kdim, segs, lo, hi, nnz);
        LAUNCHCHK("k_cbsp_basescan");
    }
    return NNC_OK;
}

static int sp_check_shape(const char *fn, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (kdim < 0 || ncols < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (label_bytes != 1 && label_bytes != 2) return fail(NNC_EINVAL, std::string(fn) + ": label_bytes must be 1 or 2");
    if (!sp_size_ok(kdim, ncols)) return fail(NNC_EINVAL, std::string(fn) + ": size too large (ncols < 2^32, kdim * ceil(ncols / 64) <= 2^40)");
    return NNC_OK;
}

extern "C" int64_t nnc_cbsp_pack_bytes(int64_t kdim, int64_t ncols, int label_bytes, int64_t nnz)
{
    if (kdim < 0 || ncols < 0 || (label_bytes != 1 && label_bytes != 2) || !sp_size_ok(kdim, ncols) || nnz < 0 || nnz > kdim * ncols)
        return 0;
    return sp_layout(kdim, ncols, label_bytes, nnz).bytes;
}

static int sp_grid(long long g) { return (int)std::max(1LL, std::min(cdiv(g, 4), 65536LL)); }

extern "C" int nnc_cbsp_pack(const void *labels, int label_bytes, int64_t kdim, int64_t ncols, int32_t zero_symbol, void *packed, int64_t packed_bytes,
                             int64_t *nnz_dev, void *stream)
{
    int rc = sp_check_shape("nnc_cbsp_pack", kdim, ncols, label_bytes);
    if (rc != NNC_OK) return rc;
    if ((rc = sp_check_z("nnc_cbsp_pack", zero_symbol, label_bytes)) != NNC_OK) return rc;
    const SpLayout L = sp_layout(kdim, ncols, label_bytes, 0);
    if (packed_bytes < L.bytes) return fail(NNC_ENOSPACE, "nnc_cbsp_pack: packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, label_bytes, 0)");
    if (!packed && L.bytes > 0) return fail(NNC_EINVAL, "nnc_cbsp_pack: packed is NULL");
    if (kdim > 0 && ncols > 0 && !labels) return fail(NNC_EINVAL, "nnc_cbsp_pack: labels is NULL");
    if (reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, "nnc_cbsp_pack: packed must be 256-byte aligned");
    if (label_bytes == 2 && reinterpret_cast<uintptr_t>(labels) % 2) return fail(NNC_EINVAL, "nnc_cbsp_pack: 2-byte labels must be 2-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned char *base = reinterpret_cast<unsigned char *>(packed);
    uint64_t *bitmap = reinterpret_cast<uint64_t *>(base);
    uint32_t *lo = reinterpret_cast<uint32_t *>(base + L.off_lo), *hi = reinterpret_cast<uint32_t *>(base + L.off_hi);
    const long long cap = (packed_bytes - L.off_sym) / label_bytes;
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (L.g > 0) {
        hipLaunchKernelGGL(k_cbsp_bits, dim3(sp_grid(L.g)), dim3(256), 0, s, lab, label_bytes, (long long)ncols, L.segs, L.g, (uint32_t)zero_symbol, bitmap, lo);
        LAUNCHCHK("k_cbsp_bits");
        hipLaunchKernelGGL(k_cbsp_rowscan, dim3((unsigned)std::min<long long>(kdim, 65536)), dim3(256), 0, s, (long long)kdim, L.segs, lo, hi);
        LAUNCHCHK("k_cbsp_rowscan");
    } else if (kdim > 0) {
        HIPCHK(hipMemsetAsync(hi, 0, (size_t)kdim * 4, s));   // ncols = 0: every row is empty
    }
    if (kdim > 0 || nnz_dev) {
        hipLaunchKernelGGL(k_cbsp_basescan, dim3(1), dim3(256), 0, s, (long long)kdim, L.segs, lo, hi, reinterpret_cast<long long *>(nnz_dev));
        LAUNCHCHK("k_cbsp_basescan");
    }
    if (L.g > 0) {
        hipLaunchKernelGGL(k_cbsp_emit, dim3(sp_grid(L.g)), dim3(256), 0, s, lab, label_bytes, (long long)ncols, L.segs, L.g, bitmap, lo, hi,
                           base + L.off_sym, cap);
        LAUNCHCHK("k_cbsp_emit");
    }
    return NNC_OK;
}

extern "C" int nnc_cbsp_unpack(const void *packed, int64_t packed_bytes, int label_bytes, int64_t kdim, int64_t ncols, int32_t zero_symbol, int64_t nnz,
                               void *labels_out, void *stream)
{
    int rc = sp_check_shape("nnc_cbsp_unpack", kdim, ncols, label_bytes);
    if (rc != NNC_OK) return rc;
    if ((rc = sp_check_z("nnc_cbsp_unpack", zero_symbol, label_bytes)) != NNC_OK) return rc;
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, "nnc_cbsp_unpack: nnz outside 0..kdim * ncols");
    const SpLayout L = sp_layout(kdim, ncols, label_bytes, nnz);
    if (packed_bytes < L.bytes) return fail(NNC_EINVAL, "nnc_cbsp_unpack: packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, label_bytes, nnz)");
    if (kdim == 0 || ncols == 0) return NNC_OK;
    if (!packed || !labels_out) return fail(NNC_EINVAL, "nnc_cbsp_unpack: packed or labels_out is NULL");
    if (reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, "nnc_cbsp_unpack: packed must be 256-byte aligned");
    if (label_bytes == 2 && reinterpret_cast<uintptr_t>(labels_out) % 2) return fail(NNC_EINVAL, "nnc_cbsp_unpack: 2-byte labels must be 2-byte aligned");
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    hipLaunchKernelGGL(k_cbsp_unpack, dim3(sp_grid(L.g)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint64_t *>(base),
                       reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi), base + L.off_sym,
                       (long long)nnz, label_bytes, (long long)ncols, L.segs, L.g, (uint32_t)zero_symbol, reinterpret_cast<unsigned char *>(labels_out));
    LAUNCHCHK("k_cbsp_unpack");
    return NNC_OK;
}

static int sp_check(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (m < 0) return fail(NNC_EINVAL, "nnc_cbsp_f32: negative size");
    int rc = sp_check_shape("nnc_cbsp_f32", kdim, ncols, label_bytes);
    if (rc != NNC_OK) return rc;
    if (k < 1 || k > NNC_KMAX) return fail(NNC_EINVAL, "nnc_cbsp_f32: k outside 1..NNC_KMAX");
    if (label_bytes == 1 && k > 256) return fail(NNC_EINVAL, "nnc_cbsp_f32: k > 256 needs 2-byte labels");
    if (m > (1LL << 40)) return fail(NNC_EINVAL, "nnc_cbsp_f32: size too large");
    return NNC_OK;
}

extern "C" int64_t nnc_cbsp_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || (label_bytes != 1 && label_bytes != 2) || m > (1LL << 40) || !sp_size_ok(kdim, ncols))
        return 0;
    return sp_ws_bytes(sp_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS), m, ncols);
}

template <typename LT, int MT>
static void launch_sp_stream(dim3 grid, size_t lds, hipStream_t s, const float *x, int m, long long kdim, const unsigned char *base, const SpLayout &L,
                             long long nnz, long long ncols, const float *centers, int k, int z, const SpPlan &p, const float *bias, int relu, int direct,
                             float *out, float *rs_out)
{
    hipLaunchKernelGGL((k_cbsp_stream<float, LT, MT>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, reinterpret_cast<const uint64_t *>(base),
                       reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi),
                       reinterpret_cast<const LT *>(base + L.off_sym), nnz, ncols, L.segs, centers, k, z, p.entries, p.cshift, p.rows_per_split, bias, relu,
                       direct, out, rs_out);
}

// every k_cbsp_stream instantiation there is; the plan is checked against this table, and the launch goes through it
using SpStreamLaunch = void (*)(dim3, size_t, hipStream_t, const float *, int, long long, const unsigned char *, const SpLayout &, long long, long long,
                                const float *, int, int, const SpPlan &, const float *, int, int, float *, float *);
struct SpStreamCase {
    int lb, mt;
    SpStreamLaunch fn;
};
static const SpStreamCase kSpStreamCases[] = {
    {1, 1, launch_sp_stream<uint8_t, 1>},   {1, 2, launch_sp_stream<uint8_t, 2>},   {1, 4, launch_sp_stream<uint8_t, 4>},
    {1, 8, launch_sp_stream<uint8_t, 8>},   {1, 16, launch_sp_stream<uint8_t, 16>}, {2, 1, launch_sp_stream<uint16_t, 1>},
    {2, 2, launch_sp_stream<uint16_t, 2>},  {2, 4, launch_sp_stream<uint16_t, 4>},  {2, 8, launch_sp_stream<uint16_t, 8>},
    {2, 16, launch_sp_stream<uint16_t, 16>},
};

static SpStreamLaunch find_sp_stream(int lb, int mt)
{
    for (const SpStreamCase &c : kSpStreamCases)
        if (c.lb == lb && c.mt == mt) return c.fn;
    return nullptr;
}

static int no_sp_stream_case(int lb, int mt)
{
    return fail(NNC_EINVAL, "nnc_cbsp: no k_cbsp_stream instantiation for label_bytes " + std::to_string(lb) + ", mt " + std::to_string(mt));
}

extern "C" int nnc_cbsp_plan(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out)
{
    const int rc = sp_check(m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbsp_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbsp_plan: out is NULL");
    const SpPlan p = sp_plan(m, kdim, ncols, label_bytes, k, cus);
    if (p.path == NNC_CBMM_STREAM && !find_sp_stream(label_bytes, p.mt)) return no_sp_stream_case(label_bytes, p.mt);
    const int64_t v[SP_PLAN_LEN] = {p.path, p.mt, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries, p.splits,
                                    p.rows_per_split, p.rowsum, p.lds, p.col_tiles, p.row_tiles, sp_ws_bytes(p, m, ncols)};
    for (int i = 0; i < SP_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbsp_f32(const float *x, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes, int64_t ncols,
                            int32_t zero_symbol, int64_t nnz, const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, float *y,
                            void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = sp_check(m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if ((rc = sp_check_z("nnc_cbsp_f32", zero_symbol, label_bytes)) != NNC_OK) return rc;
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, "nnc_cbsp_f32: nnz outside 0..kdim * ncols");
    const SpLayout L = sp_layout(kdim, ncols, label_bytes, nnz);
    if (packed_bytes < L.bytes) return fail(NNC_EINVAL, "nnc_cbsp_f32: packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, label_bytes, nnz)");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbsp_f32: centers is NULL");
    if (m > 0 && ncols > 0 && !y) return fail(NNC_EINVAL, "nnc_cbsp_f32: y is NULL");
    if (m > 0 && ncols > 0 && kdim > 0 && (!x || !packed)) return fail(NNC_EINVAL, "nnc_cbsp_f32: x or packed is NULL");
    if (m > 0 && ncols > 0 && kdim > 0 && reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, "nnc_cbsp_f32: packed must be 256-byte aligned");
    const int64_t need = nnc_cbsp_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace("nnc_cbsp_f32", "nnc_cbsp_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    if (m > 0 && ncols > 0 && kdim > 0 && reinterpret_cast<uintptr_t>(workspace) % 4) return fail(NNC_EINVAL, "nnc_cbsp_f32: workspace must be 4-byte aligned");
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const int rgrid = (int)std::max(1LL, std::min(cdiv(mn, 64), 8192LL));
    const SpPlan p = sp_plan(m, kdim, ncols, label_bytes, k, cu_count());
    if (p.path == NNC_CBMM_BIAS) {   // kdim = 0: y = bias (zeros without one)
        hipLaunchKernelGGL((k_cbsp_reduce<float, float>), dim3(rgrid), dim3(256), 0, s, (const float *)nullptr, 0LL, (long long)m, (long long)ncols, (const float *)nullptr,
                           0LL, centers_dev, (int)k, (int)zero_symbol, bias_dev, (int)relu, y);
        LAUNCHCHK("k_cbsp_reduce");
        return NNC_OK;
    }
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    const int direct = p.splits == 1;
    float *part = reinterpret_cast<float *>(workspace);
    float *rsp = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sp_part_bytes(p, m, ncols));
    float *out = direct ? y : part;
    if (p.path == NNC_CBMM_STREAM) {
        const SpStreamLaunch fn = find_sp_stream(label_bytes, p.mt);
        if (!fn) return no_sp_stream_case(label_bytes, p.mt);
        fn(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, base, L, nnz, ncols, centers_dev, k, zero_symbol, p,
           bias_dev, relu, direct, out, direct ? nullptr : rsp);
        LAUNCHCHK("k_cbsp_stream");
    } else {
        if ((rc = cbsp_rowsum(x, m, kdim, rsp, s)) != NNC_OK) return rc;
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        const uint64_t *bm = reinterpret_cast<const uint64_t *>(base);
        const uint32_t *lo = reinterpret_cast<const uint32_t *>(base + L.off_lo), *hi = reinterpret_cast<const uint32_t *>(base + L.off_hi);
        if (label_bytes == 1)
            hipLaunchKernelGGL(k_cbsp_tiled<uint8_t>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, bm, lo, hi,
                               reinterpret_cast<const uint8_t *>(base + L.off_sym), (long long)nnz, (long long)ncols, L.segs, centers_dev, (int)k,
                               (int)zero_symbol, p.col_tiles, p.rows_per_split, rsp, bias_dev, (int)relu, direct, out);
        else
            hipLaunchKernelGGL(k_cbsp_tiled<uint16_t>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, bm, lo, hi,
                               reinterpret_cast<const uint16_t *>(base + L.off_sym), (long long)nnz, (long long)ncols, L.segs, centers_dev, (int)k,
                               (int)zero_symbol, p.col_tiles, p.rows_per_split, rsp, bias_dev, (int)relu, direct, out);
        LAUNCHCHK("k_cbsp_tiled");
    }
    if (!direct) {
        hipLaunchKernelGGL((k_cbsp_reduce<float, float>), dim3(rgrid), dim3(256), 0, s, part, (long long)p.splits, (long long)m, (long long)ncols, rsp, sp_rsplits(p),
                           centers_dev, (int)k, (int)zero_symbol, bias_dev, (int)relu, y);
        LAUNCHCHK("k_cbsp_reduce");
    }
    return NNC_OK;
}
