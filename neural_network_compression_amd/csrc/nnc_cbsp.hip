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
//   k_cbsp_stream  m <= 16: a wave owns one 64-column segment (a lane a column) over a range of rows.  The bitmap words and
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

#define SP_ROWS 64                // rows whose bitmap words one vector load brings to a wave
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

// ------------------------------------------------------------------ the plan (host)
struct SpPlan {
    int path;                     // NNC_CBMM_NONE / _STREAM / _TILED / _BIAS
    int mt;                       // stream: rows of x per launch (a power of two >= m)
    int entries, cshift;          // the LDS d table: entries x (1 << cshift) copies
    int rowsum;                   // NNC_CBSP_ROWSUM_*
    long long col_tiles, row_tiles, splits, rows_per_split, lds;
};

static SpPlan sp_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus)
{
    SpPlan p{};
    if (m == 0 || ncols == 0) return p;
    if (kdim == 0) {
        p.path = NNC_CBMM_BIAS;
        return p;
    }
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    long long s;
    if (m <= CB_SKINNY_M) {
        p.path = NNC_CBMM_STREAM;
        p.rowsum = NNC_CBSP_ROWSUM_FUSED;
        p.mt = cb_mt(m);
        p.col_tiles = cdiv(ncols, 64);
        p.row_tiles = 1;
        // four workgroups per CU; every wave keeps at least one batch of SP_ROWS rows; the partials (splits x m x ncols x 4 B)
        // stay within a quarter of the bitmap
        s = std::min({cdiv(4LL * cus, p.col_tiles), kdim / (CB_WAVES * SP_ROWS), kdim / (16 * m)});
        if (lb == 1) {
            p.entries = 256;
            p.cshift = __builtin_ctz(CB_U8_COPIES);
        } else {
            p.entries = k + 1;
            while ((1 << p.cshift) < CB_U8_COPIES && (long long)p.entries << (p.cshift + 1) <= CB_U16_WORDS) ++p.cshift;
        }
        p.lds = ((long long)p.entries << p.cshift) * 4 + (long long)p.mt * 65 * 4 + (long long)p.entries * 4;
    } else {
        p.path = NNC_CBMM_TILED;
        p.rowsum = NNC_CBSP_ROWSUM_PASS;
        p.col_tiles = cdiv(ncols, TB_N);
        p.row_tiles = cdiv(m, TB_M);
        s = std::min({cdiv(2LL * cus, p.col_tiles * p.row_tiles), kdim / (16 * TB_K), 16LL});
        p.entries = k + 1;
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + k + 1) * 4 + TB_K * TB_N;
    }
    s = std::max(1LL, s);
    p.rows_per_split = cdiv(kdim, s);
    p.splits = cdiv(kdim, p.rows_per_split);
    return p;
}

// the workspace: [partials: splits x m x ncols floats, when split][row sums: rsplits x m floats], 256-byte aligned parts
static long long sp_rsplits(const SpPlan &p)
{
    if (p.path == NNC_CBMM_TILED) return 1;
    return p.path == NNC_CBMM_STREAM && p.splits > 1 ? p.splits : 0;
}
static long long sp_part_bytes(const SpPlan &p, long long m, long long ncols)
{
    return p.splits > 1 ? (p.splits * m * ncols * 4 + 255) / 256 * 256 : 0;
}
static int64_t sp_ws_bytes(const SpPlan &p, long long m, long long ncols) { return sp_part_bytes(p, m, ncols) + sp_rsplits(p) * m * 4; }

// ------------------------------------------------------------------ device helpers
__device__ __forceinline__ float sp_epilogue(float acc, float cz, float rs, const float *__restrict__ bias, long long c, int relu)
{
    float v = cz != 0.0f ? cz * rs + acc : acc;
    if (bias) v += bias[c];
    if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
    return v;
}

// ------------------------------------------------------------------ skinny: m <= 16
// grid (segments, splits), CB_THREADS threads.  out: y (splits == 1) or the partials [split][m][ncols]; rs_out: the row-sum
// partials [split][m] (split only; written by the segment-0 workgroups).
template <typename LT, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbsp_stream(const float *__restrict__ x, int m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                            const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const LT *__restrict__ sym,
                                                            long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                            int z, int entries, int cshift, long long rows_per_split, const float *__restrict__ bias,
                                                            int relu, int direct, float *__restrict__ out, float *__restrict__ rs_out)
{
    constexpr int U = CB_UNROLL;
    extern __shared__ float smem[];
    float *tab = smem;
    float *red = smem + (entries << cshift);          // [MT][64] accumulators, then [MT] row sums
    float *stage = red + MT * 65;
    const float cz = sp_cz(centers, k, z);
    sp_fill(tab, stage, centers, k, cz, entries, cshift);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long seg = blockIdx.x;
    const long long col = seg * 64 + lane;
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    const long long per_wave = (s_hi - s_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(s_hi, s_lo + wave * per_wave), i1 = std::min(s_hi, i0 + per_wave);

    float acc[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) acc[r] = 0.0f;
    float rsa = 0.0f, rsb = 0.0f;                     // row sums: lane f holds those of x[f / U, . + f % U] (and f + 64)
    __syncthreads();

    for (long long ib = i0; ib < i1; ib += SP_ROWS) {
        // the words and counts of rows ib .. ib + 63, one row per lane (rows past i1: an empty word)
        const long long ir = ib + lane;
        uint64_t wl = 0;
        long long cl = 0;
        if (ir < i1) {
            const long long gi = ir * segs;
            wl = bitmap[gi + seg];
            cl = sp_count(lo[gi + seg], lo[gi], hi[ir]);
        }
        const uint32_t wlo = (uint32_t)wl, whi = (uint32_t)(wl >> 32), clo = (uint32_t)cl, chi = (uint32_t)((uint64_t)cl >> 32);
        const int nb = (int)std::min((long long)SP_ROWS, i1 - ib);
        for (int u0 = 0; u0 < nb; u0 += U) {
            const long long i = ib + u0;
            float xa, xb;
            {
                const int f0 = lane, f1 = lane + 64, r0 = f0 / U, r1 = f1 / U;
                xa = (r0 < m && i + f0 % U < i1) ? x[(long long)r0 * kdim + i + f0 % U] : 0.0f;
                xb = (MT * U > 64 && r1 < m && i + f1 % U < i1) ? x[(long long)r1 * kdim + i + f1 % U] : 0.0f;
            }
            uint32_t bits[U], sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {   // the symbol loads of U rows in flight together
                const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)whi, u0 + u) << 32) |
                                      (uint32_t)__builtin_amdgcn_readlane((int)wlo, u0 + u);
                const long long cnt = (long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)chi, u0 + u) << 32) |
                                                  (uint32_t)__builtin_amdgcn_readlane((int)clo, u0 + u));
                bits[u] = (uint32_t)(word >> lane) & 1u;
                const long long pos = cnt + sp_rank(word);
                sv[u] = 0;
                if (bits[u] && pos < nnz) sv[u] = sym[pos];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float wv = tab[CbTable<LT>::index(sv[u], k, cshift, lane)];
#pragma unroll
                for (int r = 0; r < MT; ++r) {
                    const int f = r * U + u;
                    const float xv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
                    if (bits[u]) acc[r] = __builtin_fmaf(xv, wv, acc[r]);
                }
            }
            rsa += xa;
            rsb += xb;
        }
    }
    // the wave's row sums, r's U lanes in lane order
    float rs[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) {
        float v = 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int f = r * U + u;
            v += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? rsa : rsb), f & 63));
        }
        rs[r] = v;
    }
    // the waves' sums, added to wave 0's in wave order
    for (int src = 1; src < CB_WAVES; ++src) {
        __syncthreads();
        if (wave == src) {
#pragma unroll
            for (int r = 0; r < MT; ++r) red[r * 64 + lane] = acc[r];
            if (lane == 0)
#pragma unroll
                for (int r = 0; r < MT; ++r) red[MT * 64 + r] = rs[r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < MT; ++r) {
                acc[r] += red[r * 64 + lane];
                rs[r] += red[MT * 64 + r];
            }
        }
    }
    if (wave != 0) return;
    if (!direct && seg == 0 && lane == 0)
        for (int r = 0; r < m && r < MT; ++r) rs_out[(long long)blockIdx.y * m + r] = rs[r];
    if (col >= ncols) return;
#pragma unroll
    for (int r = 0; r < MT; ++r) {
        if (r >= m) continue;
        if (direct) out[(long long)r * ncols + col] = sp_epilogue(acc[r], cz, rs[r], bias, col, relu);
        else out[((long long)blockIdx.y * m + r) * ncols + col] = acc[r];
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
__global__ __launch_bounds__(256) void k_cbsp_rowsum(const float *__restrict__ x, long long m, long long kdim, float *__restrict__ rs)
{
    __shared__ float part[256];
    for (long long r = blockIdx.x; r < m; r += gridDim.x) {
        float v = 0.0f;
        for (long long i = threadIdx.x; i < kdim; i += 256) v += x[r * kdim + i];
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

// ------------------------------------------------------------------ split-K combine
// the partials as k_cbmm_reduce sums them (four quarters of the splits in order, then the quarters in order); the row sum of r
// is the sum of its rsplits partials in split order.  part == NULL (kdim = 0): y = bias.
#define RED_Q 4
__global__ __launch_bounds__(256) void k_cbsp_reduce(const float *__restrict__ part, long long splits, long long m, long long ncols,
                                                     const float *__restrict__ rsp, long long rsplits, const float *__restrict__ centers, int k,
                                                     int z, const float *__restrict__ bias, int relu, float *__restrict__ y)
{
    __shared__ float qs[RED_Q - 1][64];
    const long long mn = m * ncols;
    const float cz = sp_cz(centers, k, z);
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long per_q = (splits + RED_Q - 1) / RED_Q;
    const long long s0 = std::min(splits, q * per_q), s1 = std::min(splits, s0 + per_q);
    for (long long base = (long long)blockIdx.x * 64; base < mn; base += (long long)gridDim.x * 64) {
        const long long idx = base + o;
        float v = 0.0f;
        if (idx < mn) {
#pragma unroll 8
            for (long long s = s0; s < s1; ++s) v += part[s * mn + idx];
        }
        __syncthreads();
        if (q > 0) qs[q - 1][o] = v;
        __syncthreads();
        if (q == 0 && idx < mn) {
#pragma unroll
            for (int j = 0; j < RED_Q - 1; ++j) v += qs[j][o];
            const long long r = idx / ncols;
            float rs = 0.0f;
            for (long long s = 0; s < rsplits; ++s) rs += rsp[s * m + r];
            y[idx] = sp_epilogue(v, cz, rs, bias, idx - r * ncols, relu);
        }
    }
}

// ------------------------------------------------------------------ C ABI
int cbsp_rowsum(const float *x, long long m, long long kdim, float *rs, hipStream_t s)
{
    hipLaunchKernelGGL(k_cbsp_rowsum, dim3((unsigned)std::min<long long>(m, 65536)), dim3(256), 0, s, x, m, kdim, rs);
    LAUNCHCHK("k_cbsp_rowsum");
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
    hipLaunchKernelGGL((k_cbsp_stream<LT, MT>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, reinterpret_cast<const uint64_t *>(base),
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
        hipLaunchKernelGGL(k_cbsp_reduce, dim3(rgrid), dim3(256), 0, s, (const float *)nullptr, 0LL, (long long)m, (long long)ncols, (const float *)nullptr,
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
        hipLaunchKernelGGL(k_cbsp_reduce, dim3(rgrid), dim3(256), 0, s, part, (long long)p.splits, (long long)m, (long long)ncols, rsp, sp_rsplits(p),
                           centers_dev, (int)k, (int)zero_symbol, bias_dev, (int)relu, y);
        LAUNCHCHK("k_cbsp_reduce");
    }
    return NNC_OK;
}
