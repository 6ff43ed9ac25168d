// nnc_cbsp.hpp -- what the bitmap-sparse codebook matmul (nnc_cbsp.hip) shares with its backward pass (nnc_cbspgrad.hip): the
// layout and the limits of the packed form, the count and rank of a stored symbol, the d table, the masked FMA step of the tiled
// kernels and the row-sum launch.  The plan (sp_plan), the stream kernel k_cbsp_stream and the split-K combine k_cbsp_reduce live
// here too, templated on the type of x: nnc_cbsp.hip instantiates them for float32, nnc_cbsp_h16.hip for bf16 / fp16 activations.
// SpTileDecode is the decode of the two forward MFMA kernels on half x (nnc_cbsp_h16.hip, nnc_cbsp_grouped_h16.hip).
#pragma once
#include "nnc_cbmfma.hpp"

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

// ------------------------------------------------------------------ the decode of the MFMA tile (bf16 / fp16 x, m > 16)
// What k_cbsp_mfma (nnc_cbsp_h16.hip) and k_cbspg_mfma (nnc_cbsp_grouped_h16.hip) put in front of the tile of nnc_cbmfma.hpp: the
// labels of a thread's 16 k rows of its column, from the form.  A wave's 64 lanes own one 64-column segment (n0 is a multiple of
// 128, wc = t & 127) and the same 16 rows of a step (wk0 = 16 (t >> 7)), so the bitmap word and the count of a row are uniform over
// the wave: load_words(kb) has lane j < 16 load those of row kb + wk0 + j, decode() broadcasts them by v_readlane, and a lane's symbol
// sits at count + v_mbcnt(word).  The kernels call load_words two k steps ahead of the MFMAs and decode one (hm_accumulate's `ahead`
// and `load_w`).  No load leaves the packed buffer: rows past k_hi load no word and segments past segs nothing, so their words are
// empty, and a symbol is loaded only where its bit is set and pos < nnz.  No readlane sits inside a lane-dependent branch.
template <typename LT> struct SpTileDecode {
    const uint64_t *__restrict__ bitmap;
    const uint32_t *__restrict__ lo, *__restrict__ hi;
    const LT *__restrict__ sym;
    long long nnz, segs, seg, k_hi;   // seg: the wave's segment
    int wk0, lane;                    // wk0: the wave's first k row of a step
    bool seg_ok;
    uint32_t wlo = 0, whi = 0, clo = 0, chi = 0;   // lane j < 16: the word and the count of row kb + wk0 + j

    __device__ __forceinline__ SpTileDecode(const uint64_t *bitmap_, const uint32_t *lo_, const uint32_t *hi_, const LT *sym_, long long nnz_, long long segs_,
                                            const HmTile &T)
        : bitmap(bitmap_), lo(lo_), hi(hi_), sym(sym_), nnz(nnz_), segs(segs_), seg((T.n0 >> 6) + __builtin_amdgcn_readfirstlane(T.wc >> 6)), k_hi(T.k_hi),
          wk0(__builtin_amdgcn_readfirstlane(T.wk0)), lane(T.lane), seg_ok(seg < segs_)
    {
    }

    __device__ __forceinline__ void load_words(long long kb)
    {
        const long long gk = kb + wk0 + lane;
        uint64_t w = 0;
        long long c = 0;
        if (lane < 16 && seg_ok && gk < k_hi) {         // rows past k_hi and segments past segs load nothing
            const long long gi = gk * segs;
            w = bitmap[gi + seg];
            c = sp_count(lo[gi + seg], lo[gi], hi[gk]);
        }
        wlo = (uint32_t)w, whi = (uint32_t)(w >> 32), clo = (uint32_t)c, chi = (uint32_t)((uint64_t)c >> 32);
    }

    // from the words the last load_words brought; z (uniform over the wave) is the label of a skipped position
    __device__ __forceinline__ void decode(uint32_t z, uint32_t (&lab)[16]) const
    {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)whi, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)wlo, j);
            const long long cnt = (long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)chi, j) << 32) |
                                              (uint32_t)__builtin_amdgcn_readlane((int)clo, j));
            const long long pos = cnt + sp_rank(word);
            lab[j] = z;                                 // a skipped position (every position of an empty word: past k_hi, past segs)
            if (((word >> lane) & 1) && pos < nnz) lab[j] = (uint32_t)sym[pos];
        }
    }
};

// ------------------------------------------------------------------ the d table
// stage[j] = c[j] - c_z (j < k), -c_z past k; then `1 << cshift` copies of each entry as in k_cbmm_stream
// RT = bf16_t / f16_t: every centre (c_z too) rounded to RT (to nearest even) and widened back before the difference, as cb_fill.
template <typename RT = float> __device__ __forceinline__ float sp_cz(const float *__restrict__ centers, int k, int z)
{
    return z < k ? (float)(RT)centers[z] : 0.0f;
}

template <typename RT = float>
__device__ __forceinline__ void sp_fill(float *tab, float *stage, const float *__restrict__ centers, int k, float cz, int entries, int cshift)
{
    for (int j = threadIdx.x; j < entries; j += blockDim.x) stage[j] = (j < k ? (float)(RT)centers[j] : 0.0f) - cz;
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

// rs[r] = sum_i x[r, i] for r < m in a fixed order (k_cbsp_rowsum, nnc_cbsp.hip), launched on `s`: NNC_OK or the launch error.  x is
// float32, or (cbsp_rowsum_dt, dtype NNC_DT_BF16 / NNC_DT_F16) widened element by element into the same float32 sums.
int cbsp_rowsum_dt(const void *x, int dtype, long long m, long long kdim, float *rs, hipStream_t s);
static inline int cbsp_rowsum(const float *x, long long m, long long kdim, float *rs, hipStream_t s) { return cbsp_rowsum_dt(x, NNC_DT_F32, m, kdim, rs, s); }

// The two scans of the pack that do not look at a label (k_cbsp_rowscan, k_cbsp_basescan, nnc_cbsp.hip), launched on `s` behind a
// bits pass that left the popcount of every segment in lo: the counts of the form in lo and hi, the total in *nnz (may be NULL).
// The group-wise pack (nnc_cbsp_grouped.hip) runs them between its own bits and emit passes.  NNC_OK or the launch error.
int cbsp_pack_scans(long long kdim, long long segs, uint32_t *lo, uint32_t *hi, long long *nnz, hipStream_t s);

#define SP_ROWS 64               // rows whose bitmap words one vector load brings to a wave of k_cbsp_stream

// ------------------------------------------------------------------ the plan (host)
// Every decision nnc_cbsp_f32 takes before it launches (nnc_cbsp_h16 follows the stream plan for m <= 16; its m > 16 plan is cb_plan's).
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
// grid (segments, splits), CB_THREADS threads.  out: y (direct != 0) or the float32 partials [split][m][ncols]; rs_out: the row-sum
// partials [split][m] (split only; written by the segment-0 workgroups).  XT = float is nnc_cbsp_f32's kernel (nnc_cbsp.hip).  XT =
// bf16_t / f16_t is nnc_cbsp_h16's (nnc_cbsp_h16.hip): x is read as XT and widened (exact), the d table is built from the centres
// rounded to XT and widened, the arithmetic is the same float32 fmaf chain, and direct = 2 stores y as XT (one rounding) where
// direct = 1 stores float32.
template <typename XT, typename LT, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbsp_stream(const XT *__restrict__ x, int m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                            const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const LT *__restrict__ sym,
                                                            long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                            int z, int entries, int cshift, long long rows_per_split, const float *__restrict__ bias,
                                                            int relu, int direct, void *__restrict__ out_, float *__restrict__ rs_out)
{
    constexpr int U = CB_UNROLL;
    extern __shared__ float smem[];
    float *tab = smem;
    float *red = smem + (entries << cshift);          // [MT][64] accumulators, then [MT] row sums
    float *stage = red + MT * 65;
    float *out = reinterpret_cast<float *>(out_);
    const float cz = sp_cz<XT>(centers, k, z);
    sp_fill<XT>(tab, stage, centers, k, cz, entries, cshift);

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
                xa = (r0 < m && i + f0 % U < i1) ? (float)x[(long long)r0 * kdim + i + f0 % U] : 0.0f;
                xb = (MT * U > 64 && r1 < m && i + f1 % U < i1) ? (float)x[(long long)r1 * kdim + i + f1 % U] : 0.0f;
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
        if (direct) {
            const float v = sp_epilogue(acc[r], cz, rs[r], bias, col, relu);
            if (!std::is_same<XT, float>::value && direct == 2)
                reinterpret_cast<XT *>(out_)[(long long)r * ncols + col] = (XT)v;
            else
                out[(long long)r * ncols + col] = v;
        } else {
            out[((long long)blockIdx.y * m + r) * ncols + col] = acc[r];
        }
    }
}

// ------------------------------------------------------------------ split-K combine
// the partials as k_cbmm_reduce sums them (four quarters of the splits in order, then the quarters in order); the row sum of r
// is the sum of its rsplits partials in split order.  part == NULL (kdim = 0): y = bias.  RT: the type c_z is rounded to (sp_cz);
// YT: the type of y, the float32 value rounded once.
#define SP_RED_Q 4
template <typename RT, typename YT>
__global__ __launch_bounds__(256) void k_cbsp_reduce(const float *__restrict__ part, long long splits, long long m, long long ncols,
                                                     const float *__restrict__ rsp, long long rsplits, const float *__restrict__ centers, int k,
                                                     int z, const float *__restrict__ bias, int relu, YT *__restrict__ y)
{
    __shared__ float qs[SP_RED_Q - 1][64];
    const long long mn = m * ncols;
    const float cz = sp_cz<RT>(centers, k, z);
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long per_q = (splits + SP_RED_Q - 1) / SP_RED_Q;
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
            for (int j = 0; j < SP_RED_Q - 1; ++j) v += qs[j][o];
            const long long r = idx / ncols;
            float rs = 0.0f;
            for (long long s = 0; s < rsplits; ++s) rs += rsp[s * m + r];
            y[idx] = (YT)sp_epilogue(v, cz, rs, bias, idx - r * ncols, relu);
        }
    }
}
