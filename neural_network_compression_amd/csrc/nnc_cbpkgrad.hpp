// nnc_cbpkgrad.hpp -- the host side the backward pass of the packed codebook matmul (nnc_cbpkgrad.hip) shares with that of the
// group-wise packed form (nnc_cbpkgrad_grouped.hip): the plans of both directions, the argument check,
// the two constants of the kernels and the list of their stream instantiations.  The glue of the entry points (the lookup in that
// list, the plan checks, the sequences of HIP calls) is nnc_cbgrad.hpp's, shared with the other backward units.  The grouped unit follows these plans unchanged, so the path, the grids, the splits and the
// order of every sum are those of nnc_cbpk_dx_f32 / nnc_cbpk_dc_f32 on the same shape.  The ungrouped stream kernels
// (k_cbpkdx_stream, k_cbpkdc_stream) are here too, as templates on the element type of x and g: the half-precision unit
// (nnc_cbpk_h16.hip, section 25) instantiates the same text for bf16 / fp16.
#pragma once
#include "nnc_cbpk.hpp"
#include "nnc_cbtile.hpp"

#define PKG_RLOG2 6               // dc: 64 copies of every LDS bin, one per lane (K <= 16: at most 8 KiB)
#define PKG_G 64                  // stream: g values a lane keeps (columns per lane x rows of m), at most

// The (bits, vb, mt) of the stream kernels pg_stream_grid can ask for, written once: the tables of nnc_cbpkgrad.hip and of
// nnc_cbpkgrad_grouped.hip are both made from this list, so the grouped unit cannot miss a case the plan produces.
#define PKG_STREAM_CASES(X)                                                                                                  \
    X(4, 16, 1) X(4, 8, 1) X(4, 4, 1) X(4, 16, 2) X(4, 8, 2) X(4, 4, 2) X(4, 8, 4) X(4, 4, 4) X(4, 4, 8) X(4, 2, 16)          \
    X(2, 16, 1) X(2, 8, 1) X(2, 4, 1) X(2, 8, 2) X(2, 4, 2) X(2, 4, 4) X(2, 2, 8) X(2, 1, 16)

// ------------------------------------------------------------------ plans (host)
struct PgPlan {
    int path;                 // NNC_CBMM_NONE / _STREAM / _TILED / _ZERO
    int vb, mt, cols;         // stream: packed bytes per lane per row, rows of m per launch (a power of two >= m), 8 * vb / bits
    int entries, copies;      // dx: the LDS table; dc: the copies of every LDS bin
    long long col_tiles, row_tiles;   // stream: column blocks x row groups; tiled: tiles
    long long splits, per_split;      // dx: splits of ncols (columns per split); dc: splits of m (rows of m per split)
    long long rows_per_group;         // stream: packed rows per workgroup
    int terms_log2;                   // dc: T of nnc_cbmm_dc_plan
    long long lds;
};

// The stream geometry both directions share.  Columns per lane: at most a 16-byte load and PKG_G values of g; from there down to a
// 4-byte load, the widest that keeps four lanes in five on a column (the last column block may be nearly empty) and leaves the
// 256-CU planning device two workgroups per CU (column blocks x the most row groups kdim allows); else the narrowest.  The shape
// alone decides, so the column blocks (the splits of dx) never change with the device; row groups for two workgroups per CU.
static void pg_stream_grid(PgPlan &p, long long m, long long kdim, long long ncols, int bits, int cus)
{
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    p.path = NNC_CBMM_STREAM;
    p.mt = cb_mt(m);
    const long long max_groups = cdiv(kdim, (long long)CB_WAVES * CB_UNROLL);   // every wave keeps a batch of rows
    const int cap = std::min(128 / bits, PKG_G / p.mt);
    p.cols = cap;
    for (int c = cap; c * bits >= 32; c /= 2) {
        p.cols = c;
        const long long tiles = cdiv(ncols, 64LL * c);
        if (tiles * 64 * c * 4 <= ncols * 5 && tiles * max_groups >= 2LL * CB_PLAN_CUS) break;
    }
    p.vb = p.cols * bits / 8;
    p.col_tiles = cdiv(ncols, 64LL * p.cols);
    const long long groups = std::max(1LL, std::min(cdiv(2LL * cus, p.col_tiles), max_groups));
    p.rows_per_group = cdiv(kdim, groups);
    p.row_tiles = cdiv(kdim, p.rows_per_group);
}

static PgPlan pg_dx_plan(long long m, long long kdim, long long ncols, int bits, int cus)
{
    PgPlan p{};
    if (m == 0 || kdim == 0) return p;                       // NNC_CBMM_NONE: dx is empty
    if (ncols == 0) {                                        // dx = 0
        p.path = NNC_CBMM_ZERO;
        return p;
    }
    p.entries = 1 << bits;
    if (m <= CB_SKINNY_M) {
        pg_stream_grid(p, m, kdim, ncols, bits, cus);
        p.splits = p.col_tiles;                              // one split per column block
        p.per_split = 64LL * p.cols;
        p.copies = PK_COPIES;
        p.lds = ((long long)p.entries * PK_COPIES + p.entries) * 4;
    } else {
        p.path = NNC_CBMM_TILED;
        p.copies = 1;
        p.col_tiles = cdiv(kdim, TB_N);
        p.row_tiles = cdiv(m, TB_M);
        long long s = std::min({cdiv(2LL * CB_PLAN_CUS, p.col_tiles * p.row_tiles), ncols / (16 * TB_K), 16LL});
        s = std::max(1LL, s);
        p.per_split = cdiv(cdiv(ncols, s), 16) * 16;         // whole dwords at either width: a thread's 4 columns lie in one
        p.splits = cdiv(ncols, p.per_split);
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + p.entries) * 4;
    }
    return p;
}

// The splits of m and T are nnc_cbmm_dc_plan's for the same shape at label_bytes = 1 (so S, every image and every sum are the byte
// form's).  NNC_OK, or that plan's error.
static int pg_dc_plan(long long m, long long kdim, long long ncols, int bits, int k, int cus, PgPlan &p)
{
    p = PgPlan{};
    if (m == 0 || kdim == 0 || ncols == 0) {                 // no terms: dc = 0
        p.path = NNC_CBMM_ZERO;
        return NNC_OK;
    }
    int64_t d[NNC_CBDC_PLAN_LEN];
    const int rc = nnc_cbmm_dc_plan(m, kdim, ncols, 1, k, CB_PLAN_CUS, 0, d);
    if (rc != NNC_OK) return rc;
    p.splits = d[NNC_CBDC_P_SPLITS];
    p.per_split = d[NNC_CBDC_P_RPS];
    p.terms_log2 = (int)d[NNC_CBDC_P_TERMS_LOG2];
    p.copies = 1 << PKG_RLOG2;
    const long long bins = ((long long)k << PKG_RLOG2) * 8;
    if (m <= CB_SKINNY_M) {
        pg_stream_grid(p, m, kdim, ncols, bits, cus);
        p.lds = bins;
    } else {
        p.path = NNC_CBMM_TILED;
        p.col_tiles = cdiv(ncols, TB_N);
        p.row_tiles = cdiv(kdim, TB_M);
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N) * 4 + bins;
    }
    return NNC_OK;
}

// ------------------------------------------------------------------ argument checks (host)
static int pg_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    const int rc = pk_check(fn, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if (m > 0 && kdim > (1LL << 44) / m) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

// ------------------------------------------------------------------ the stream kernels (device)
// Templated on the element type of x and g: nnc_cbpkgrad.hip instantiates them for float32, nnc_cbpk_h16.hip for bf16 / fp16 (DESIGN.md
// section 25).
// ------------------------------------------------------------------ dx, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  out: dx (one column block; direct 1: float32, 2: XT) or the float32 partials
// [block][m][kdim].  XT = float is nnc_cbpk_dx_f32's kernel; XT = bf16_t / f16_t nnc_cbpk_dx_h16's (nnc_cbpk_h16.hip): g is read as XT and
// widened, the table holds the centres rounded to XT and widened, the arithmetic is the same float32 fmaf chain.
template <typename XT, int BITS, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbpkdx_stream(const XT *__restrict__ g, int m, long long kdim, const unsigned char *__restrict__ packed,
                                                              long long row_bytes, long long ncols, const float *__restrict__ centers, int k,
                                                              long long rows_per_group, int direct, void *__restrict__ out_)
{
    constexpr int E = 8 * VB / BITS, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BITS, ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    static_assert(E * MT <= PKG_G, "g values per lane");
    extern __shared__ float smem[];
    float *cb = smem;                                   // [ENTRIES][PK_COPIES]
    float *stage = smem + ENTRIES * PK_COPIES;
    float *out = reinterpret_cast<float *>(out_);
    cb_fill<XT>(cb, stage, centers, k, ENTRIES, PK_CSHIFT);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;                     // then the lane's VB bytes lie inside the padded row
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));   // the lane's columns inside the matrix
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (r < m && e < ne) ? (float)g[(long long)r * ncols + c0 + e] : 0.0f;

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const unsigned char *mine = packed + (active ? (long long)blockIdx.x * (64 * VB) + lane * VB : 0LL);
    const char *tab = reinterpret_cast<const char *>(cb) + ((lane & (PK_COPIES - 1)) << 2);
    float *dst = direct ? out : out + (long long)blockIdx.x * m * kdim;
    __syncthreads();

    auto consume = [&](const uint32_t *w, long long i) {
        float p[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) p[r] = 0.0f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            constexpr int SH = 7;                                        // entry l of this lane's copy at byte l << 7
            const int bit = BITS * (e % PER);
            const uint32_t d = w[e / PER];
            const uint32_t a = (bit >= SH ? d >> (bit - SH) : d << (SH - bit)) & (MASK << SH);
            const float wv = e < ne ? *reinterpret_cast<const float *>(tab + a) : 0.0f;   // (columns past the row: no Inf * 0)
#pragma unroll
            for (int r = 0; r < MT; ++r) p[r] = __builtin_fmaf(gv[r][e], wv, p[r]);
        }
        int row;
        const float v = wave_reduce_rows<MT>(p, lane, row);
        if ((lane & (64 / MT - 1)) == 0 && row < m) {
            if (!std::is_same<XT, float>::value && direct == 2)
                reinterpret_cast<XT *>(out_)[(long long)row * kdim + i] = (XT)v;
            else
                dst[(long long)row * kdim + i] = v;
        }
    };

    long long i = i0;
    for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
        uint32_t w[CB_UNROLL][N];
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) pk_load<VB>(mine + (i + u) * row_bytes, w[u]);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], i + u);
    }
    for (; i < i1; ++i) {
        uint32_t w[N];
        pk_load<VB>(mine + i * row_bytes, w);
        consume(w, i);
    }
}


// ------------------------------------------------------------------ dc, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  LDS: the bins, [k][64] int64, copy `lane` of every bin this lane's own.
// XT = bf16_t / f16_t (nnc_cbpk_dc_h16): x and g are widened as they are loaded; the rest is the float32 kernel.
template <typename XT, int BITS, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbpkdc_stream(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
                                                              const unsigned char *__restrict__ packed, long long row_bytes, long long ncols, int k,
                                                              int terms_log2, long long rows_per_group, uint32_t *__restrict__ hdr,
                                                              unsigned long long *__restrict__ sums)
{
    constexpr int E = 8 * VB / BITS, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    static_assert(E * MT <= PKG_G, "g values per lane");
    extern __shared__ unsigned long long bins[];
    int flag;
    const int S = cbdc_shift(hdr, m, terms_log2, flag);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        hdr[2] = (uint32_t)S;
        hdr[3] = (uint32_t)flag;
    }
    if (flag != CBG_FLAG_OK) return;   // (uniform over the launch)
    int scx, scg;
    cbdc_scales(hdr, scx, scg);
    const int Sw = S - scx - scg;      // the shift of dW' = dW * 2^(scx + scg)
    for (int j = threadIdx.x; j < (k << PKG_RLOG2); j += CB_THREADS) bins[j] = 0ull;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (float)g[cbdc_idx((long long)r * ncols + c0 + e, r < m && e < ne)];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = cbdc_scaled(gv[r][e], r < m && e < ne, scg);

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const unsigned char *mine = packed + (active ? (long long)blockIdx.x * (64 * VB) + lane * VB : 0LL);
    unsigned long long *mybins = bins + lane;
    __syncthreads();

    auto load_x = [&](long long i, int U, float &xa, float &xb) { cbdc_load_x<MT>(x, kdim, m, scx, lane, i, U, xa, xb); };
    auto consume = [&](const uint32_t *w, float xa, float xb, int u, int U) {
        float xv[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            const int f = r * U + u;
            xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t l = (w[e / PER] >> (BITS * (e % PER))) & MASK;
            float d = 0.0f;
#pragma unroll
            for (int r = 0; r < MT; ++r) d = __builtin_fmaf(xv[r], gv[r][e], d);   // dW'[i, o], r ascending
            if (e < ne && l < (uint32_t)k) atomicAdd(&mybins[l << PKG_RLOG2], cbdc_fix(d, Sw));
        }
    };

    long long i = i0;
    for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
        uint32_t w[CB_UNROLL][N];
        float xa, xb;
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) pk_load<VB>(mine + (i + u) * row_bytes, w[u]);
        load_x(i, CB_UNROLL, xa, xb);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], xa, xb, u, CB_UNROLL);
    }
    for (; i < i1; ++i) {
        uint32_t w[N];
        float xa, xb;
        pk_load<VB>(mine + i * row_bytes, w);
        load_x(i, 1, xa, xb);
        consume(w, xa, xb, 0, 1);
    }
    cbdc_flush(bins, k, PKG_RLOG2, sums);
}
