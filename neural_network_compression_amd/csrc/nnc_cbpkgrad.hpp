// nnc_cbpkgrad.hpp -- the host side the backward pass of the packed codebook matmul (nnc_cbpkgrad.hip) shares with that of the
// group-wise packed form (nnc_cbpkgrad_grouped.hip): the plans of both directions, the argument check,
// the two constants of the kernels and the list of their stream instantiations.  The glue of the entry points (the lookup in that
// list, the plan checks, the sequences of HIP calls) is nnc_cbgrad.hpp's, shared with the other backward units.  The grouped unit follows these plans unchanged, so the path, the grids, the splits and the
// order of every sum are those of nnc_cbpk_dx_f32 / nnc_cbpk_dc_f32 on the same shape.
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
