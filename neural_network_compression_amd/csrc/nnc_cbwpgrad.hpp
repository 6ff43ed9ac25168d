// nnc_cbwpgrad.hpp -- the host half of the backward pass of the 5-, 6- and 9-bit split-plane ("wide packed") codebook matmul
// (nnc_cbwpgrad.hip): the list of its stream instantiations, the plans of both directions and the argument
// check.  Nothing here is new arithmetic: the layout and the table copies are nnc_cbwp.hpp's (wp_*), the stream geometry is the
// packed form's rule with the base width in the place of `bits` (pg_stream_grid, nnc_cbpkgrad.hpp, whose PgPlan this unit fills),
// the MFMA tiles and splits are nnc_cbh16plan.hpp's, the copies of the dc bins the byte form's (dc_rlog2), and the splits of m and
// T of dc are read from the byte form's own plan calls, so S, every dW and every sum are that form's.
#pragma once
#include "nnc_cbwp.hpp"
#include "nnc_cbh16plan.hpp"
#include "nnc_cbpkgrad.hpp"
#include "nnc_cbwpgrad.h"

// The (BASE, PLANES, VB, MT) of the stream kernels wg_dx_plan / wg_dc_plan can ask for, written once: pg_stream_grid at bits = BASE
// gives, per MT, the VB of PKG_STREAM_CASES' 4-bit rows at BASE = 4 and 16 / 8 / 4 bytes down from min(16, 64 / MT) at BASE = 8.
#define WPG_BASE4_CASES(X, P) X(4, P, 16, 1) X(4, P, 8, 1) X(4, P, 4, 1) X(4, P, 16, 2) X(4, P, 8, 2) X(4, P, 4, 2) X(4, P, 8, 4) X(4, P, 4, 4) X(4, P, 4, 8) X(4, P, 2, 16)
#define WPG_BASE8_CASES(X)                                                                                                          \
    X(8, 1, 16, 1) X(8, 1, 8, 1) X(8, 1, 4, 1) X(8, 1, 16, 2) X(8, 1, 8, 2) X(8, 1, 4, 2) X(8, 1, 16, 4) X(8, 1, 8, 4) X(8, 1, 4, 4) \
    X(8, 1, 8, 8) X(8, 1, 4, 8) X(8, 1, 4, 16)
#define WPG_STREAM_CASES(X) WPG_BASE4_CASES(X, 1) WPG_BASE4_CASES(X, 2) WPG_BASE8_CASES(X)

// ------------------------------------------------------------------ plans (host)
// PgPlan's fields as the packed form reads them; copies is the per-bank copies of the table (dx) or of every bin (dc).
static PgPlan wg_dx_plan(int x_dtype, long long m, long long kdim, long long ncols, int bits, int cus)
{
    PgPlan p{};
    if (m == 0 || kdim == 0) return p;                       // NNC_CBMM_NONE: dx is empty
    if (ncols == 0) {                                        // dx = 0
        p.path = NNC_CBMM_ZERO;
        return p;
    }
    const int entries = 1 << bits, cshift = wp_cshift(bits);
    if (m <= CB_SKINNY_M) {
        pg_stream_grid(p, m, kdim, ncols, wp_base(bits), cus);
        p.splits = p.col_tiles;                              // one split per column block
        p.per_split = 64LL * p.cols;
        p.copies = 1 << cshift;
        p.lds = (((long long)entries << cshift) + entries) * 4;
    } else if (x_dtype != NNC_DT_F32) {
        p = h16_mfma_plan<PgPlan>(h16_dx_tiles(m, kdim, ncols), (long long)hm_table_words(entries, cshift) * 4);
        p.copies = 1 << cshift;
    } else {
        p.path = NNC_CBMM_TILED;
        p.copies = 1;
        p.col_tiles = cdiv(kdim, TB_N);
        p.row_tiles = cdiv(m, TB_M);
        const long long s = std::max(1LL, std::min({cdiv(2LL * CB_PLAN_CUS, p.col_tiles * p.row_tiles), ncols / (16 * TB_K), 16LL}));
        p.per_split = cdiv(cdiv(ncols, s), 32) * 32;         // whole plane dwords: a thread's 4 plane bits lie in one
        p.splits = cdiv(ncols, p.per_split);
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + entries) * 4;
    }
    p.entries = entries;
    return p;
}

// The path, the splits of m and T are the byte form's plan call for the same shape (nnc_cbmm_dc_plan for float32,
// nnc_cbmm_dc_h16_plan for half) at label_bytes = 1 (bits 5, 6) or 2 (bits 9).  NNC_OK, or that plan's error.
static int wg_dc_plan(int x_dtype, long long m, long long kdim, long long ncols, int bits, int k, int cus, PgPlan &p)
{
    p = PgPlan{};
    if (m == 0 || kdim == 0 || ncols == 0) {                 // no terms: dc = 0
        p.path = NNC_CBMM_ZERO;
        return NNC_OK;
    }
    const int lb = bits > 8 ? 2 : 1;
    int64_t d[NNC_CBDC_H16_PLAN_LEN];
    const int rc = x_dtype == NNC_DT_F32 ? nnc_cbmm_dc_plan(m, kdim, ncols, lb, k, CB_PLAN_CUS, 0, d)
                                         : nnc_cbmm_dc_h16_plan(x_dtype, m, kdim, ncols, lb, k, CB_PLAN_CUS, 0, d);
    if (rc != NNC_OK) return rc;
    const long long bins = ((long long)k << dc_rlog2(k)) * 8;
    if (d[NNC_CBDC_P_PATH] == NNC_CBMM_STREAM) {
        pg_stream_grid(p, m, kdim, ncols, wp_base(bits), cus);
        p.lds = bins;
    } else {
        p.path = (int)d[NNC_CBDC_P_PATH];                    // NNC_CBMM_TILED (float32) or NNC_CBMM_MFMA (half): 128 x 128 tiles of dW
        p.col_tiles = d[NNC_CBDC_P_COL_TILES];
        p.row_tiles = d[NNC_CBDC_P_ROW_TILES];
        p.lds = bins + (p.path == NNC_CBMM_MFMA ? (long long)(HM_BM + HM_BN) * HM_LD * 2 : (long long)(TB_K * TB_M + TB_K * TB_N) * 4);
    }
    p.splits = d[NNC_CBDC_P_SPLITS];
    p.per_split = d[NNC_CBDC_P_RPS];
    p.terms_log2 = (int)d[NNC_CBDC_P_TERMS_LOG2];
    p.copies = 1 << dc_rlog2(k);
    return NNC_OK;
}

// ------------------------------------------------------------------ argument checks (host)
static int wg_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    const int rc = wp_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if (m > 0 && kdim > (1LL << 44) / m) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

// ------------------------------------------------------------------ what the group-wise unit (nnc_cbwpgrad_grouped.hip, section 39) shares
// the packed buffer as the launches carry it
struct WgArgs {
    const unsigned char *packed;
    long long base_bytes, plane_bytes, ncols;
};

// the table of a unit's stream instantiations for x_dtype: one per dtype, the same cases (N)
template <typename Case, size_t N> static inline const Case (&wg_cases(int dt, const Case (&f32)[N], const Case (&bf16)[N], const Case (&f16)[N]))[N]
{
    return dt == NNC_DT_F32 ? f32 : (dt == NNC_DT_BF16 ? bf16 : f16);
}

// label (i, o)'s base field from the dword `w` that holds it and its plane bits from the plane dwords pl[] (bit o % 32)
template <int BASE, int PLANES>
__device__ __forceinline__ uint32_t wg_label(uint32_t w, const uint32_t *pl, long long o)
{
    constexpr int PER = 32 / BASE;
    uint32_t l = (w >> (BASE * (int)(o % PER))) & ((1u << BASE) - 1);
#pragma unroll
    for (int p = 0; p < PLANES; ++p) l |= ((pl[p] >> (int)(o & 31)) & 1u) << (BASE + p);
    return l;
}
