// nnc_cbwp.hpp -- the host half of the 5-, 6- and 9-bit split-plane ("wide packed") codebook matmul (nnc_cbwp.hip, DESIGN.md
// section 36): the layout arithmetic and the limits of the form, the argument checks and the plan, and, shared with the backward
// pass (nnc_cbwpgrad.hip, section 37), the <BASE, PLANES> dispatch and the decode of a lane's plane bits.  The launch constants, the
// per-bank table, the tiles and the split-K combine are nnc_cbmm.hpp's; the aligned row load (pk_load), the accumulator budget
// (PK_ACC) and the size limit (pk_size_ok) are the packed form's, nnc_cbpk.hpp.
#pragma once
#include "nnc_cbpk.hpp"
#include "nnc_cbwp.h"

// ------------------------------------------------------------------ the layout (host)
static inline bool wp_bits_ok(int bits) { return bits == 5 || bits == 6 || bits == 9; }
static inline int wp_base(int bits) { return bits == 9 ? 8 : 4; }
static inline long long wp_base_bytes(long long ncols, int bits) { return 16 * cdiv(ncols * wp_base(bits), 128); }
static inline long long wp_plane_bytes(long long ncols) { return 16 * cdiv(ncols, 128); }
static inline long long wp_row_bytes(long long ncols, int bits) { return wp_base_bytes(ncols, bits) + (bits - wp_base(bits)) * wp_plane_bytes(ncols); }
// the per-bank table of the stream and MFMA kernels: 2^bits entries (centres, then zeros); 32 copies at 32 or 64 entries, at 512
// the copies CbTable<uint16_t>'s rule gives (the largest power of two with entries * copies <= CB_U16_WORDS: 16)
static inline int wp_cshift(int bits)
{
    int cshift = 0;
    while ((1 << cshift) < CB_U8_COPIES && (1LL << bits) << (cshift + 1) <= CB_U16_WORDS) ++cshift;
    return cshift;
}

// ------------------------------------------------------------------ argument checks (host)
static int wp_check_form(const char *fn, int64_t kdim, int64_t ncols, int bits)
{
    if (kdim < 0 || ncols < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (!wp_bits_ok(bits)) return fail(NNC_EINVAL, std::string(fn) + ": bits must be 5, 6 or 9");
    if (!pk_size_ok(kdim, ncols)) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

static int wp_check_buffer(const char *fn, const void *packed, int64_t packed_bytes, int64_t kdim, int64_t ncols, int bits)
{
    if (packed_bytes != kdim * wp_row_bytes(ncols, bits)) return fail(NNC_EINVAL, std::string(fn) + ": packed_bytes is not nnc_cbwp_pack_bytes(kdim, ncols, bits)");
    if (packed_bytes > 0 && !packed) return fail(NNC_EINVAL, std::string(fn) + ": packed is NULL");
    if (reinterpret_cast<uintptr_t>(packed) % 16) return fail(NNC_EINVAL, std::string(fn) + ": packed must be 16-byte aligned");
    return NNC_OK;
}

static int wp_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    if (x_dtype != NNC_DT_F32 && x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16)
        return fail(NNC_EINVAL, std::string(fn) + ": x_dtype must be NNC_DT_F32, NNC_DT_BF16 or NNC_DT_F16");
    if (m < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    const int rc = wp_check_form(fn, kdim, ncols, bits);
    if (rc != NNC_OK) return rc;
    if (k < 1 || k > (1 << bits)) return fail(NNC_EINVAL, std::string(fn) + ": k outside 1..2^bits");
    if (m > (1LL << 40)) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

// the checks of the group-wise entry points, forward (nnc_cbwp_grouped.hip) and backward (nnc_cbwpgrad_grouped.hip): 5 or 6 bits and
// 17 .. 64 centres, wp_check's, then those of group_rows (bins_k = k where the caller keeps G * k bins: cb_check_group_rows)
static int wpg_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t bins_k = 0)
{
    const std::string f(fn);
    if (bits == 9 || k > 64)
        return fail(NNC_EINVAL, f + ": k > 64 (bits 9) is refused: the group-wise byte form holds uint8 labels, and 9 bits would be larger than it");
    if (bits != 5 && bits != 6) return fail(NNC_EINVAL, f + ": bits must be 5 or 6");
    if (k <= 16) return fail(NNC_EINVAL, f + ": k <= 16 is refused: the 2- and 4-bit packed form serves it (nnc_cbpk_grouped)");
    const int rc = wp_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    return cb_check_group_rows(fn, kdim, group_rows, bins_k);
}

// ------------------------------------------------------------------ the plan (host)
// Every decision nnc_cbwp takes before it launches; nnc_cbwp_plan reports it.
struct WpPlan {
    int path;                // NNC_CBMM_NONE / _STREAM / _TILED / _BIAS / _MFMA
    int vb, mt;              // stream: base bytes per lane per row, rows of x per launch (a power of two >= m)
    int cols;                // stream: columns per lane per row (8 * vb / base): 4, 8, 16 or 32, so a lane's plane bits are a
                             // nibble, a byte, two bytes or a dword of the plane
    int base, planes;
    int copies, entries;
    long long col_tiles, row_tiles;
    long long splits, rows_per_split;
    long long lds;
};

static WpPlan wp_plan(int x_dtype, long long m, long long kdim, long long ncols, int bits, int cus)
{
    WpPlan p{};
    if (m == 0 || ncols == 0) return p;
    if (kdim == 0) {
        p.path = NNC_CBMM_BIAS;
        return p;
    }
    p.base = wp_base(bits);
    p.planes = bits - p.base;
    p.entries = 1 << bits;
    if (m > CB_SKINNY_M) {   // the grids of the byte form's tiles (cb_grid): the 128 x 128 float32 tile, the MFMA tile for half x
        CbPlan c{};
        cb_grid(c, m, kdim, ncols, 1, cus, x_dtype != NNC_DT_F32);
        p.path = c.path;
        p.col_tiles = c.col_tiles;
        p.row_tiles = c.row_tiles;
        p.splits = c.splits;
        p.rows_per_split = c.rows_per_split;
        if (p.path == NNC_CBMM_MFMA) {
            p.copies = 1 << wp_cshift(bits);
            p.lds = (long long)hm_table_words(p.entries, wp_cshift(bits)) * 4 + (long long)(HM_BM + HM_BN) * HM_LD * 2;
        } else {
            p.copies = 1;
            p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + p.entries) * 4;
        }
        return p;
    }
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    p.path = NNC_CBMM_STREAM;
    p.mt = cb_mt(m);
    p.copies = 1 << wp_cshift(bits);
    // every wave keeps at least one batch of rows; the partials (splits x m x ncols x 4 B) stay within the index stream
    const long long s_max = std::max(1LL, std::min(kdim / (CB_WAVES * CB_UNROLL), kdim * bits / (32 * m)));
    // columns per lane: at most a 16-byte load of the base part and PK_ACC accumulators; from there down to a 4-byte load, the
    // widest that keeps four lanes in five on a column and gives every CU of the planning device a workgroup, else the narrowest
    // (pk_plan's rule).  Shape alone decides, so the splits never shrink with more CUs.
    const int cap = std::min(128 / p.base, PK_ACC / p.mt);
    p.cols = cap;
    for (int c = cap; c * p.base >= 32 && c >= cap / 4; c /= 2) {
        p.cols = c;
        const long long tiles = cdiv(ncols, 64LL * c);
        if (tiles * 64 * c * 4 <= ncols * 5 && tiles * s_max >= CB_PLAN_CUS) break;
    }
    p.vb = p.cols * p.base / 8;
    p.row_tiles = 1;
    p.col_tiles = cdiv(ncols, 64LL * p.cols);
    const long long s = std::max(1LL, std::min(cdiv(2LL * cus, p.col_tiles), s_max));   // enough workgroups for two per CU
    p.rows_per_split = cdiv(kdim, s);
    p.splits = cdiv(kdim, p.rows_per_split);
    p.lds = ((long long)p.entries * p.copies + (long long)p.mt * p.cols * 64 + p.entries) * 4;
    return p;
}

static int64_t wp_ws_bytes(const WpPlan &p, long long m, long long ncols) { return p.splits > 1 ? (int64_t)p.splits * m * ncols * 4 : 0; }

// the one place that turns `bits` into <BASE, PLANES>
#define WP_BY_BITS(bits, CALL) ((bits) == 5 ? CALL(4, 1) : (bits) == 6 ? CALL(4, 2) : CALL(8, 1))

// ------------------------------------------------------------------ the decode the stream kernels of both directions share (device)
// the bits of `d` selected by `mask` at bit `from`, moved to bit `to` (both compile-time constants behind the unrolled loops)
__device__ __forceinline__ uint32_t wp_move(uint32_t d, int from, int to, uint32_t mask)
{
    return (from >= to ? d >> (from - to) : d << (to - from)) & (mask << to);
}

// a lane's E plane bits: a nibble (E = 4: the lane's half of the byte), a byte, two bytes or a dword of the plane; `p` is the
// plane's byte that holds the lane's first column, aligned to the width of the load
template <int E>
__device__ __forceinline__ uint32_t wp_plane_load(const unsigned char *p, int lane)
{
    if constexpr (E == 4) return (uint32_t)*p >> ((lane & 1) * 4);
    else if constexpr (E == 8) return *p;
    else if constexpr (E == 16) return *reinterpret_cast<const uint16_t *>(p);
    else return *reinterpret_cast<const uint32_t *>(p);
}
