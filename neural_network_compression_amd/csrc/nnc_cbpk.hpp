// nnc_cbpk.hpp -- what the 2- and 4-bit packed codebook matmul (nnc_cbpk.hip) shares with its backward pass (nnc_cbpkgrad.hip):
// the layout arithmetic and the limits of the packed form, the argument checks, the constants of the per-bank lookup table and
// the aligned row load of the stream kernels; and with the group-wise packed call (nnc_cbpk_grouped.hip) also the plan.
#pragma once
#include "nnc_cbmm.hpp"

#define PK_COPIES 32              // per-bank copies of the table
#define PK_CSHIFT 5
#define PK_ACC 64                 // accumulators per lane: columns per lane per row x rows of x

// ------------------------------------------------------------------ the layout (host)
static inline bool pk_bits_ok(int bits) { return bits == 2 || bits == 4; }
static inline long long pk_row_bytes(long long ncols, int bits) { return 16 * cdiv(ncols * bits, 128); }
static inline bool pk_size_ok(int64_t kdim, int64_t ncols) { return kdim <= (1LL << 40) && ncols <= (1LL << 40) && (ncols == 0 || kdim <= (1LL << 44) / cdiv(ncols, 2)); }

// ------------------------------------------------------------------ argument checks (host)
static int pk_check_form(const char *fn, int64_t kdim, int64_t ncols, int bits)
{
    if (kdim < 0 || ncols < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (!pk_bits_ok(bits)) return fail(NNC_EINVAL, std::string(fn) + ": bits must be 2 or 4");
    if (!pk_size_ok(kdim, ncols)) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

static int pk_check_buffer(const char *fn, const void *packed, int64_t packed_bytes, int64_t kdim, int64_t ncols, int bits)
{
    if (packed_bytes != kdim * pk_row_bytes(ncols, bits)) return fail(NNC_EINVAL, std::string(fn) + ": packed_bytes is not nnc_cbpk_pack_bytes(kdim, ncols, bits)");
    if (packed_bytes > 0 && !packed) return fail(NNC_EINVAL, std::string(fn) + ": packed is NULL");
    if (reinterpret_cast<uintptr_t>(packed) % 16) return fail(NNC_EINVAL, std::string(fn) + ": packed must be 16-byte aligned");
    return NNC_OK;
}

static int pk_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    if (m < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    const int rc = pk_check_form(fn, kdim, ncols, bits);
    if (rc != NNC_OK) return rc;
    if (k < 1 || k > (1 << bits)) return fail(NNC_EINVAL, std::string(fn) + ": k outside 1..2^bits");
    if (m > (1LL << 40)) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

// ------------------------------------------------------------------ the plan (host)
// Every decision nnc_cbpk_f32 takes before it launches; nnc_cbpk_plan reports it.  The group-wise packed call (nnc_cbpk_grouped.hip)
// takes the same plan for its stream and tiled kernels.
struct PkPlan {
    int path;                // NNC_CBMM_NONE / _STREAM / _TILED / _BIAS
    int vb, mt;              // stream: packed bytes per lane per row, rows of x per launch (a power of two >= m)
    int cols, xrows;         // stream: columns per lane per row (8 * vb / bits), rows of x per pass over the indices (= mt: one pass)
    int table, copies, entries;
    long long col_tiles, row_tiles;
    long long splits, rows_per_split;
    long long lds;
};

static PkPlan pk_plan(long long m, long long kdim, long long ncols, int bits, int cus)
{
    PkPlan p{};
    if (m == 0 || ncols == 0) return p;
    if (kdim == 0) {
        p.path = NNC_CBMM_BIAS;
        return p;
    }
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    p.table = NNC_CBPK_TABLE_BANKED;
    p.entries = 1 << bits;
    long long s;
    if (m <= CB_SKINNY_M) {
        p.path = NNC_CBMM_STREAM;
        p.mt = cb_mt(m);
        p.xrows = p.mt;
        // every wave keeps at least one batch of rows; the partials (splits x m x ncols x 4 B) stay within the packed index
        // stream (kdim x ncols x bits / 8 B)
        const long long s_max = std::max(1LL, std::min(kdim / (CB_WAVES * CB_UNROLL), kdim * bits / (32 * m)));
        // bytes per lane: at most a 16-byte load and PK_ACC accumulators; from there down to 4 bytes, the widest load that
        // keeps four lanes in five on a column (the last column tile may be nearly empty) and gives every CU of the planning
        // device a workgroup; else the narrowest.  Shape alone decides, so the splits below never shrink with more CUs.
        const int cap = std::min(128 / bits, PK_ACC / p.mt);
        p.cols = cap;
        for (int c = cap; c * bits >= 32; c /= 2) {
            p.cols = c;
            const long long tiles = cdiv(ncols, 64LL * c);
            if (tiles * 64 * c * 4 <= ncols * 5 && tiles * s_max >= CB_PLAN_CUS) break;
        }
        p.vb = p.cols * bits / 8;
        p.copies = PK_COPIES;
        p.row_tiles = 1;
        p.col_tiles = cdiv(ncols, 64LL * p.cols);
        s = std::min(cdiv(2LL * cus, p.col_tiles), s_max);          // enough workgroups for two per CU
        p.lds = ((long long)p.entries * p.copies + (long long)p.mt * p.cols * 64 + p.entries) * 4;
    } else {
        p.path = NNC_CBMM_TILED;
        p.copies = 1;
        p.col_tiles = cdiv(ncols, TB_N);
        p.row_tiles = cdiv(m, TB_M);
        s = std::min({cdiv(2LL * cus, p.col_tiles * p.row_tiles), kdim / (16 * TB_K), 16LL});
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + p.entries) * 4;
    }
    s = std::max(1LL, s);
    p.rows_per_split = cdiv(kdim, s);
    p.splits = cdiv(kdim, p.rows_per_split);
    return p;
}

static int64_t pk_ws_bytes(const PkPlan &p, long long m, long long ncols) { return p.splits > 1 ? (int64_t)p.splits * m * ncols * 4 : 0; }

// ------------------------------------------------------------------ a lane's VB bytes of a packed row (aligned: VB divides 16)
template <int VB>
__device__ __forceinline__ void pk_load(const unsigned char *p, uint32_t *w)
{
    if constexpr (VB == 1) w[0] = *p;
    else if constexpr (VB == 2) w[0] = *reinterpret_cast<const uint16_t *>(p);
    else load_chunk<VB>(p, w);
}
