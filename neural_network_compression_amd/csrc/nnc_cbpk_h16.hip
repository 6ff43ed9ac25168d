// nnc_cbpk_h16.hip -- the 2- and 4-bit packed codebook layer on bf16 / fp16 activations, forward and backward, from the packed
// indices (include/nnc_cbpk_h16.h, nnc_cbpk_h16 / nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16).  W_h[i, o] = the centre
// of label (i, o) rounded to the type of x, a label >= K reading 0.  A product of two bf16 or two fp16 values is exact in float32,
// every sum is float32, dc is binned as section 12's exact integers.
//
//   forward   nnc_cbpk_grouped (nnc_cbpk_grouped.hip, section 18) with one group: no kernel of its own.
//   m <= 16   k_cbpkdx_stream<XT> / k_cbpkdc_stream<XT> of nnc_cbpkgrad.hpp: section 15's stream plans and kernels with g and x
//             widened as they are loaded and, for dx, the table of the rounded centres.  Bit for bit the float32 entry points on
//             the widened inputs.
//   k_cbpkdx_mfma  m > 16.  k_cbdx_mfma's tile, main loop (hm_accumulate, nnc_cbmfma.hpp), tiles and splits (nnc_cbh16plan.hpp); g is
//             the A operand (hm_load_x / hm_store_x).
//             The B operand W^T: thread t owns index row n0 + (t mod 128) and the 16 consecutive o of its half of the k step, which
//             are 8 bytes (4 bits) or 4 bytes (2 bits) of the packed row: naturally aligned (a row starts on 16 bytes, a split on
//             a multiple of 32 columns) and inside the row (32 fields are at most one 16-byte granule).  One load, the fields looked
//             up in the 2^BITS-entry per-bank table, hm_store_w.  A column at or past ncols is 0 in the image, not table[0]: the
//             padding fields hold label 0, and a centre that rounds to Inf would otherwise meet the zero of the g image.
//   k_cbpkdc_mfma  m > 16.  k_cbdc_mfma's main loop (dcm_accumulate, nnc_cbgrad_h16.hpp), so the same accumulators; in the epilogue the 32 lanes of
//             an accumulator row read 32 consecutive fields of one packed row (16 or 8 bytes): a lane loads the dword that holds
//             its field, shifts and masks.  Every lane adds into its own copy of the K <= 16 bins (64 copies, at most 8 KiB).
// No load leaves the packed buffer: rows past kdim and columns past the split (dx) or past ncols (dc) load nothing.  Everything past
// m, kdim, ncols and the end of a split is zero in the images, never memory.  No float atomics; no host read.
#include "nnc_cbgrad_h16.hpp"
#include "nnc_cbh16plan.hpp"
#include "nnc_cbpkgrad.hpp"

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads; out, direct and cols_per_split as k_cbdx_mfma
template <typename XT, int BITS, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbpkdx_mfma(const XT *__restrict__ g, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                            long long row_bytes, long long ncols, const float *__restrict__ centers, int k,
                                                            long long col_tiles, long long cols_per_split, int direct, void *__restrict__ out_)
{
    constexpr int ENTRIES = 1 << BITS, PER = 32 / BITS, NW = 16 / PER;   // NW: the dwords of a thread's 16 fields
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    float *cb = hm_smem;                                // [ENTRIES][PK_COPIES]
    float *stage = cb + ENTRIES * PK_COPIES;            // ENTRIES
    XT *gs = reinterpret_cast<XT *>(hm_smem + hm_table_words(ENTRIES, PK_CSHIFT));   // [HM_BM][HM_LD]: g tile, row-major in o
    XT *ws = gs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: W^T tile, [i][o]
    cb_fill<XT>(cb, stage, centers, k, ENTRIES, PK_CSHIFT);

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);   // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const long long gi = T.n0 + T.wc;
    const bool row_ok = gi < kdim;
    const unsigned char *prow = packed + (row_ok ? gi * row_bytes : 0LL);
    uint32_t lw[NW];

    auto load_w = [&](long long ob) {
        const long long o0 = ob + T.wk0;                // a multiple of 16: the 16 fields are 16 * BITS / 8 aligned bytes
#pragma unroll
        for (int d = 0; d < NW; ++d) lw[d] = 0u;
        if (row_ok && o0 < T.k_hi) {                    // (k_hi <= ncols: the bytes lie inside the padded row)
            const unsigned char *p = prow + o0 * BITS / 8;
            if constexpr (NW == 2) {
                const uint2 v = *reinterpret_cast<const uint2 *>(p);
                lw[0] = v.x, lw[1] = v.y;
            } else {
                lw[0] = *reinterpret_cast<const uint32_t *>(p);
            }
        }
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t l = (lw[j / PER] >> (BITS * (j % PER))) & MASK;
            // a column past the split, so every column past ncols, is 0 and not table[label 0 of the padding]
            w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? cb[(l << PK_CSHIFT) | (T.lane & (PK_COPIES - 1))] : 0.0f;
        }
        hm_store_w(ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(g, m, ncols, T, gs, ws, acc, load_w, store_w);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads.  LDS: the two images, then the bins [k][64] int64, copy `lane` of
// every bin this lane's own.  rows_per_split and XVEC as k_cbdc_mfma.
template <typename XT, int BITS, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbpkdc_mfma(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                            const unsigned char *__restrict__ packed, long long row_bytes, long long ncols, int k,
                                                            int terms_log2, long long col_tiles, long long rows_per_split, uint32_t *__restrict__ hdr,
                                                            unsigned long long *__restrict__ sums)
{
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    XT *xs = reinterpret_cast<XT *>(hm_smem);           // [HM_BM][HM_LD]: x^T tile, [i][r]
    XT *gs = xs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: g^T tile, [o][r]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + HM_BN * HM_LD);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, k << PKG_RLOG2, scx, scg, Sw)) return;   // (uniform over the launch)
    dcm_scales<XT>(scx, scg, Sw);

    const HmTile T = hm_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i, [k_lo, k_hi): rows r
    typename HFrag<XT>::C acc[2][2];
    dcm_accumulate<XT, XVEC>(x, g, kdim, ncols, T, scx, scg, xs, gs, acc);

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col): the 32 lanes of a row read 32 consecutive fields of packed row i,
    // which start on a multiple of 32 columns; a lane's dword lies inside the padded row when its column lies inside the matrix
    unsigned long long *mybins = bins + T.lane;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const long long o = hm_acc_col(T.n0 + T.wn, b, T.lane);
            if (o >= ncols) continue;
            const long long bitpos = o * BITS;
            const unsigned char *pcol = packed + ((bitpos >> 5) << 2);
            const int sh = (int)(bitpos & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = hm_acc_row(T.m0 + T.wm, a, r, T.lane);
                if (i >= kdim) continue;
                const uint32_t l = (*reinterpret_cast<const uint32_t *>(pcol + i * row_bytes) >> sh) & MASK;
                if (l < (uint32_t)k) atomicAdd(&mybins[l << PKG_RLOG2], cbdc_fix(acc[a][b][r], Sw));
            }
        }
    }
    cbdc_flush(bins, k, PKG_RLOG2, sums);
}

// ------------------------------------------------------------------ plans (host)
// m <= 16 and the empty shapes: section 15's plans (pg_dx_plan, pg_dc_plan) field for field.  m > 16: nnc_cbh16plan.hpp's tiles and
// splits, so the tiles, the splits, S and every image are the byte form's; the table is the packed form's (2^bits entries x
// PK_COPIES), the bins one copy per lane.
static PgPlan h16_dx_plan(long long m, long long kdim, long long ncols, int bits, int cus)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return pg_dx_plan(m, kdim, ncols, bits, cus);
    PgPlan p = h16_mfma_plan<PgPlan>(h16_dx_tiles(m, kdim, ncols), (long long)hm_table_words(1 << bits, PK_CSHIFT) * 4);
    p.entries = 1 << bits;
    p.copies = PK_COPIES;
    return p;
}

static int h16_dc_plan(long long m, long long kdim, long long ncols, int bits, int k, int cus, PgPlan &p)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return pg_dc_plan(m, kdim, ncols, bits, k, cus, p);
    p = h16_mfma_plan<PgPlan>(h16_dc_tiles(m, kdim, ncols), ((long long)k << PKG_RLOG2) * 8);
    p.copies = 1 << PKG_RLOG2;
    return NNC_OK;
}

// ------------------------------------------------------------------ launches
template <typename XT, int BITS, int VB, int MT>
static void launch_dx_stream(dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const unsigned char *packed, long long row_bytes,
                             long long ncols, const float *centers, int k, long long rpg, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbpkdx_stream<XT, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(g), m, kdim, packed, row_bytes, ncols,
                       centers, k, rpg, direct, out);
}

template <typename XT, int BITS, int VB, int MT>
static void launch_dc_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const unsigned char *packed,
                             long long row_bytes, long long ncols, int k, int tl, long long rpg, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbpkdc_stream<XT, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m,
                       kdim, packed, row_bytes, ncols, k, tl, rpg, hdr, sums);
}

template <typename XT, int BITS>
static void launch_dx_mfma(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const unsigned char *packed, long long row_bytes,
                           long long ncols, const float *centers, int k, long long col_tiles, long long cps, int direct, void *out)
{
    hm_launch(g, ncols, k_cbpkdx_mfma<XT, BITS, true>, k_cbpkdx_mfma<XT, BITS, false>, grid, lds, s, reinterpret_cast<const XT *>(g), m, kdim, packed, row_bytes,
              ncols, centers, k, col_tiles, cps, direct, out);
}

template <typename XT, int BITS>
static void launch_dc_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const unsigned char *packed,
                           long long row_bytes, long long ncols, int k, int tl, long long col_tiles, long long rps, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((dcm_xvec(x, g, kdim, ncols) ? k_cbpkdc_mfma<XT, BITS, true> : k_cbpkdc_mfma<XT, BITS, false>), grid, dim3(HM_THREADS), lds, s,
                       reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim, packed, row_bytes, ncols, k, tl, col_tiles, rps, hdr, sums);
}

// every kernel instantiation of this unit, a table of the stream ones (the list of nnc_cbpkgrad.hpp) per dtype; the plans are checked
// against these tables, and the launches go through them
using DxStream = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const unsigned char *, long long, long long, const float *, int, long long,
                          int, void *);
using DcStream = void (*)(dim3, size_t, hipStream_t, const void *, const void *, int, long long, const unsigned char *, long long, long long, int, int,
                          long long, uint32_t *, unsigned long long *);
using DxMfma = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const unsigned char *, long long, long long, const float *, int,
                        long long, long long, int, void *);
using DcMfma = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const unsigned char *, long long, long long, int, int,
                        long long, long long, uint32_t *, unsigned long long *);
struct StreamCase {
    int a, vb, mt;            // a: bits
    DxStream dx;
    DcStream dc;
};
struct MfmaCase {
    int dt, a;                // a: bits
    DxMfma dx;
    DcMfma dc;
};
#define BF_CASE(B, V, M) {B, V, M, launch_dx_stream<bf16_t, B, V, M>, launch_dc_stream<bf16_t, B, V, M>},
#define HF_CASE(B, V, M) {B, V, M, launch_dx_stream<f16_t, B, V, M>, launch_dc_stream<f16_t, B, V, M>},
static const StreamCase kBf16Cases[] = {PKG_STREAM_CASES(BF_CASE)};
static const StreamCase kF16Cases[] = {PKG_STREAM_CASES(HF_CASE)};
#undef BF_CASE
#undef HF_CASE
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 4, launch_dx_mfma<bf16_t, 4>, launch_dc_mfma<bf16_t, 4>}, {NNC_DT_BF16, 2, launch_dx_mfma<bf16_t, 2>, launch_dc_mfma<bf16_t, 2>},
    {NNC_DT_F16, 4, launch_dx_mfma<f16_t, 4>, launch_dc_mfma<f16_t, 4>},   {NNC_DT_F16, 2, launch_dx_mfma<f16_t, 2>, launch_dc_mfma<f16_t, 2>},
};
static const CbgCaseNames kPkNames = {false, "bits", true};

// ------------------------------------------------------------------ C ABI
static int h16_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    const int rc = h16_check_dtype(fn, x_dtype);
    return rc != NNC_OK ? rc : pg_check(fn, m, kdim, ncols, bits, k);
}

// the one group of the forward call: every index row of the layer, as a multiple of 32
static inline int64_t one_group_rows(int64_t kdim) { return std::max<int64_t>(32, 32 * cdiv(kdim, 32)); }

// an error nnc_cbpk_grouped / nnc_cbpk_grouped_plan reported, under the name of the entry point that was called
static int renamed(const char *fn, int rc)
{
    if (rc == NNC_OK) return rc;
    const std::string e(nnc_last_error());
    const size_t colon = e.find(": ");
    return fail(rc, std::string(fn) + (colon == std::string::npos ? ": " + e : e.substr(colon)));
}

extern "C" int64_t nnc_cbpk_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (pk_check("nnc_cbpk_h16_workspace_bytes", m, kdim, ncols, bits, 1) != NNC_OK) return 0;
    return nnc_cbpk_grouped_workspace_bytes(NNC_DT_BF16, m, kdim, ncols, bits);
}

extern "C" int nnc_cbpk_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbpk_h16_plan";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if (!out) return fail(NNC_EINVAL, "nnc_cbpk_h16_plan: out is NULL");
    int64_t g[NNC_CBPK_GROUPED_PLAN_LEN];
    if ((rc = renamed(fn, nnc_cbpk_grouped_plan(x_dtype, m, kdim, ncols, bits, k, one_group_rows(kdim), cus, g))) != NNC_OK) return rc;
    for (int i = 0; i < NNC_CBPK_PLAN_LEN; ++i) out[i] = g[i];
    out[NNC_CBPK_H16_P_DTYPE] = x_dtype;
    return NNC_OK;
}

extern "C" int nnc_cbpk_h16(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                            const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, void *y, int y_dtype, void *workspace,
                            int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbpk_h16";
    const int rc = h16_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    return renamed(fn, nnc_cbpk_grouped(x, x_dtype, m, kdim, packed, packed_bytes, bits, ncols, centers_dev, k, one_group_rows(kdim), bias_dev, relu, y, y_dtype,
                                        workspace, workspace_bytes, stream));
}

extern "C" int64_t nnc_cbpk_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (pg_check("nnc_cbpk_dx_h16_workspace_bytes", m, kdim, ncols, bits, 1) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(h16_dx_plan(m, kdim, ncols, bits, CB_PLAN_CUS).splits, m, kdim);
}

extern "C" int nnc_cbpk_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbpk_dx_h16_plan";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    const PgPlan p = h16_dx_plan(m, kdim, ncols, bits, std::max(cus, 1));
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kPkNames, p.path, x_dtype, bits, mc)) != NNC_OK) return rc;
    const int64_t v[NNC_CBPKDX_H16_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.copies, p.entries, p.splits, p.per_split, p.lds, p.col_tiles, p.row_tiles,
                                                cbg_dx_ws_bytes(p.splits, m, kdim), x_dtype};
    for (int i = 0; i < NNC_CBPKDX_H16_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbpk_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                               const float *centers_dev, int32_t k, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbpk_dx_h16";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbpk_dx_h16: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbpk_dx_h16: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbpk_dx_h16: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbpk_dx_h16: g is NULL");
    if (reinterpret_cast<uintptr_t>(g) % 2 || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbpk_dx_h16: g or dx is not aligned to its element size");
    const int64_t need = nnc_cbpk_dx_h16_workspace_bytes(m, kdim, ncols, bits);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_dx_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK) return rc;
    PgPlan p = h16_dx_plan(m, kdim, ncols, bits, CB_PLAN_CUS);
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kPkNames, p.path, x_dtype, bits, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM) p = pg_dx_plan(m, kdim, ncols, bits, cu_count());      // (the row groups of this device)
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, pk, row_bytes, ncols, centers_dev, k, p.rows_per_group,
                   direct, out);
            LAUNCHCHK("k_cbpkdx_stream (h16)");
        } else {
            mc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, pk, row_bytes, ncols, centers_dev, k, p.col_tiles,
                   p.per_split, direct, out);
            LAUNCHCHK("k_cbpkdx_mfma");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbpk_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    if (pg_check("nnc_cbpk_dc_h16_workspace_bytes", m, kdim, ncols, bits, k) != NNC_OK) return 0;
    PgPlan p;
    if (h16_dc_plan(m, kdim, ncols, bits, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return h16_dc_ws_bytes(p.path, k);
}

extern "C" int nnc_cbpk_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbpk_dc_h16_plan";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    PgPlan p;
    if ((rc = h16_dc_plan(m, kdim, ncols, bits, k, std::max(cus, 1), p)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kPkNames, p.path, x_dtype, bits, mc)) != NNC_OK) return rc;
    const int64_t v[NNC_CBPKDC_H16_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.path == NNC_CBMM_ZERO ? 0 : p.copies, p.splits, p.per_split, p.lds, p.col_tiles,
                                                p.row_tiles, p.terms_log2, h16_dc_ws_bytes(p.path, k), x_dtype};
    for (int i = 0; i < NNC_CBPKDC_H16_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbpk_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                               int64_t ncols, int32_t k, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbpk_dc_h16";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbpk_dc_h16: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbpk_dc_h16: x or g is NULL");
    if (reinterpret_cast<uintptr_t>(x) % 2 || reinterpret_cast<uintptr_t>(g) % 2) return fail(NNC_EINVAL, "nnc_cbpk_dc_h16: x or g is not aligned to its element size");
    PgPlan p;
    if ((rc = h16_dc_plan(m, kdim, ncols, bits, k, CB_PLAN_CUS, p)) != NNC_OK) return rc;
    const int64_t need = h16_dc_ws_bytes(p.path, k);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_dc_h16_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kPkNames, p.path, x_dtype, bits, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM && (rc = pg_dc_plan(m, kdim, ncols, bits, k, cu_count(), p)) != NNC_OK) return rc;   // (the row groups of this device)
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, (int)k, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, pk, row_bytes, ncols, k, p.terms_log2,
                   p.rows_per_group, hdr, sums);
            LAUNCHCHK("k_cbpkdc_stream (h16)");
        } else {
            mc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, pk, row_bytes, ncols, k, p.terms_log2,
                   p.col_tiles, p.per_split, hdr, sums);
            LAUNCHCHK("k_cbpkdc_mfma");
        }
        return NNC_OK;
    });
}
