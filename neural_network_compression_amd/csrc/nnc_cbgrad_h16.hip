// nnc_cbgrad_h16.hip -- the backward pass of nnc_cbmm_h16 (nnc_cbmm_h16.hip): the byte form of the indices on bf16 / fp16
// activations (include/nnc_cbgrad_h16.h, nnc_cbmm_dx_h16 / nnc_cbmm_dc_h16).  W_h[i, o] = the centre of
// labels[i, o] rounded to the type of g, exactly the forward's; a product of two bf16 or two fp16 values is exact in float32,
// every sum is float32, dc is binned as section 12's exact integers.
//
//   m <= 16   k_cbdx_stream<XT> / k_cbdc_stream<XT> of nnc_cbgrad.hpp: section 12's stream plan and kernels with g and x widened
//             as they are loaded and, for dx, the table of the rounded centres.  Bit for bit the float32 entry points on the
//             widened inputs.
//   k_cbdx_mfma  m > 16.  128 (r) x 128 (i) tiles of dx on nnc_cbmfma.hpp's tile: the A operand is g (row-major in the reduction
//             index o: hm_load_x / hm_store_x with ncols as the row length), the B operand W^T: thread t owns index row
//             n0 + (t mod 128) and 16 consecutive o of the step, which lie one after the other in memory (loaded as wide as the
//             address allows: 16 bytes, 4 bytes, or label by label), looks them up in the per-bank table and writes them with
//             hm_store_w -- the [i][o] image has o contiguous, no transpose.  ncols is split by section 16's rule.
//   k_cbdc_mfma  m > 16.  128 (i) x 128 (o) tiles of dW = x^T g, the reduction over r in steps of HM_BK, m split by the same rule.
//             Both operands arrive row-major in the wrong index, so both go through a transposing LDS store into [i][r] / [o][r]
//             images with r contiguous, the forward's W image: a thread owns one column and 16 rows of the step (2-byte loads,
//             coalesced over the wave, two 16-byte LDS stores: hm_store_w), or, XVEC, two columns and 8 rows (4-byte loads).
//             bf16 operands are scaled by section 12's powers of two as they are staged (rn_bf16(ldexpf(float(v), sc)): exact
//             for every element whose scaled value is a normal bf16); fp16 operands are not scaled.  The epilogue bins the
//             accumulators: cbdc_fix, the 64-bit LDS atomicAdd into the replicated bins, cbdc_flush.
// Everything past m, kdim, ncols and the end of a split is zero in both images, never memory.  No float atomics; no host read.
// The two main loops are shared with the other four half backward units (section 27): hm_accumulate (nnc_cbmfma.hpp) around this
// form's label load and lookup, dcm_accumulate (nnc_cbgrad_h16.hpp) in front of this form's epilogue; the tiles and splits of the
// MFMA plan and the half glue of the entry points are nnc_cbh16plan.hpp's.
#include "nnc_cbdxm.hpp"
#include "nnc_cbgrad_h16.hpp"
#include "nnc_cbh16plan.hpp"

// ------------------------------------------------------------------ dx, m > 16
// (the main loop, hm_accumulate, is the tile's, nnc_cbmfma.hpp; the label load, dxm_load_labels, is nnc_cbdxm.hpp's)
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads.  `out` is dx (direct 1: float32, 2: XT) or the float32 partials
// [split][m][kdim] (direct 0).  cols_per_split is a multiple of HM_BK.
template <typename XT, typename LT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbdx_mfma(const XT *__restrict__ g, long long m, long long kdim, const LT *__restrict__ labels,
                                                          long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                          long long col_tiles, long long cols_per_split, int direct, void *__restrict__ out_)
{
    constexpr int LB = sizeof(LT), PER = 4 / LB;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    float *cb = hm_smem;                                // entries << cshift
    float *stage = cb + (entries << cshift);            // entries
    XT *gs = reinterpret_cast<XT *>(hm_smem + hm_table_words(entries, cshift));   // [HM_BM][HM_LD]: g tile, row-major in o
    XT *ws = gs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: W^T tile, [i][o]
    cb_fill<XT>(cb, stage, centers, k, entries, cshift);

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);   // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const long long gi = T.n0 + T.wc;
    const bool row_ok = gi < kdim;
    const LT *lrow = labels + gi * ncols;
    uint32_t lw[4 * LB];

    auto load_w = [&](long long ob) {
        const long long left = T.k_hi - (ob + T.wk0);
        dxm_load_labels<LT>(lrow + ob + T.wk0, row_ok ? (int)std::max(0LL, std::min(16LL, left)) : 0, lw);
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t l = (lw[j / PER] >> (8 * LB * (j % PER))) & (LB == 1 ? 0xFFu : 0xFFFFu);
            w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? cb[CbTable<LT>::index(l, k, cshift, T.lane)] : 0.0f;
        }
        hm_store_w(ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(g, m, ncols, T, gs, ws, acc, load_w, store_w);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads.  LDS: the two images, then the bins [k][1 << rlog2] int64.
// rows_per_split is a multiple of HM_BK.  XVEC: x and g 4-byte aligned, kdim and ncols even.
template <typename XT, typename LT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbdc_mfma(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                          const LT *__restrict__ labels, long long ncols, int k, int rlog2, int terms_log2,
                                                          long long col_tiles, long long rows_per_split, uint32_t *__restrict__ hdr,
                                                          unsigned long long *__restrict__ sums)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    XT *xs = reinterpret_cast<XT *>(hm_smem);           // [HM_BM][HM_LD]: x^T tile, [i][r]
    XT *gs = xs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: g^T tile, [o][r]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + HM_BN * HM_LD);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, k << rlog2, scx, scg, Sw)) return;   // (uniform over the launch)
    dcm_scales<XT>(scx, scg, Sw);

    const HmTile T = hm_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i, [k_lo, k_hi): rows r
    typename HFrag<XT>::C acc[2][2];
    dcm_accumulate<XT, XVEC>(x, g, kdim, ncols, T, scx, scg, xs, gs, acc);

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col); the label loads are coalesced over the 32 lanes of a row
    const int rep = T.t & ((1 << rlog2) - 1);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const long long o = hm_acc_col(T.n0 + T.wn, b, T.lane);
            if (o >= ncols) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = hm_acc_row(T.m0 + T.wm, a, r, T.lane);
                if (i >= kdim) continue;
                const uint32_t l = (uint32_t)labels[i * ncols + o];
                if (l < (uint32_t)k) atomicAdd(&bins[(l << rlog2) + rep], cbdc_fix(acc[a][b][r], Sw));
            }
        }
    }
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ plans (host)
// m <= 16 and the empty shapes: section 12's plans (dx_plan, dc_plan) field for field.  m > 16: nnc_cbh16plan.hpp's tiles and splits
// with the per-bank table of k_cbmm_mfma (dx) or the replicated bins (dc).
static CgPlan dx_plan_h16(long long m, long long kdim, long long ncols, int lb, int k, int cus, uintptr_t labels)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return dx_plan(m, kdim, ncols, lb, k, cus, labels);
    int entries = 0, cshift = 0;   // (cb_table_shape counts cshift up from 0)
    cb_table_shape(lb, k, entries, cshift);
    CgPlan p = h16_mfma_plan<CgPlan>(h16_dx_tiles(m, kdim, ncols), (long long)hm_table_words(entries, cshift) * 4);
    p.entries = entries, p.cshift = cshift;
    return p;
}

static CgPlan dc_plan_h16(long long m, long long kdim, long long ncols, int lb, int k, int cus, uintptr_t labels)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return dc_plan(m, kdim, ncols, lb, k, cus, labels);
    CgPlan p = h16_mfma_plan<CgPlan>(h16_dc_tiles(m, kdim, ncols), ((long long)k << dc_rlog2(k)) * 8);
    p.rlog2 = dc_rlog2(k);
    return p;
}

// ------------------------------------------------------------------ launches
template <typename XT, typename LT, int VB, int MT>
static void launch_dx_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const void *labels, long long ncols,
                             const float *centers, int k, int entries, int cshift, long long rpg, int direct, void *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    const XT *gp = reinterpret_cast<const XT *>(g);
    if (aligned)
        hipLaunchKernelGGL((k_cbdx_stream<XT, LT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, gp, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, direct, out);
    else
        hipLaunchKernelGGL((k_cbdx_stream<XT, LT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, gp, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, direct, out);
}

template <typename XT, typename LT, int VB, int MT>
static void launch_dc_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const void *labels,
                             long long ncols, int k, int rlog2, int tl, long long rpg, uint32_t *hdr, unsigned long long *sums)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    const XT *xp = reinterpret_cast<const XT *>(x), *gp = reinterpret_cast<const XT *>(g);
    if (aligned)
        hipLaunchKernelGGL((k_cbdc_stream<XT, LT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, xp, gp, m, kdim, lab, ncols, k, rlog2, tl, rpg, hdr, sums);
    else
        hipLaunchKernelGGL((k_cbdc_stream<XT, LT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, xp, gp, m, kdim, lab, ncols, k, rlog2, tl, rpg, hdr, sums);
}

template <typename XT, typename LT>
static void launch_dx_mfma(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const void *labels, long long ncols,
                           const float *centers, int k, int entries, int cshift, long long col_tiles, long long cps, int direct, void *out)
{
    hm_launch(g, ncols, k_cbdx_mfma<XT, LT, true>, k_cbdx_mfma<XT, LT, false>, grid, lds, s, reinterpret_cast<const XT *>(g), m, kdim,
              reinterpret_cast<const LT *>(labels), ncols, centers, k, entries, cshift, col_tiles, cps, direct, out);
}

template <typename XT, typename LT>
static void launch_dc_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const void *labels,
                           long long ncols, int k, int rlog2, int tl, long long col_tiles, long long rps, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((dcm_xvec(x, g, kdim, ncols) ? k_cbdc_mfma<XT, LT, true> : k_cbdc_mfma<XT, LT, false>), grid, dim3(HM_THREADS), lds, s, reinterpret_cast<const XT *>(x),
                       reinterpret_cast<const XT *>(g), m, kdim, reinterpret_cast<const LT *>(labels), ncols, k, rlog2, tl, col_tiles, rps, hdr, sums);
}

// every kernel instantiation of this unit, a table of the stream ones (the lists of nnc_cbgrad.hpp) per dtype; the plans are checked
// against these tables, and the launches go through them
using DxLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, int, long long, const void *, long long, const float *, int, int, int, long long,
                          int, void *);
using DcLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, const void *, int, long long, const void *, long long, int, int, int, long long,
                          uint32_t *, unsigned long long *);
using DxMfma = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const void *, long long, const float *, int, int, int, long long,
                        long long, int, void *);
using DcMfma = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const void *, long long, int, int, int, long long,
                        long long, uint32_t *, unsigned long long *);
struct GradCase {
    int a, vb, mt;            // a: label_bytes
    DxLaunch dx;
    DcLaunch dc;
};
struct MfmaCase {
    int dt, a;                // a: label_bytes
    DxMfma dx;
    DcMfma dc;
};
#define BF_U8(VB, MT) {1, VB, MT, launch_dx_stream<bf16_t, uint8_t, VB, MT>, launch_dc_stream<bf16_t, uint8_t, VB, MT>},
#define BF_U16(VB, MT) {2, VB, MT, launch_dx_stream<bf16_t, uint16_t, VB, MT>, launch_dc_stream<bf16_t, uint16_t, VB, MT>},
#define HF_U8(VB, MT) {1, VB, MT, launch_dx_stream<f16_t, uint8_t, VB, MT>, launch_dc_stream<f16_t, uint8_t, VB, MT>},
#define HF_U16(VB, MT) {2, VB, MT, launch_dx_stream<f16_t, uint16_t, VB, MT>, launch_dc_stream<f16_t, uint16_t, VB, MT>},
static const GradCase kBf16Cases[] = {CBG_U8_STREAM_CASES(BF_U8) CBG_U16_STREAM_CASES(BF_U16)};
static const GradCase kF16Cases[] = {CBG_U8_STREAM_CASES(HF_U8) CBG_U16_STREAM_CASES(HF_U16)};
#undef BF_U8
#undef BF_U16
#undef HF_U8
#undef HF_U16
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 1, launch_dx_mfma<bf16_t, uint8_t>, launch_dc_mfma<bf16_t, uint8_t>}, {NNC_DT_BF16, 2, launch_dx_mfma<bf16_t, uint16_t>, launch_dc_mfma<bf16_t, uint16_t>},
    {NNC_DT_F16, 1, launch_dx_mfma<f16_t, uint8_t>, launch_dc_mfma<f16_t, uint8_t>},   {NNC_DT_F16, 2, launch_dx_mfma<f16_t, uint16_t>, launch_dc_mfma<f16_t, uint16_t>},
};
static const CbgCaseNames kGradNames = {false, "label_bytes", true};

// ------------------------------------------------------------------ C ABI
static int h16_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    const int rc = h16_check_dtype(fn, x_dtype);
    return rc != NNC_OK ? rc : cg_check(fn, m, kdim, ncols, label_bytes, k);
}

extern "C" int64_t nnc_cbmm_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (cg_check("nnc_cbmm_dx_h16_workspace_bytes", m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(dx_plan_h16(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS, 0).splits, m, kdim);
}

extern "C" int nnc_cbmm_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr,
                                    int64_t *out)
{
    int rc = h16_check("nnc_cbmm_dx_h16_plan", x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    const CgPlan p = dx_plan_h16(m, kdim, ncols, label_bytes, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out("nnc_cbmm_dx_h16_plan", h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, label_bytes, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case("nnc_cbmm_dx_h16_plan", kMfmaCases, kGradNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    const int64_t v[NNC_CBDX_H16_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_STREAM || p.path == NNC_CBMM_MFMA ? 1LL << p.cshift : 0, p.entries,
                                              p.splits, p.per_split, p.aligned, p.lds, p.col_tiles, p.row_tiles, cbg_dx_ws_bytes(p.splits, m, kdim), x_dtype};
    for (int i = 0; i < NNC_CBDX_H16_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols,
                               const float *centers_dev, int32_t k, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbmm_dx_h16";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbmm_dx_h16: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbmm_dx_h16: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbmm_dx_h16: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_dx_h16: g or labels is NULL");
    if (reinterpret_cast<uintptr_t>(g) % 2 || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbmm_dx_h16: g or dx is not aligned to its element size");
    if (label_bytes == 2 && reinterpret_cast<uintptr_t>(labels) % 2) return fail(NNC_EINVAL, "nnc_cbmm_dx_h16: 2-byte labels on an odd address");
    const int64_t need = nnc_cbmm_dx_h16_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace(fn, "nnc_cbmm_dx_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace not 4-byte aligned")) != NNC_OK) return rc;
    const CgPlan p = dx_plan_h16(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, label_bytes, p.vb, p.mt, gc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kGradNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dx(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, labels, ncols, centers_dev, k,
                   p.entries, p.cshift, p.rows_per_group, direct, out);
            LAUNCHCHK("k_cbdx_stream (h16)");
        } else {
            mc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, labels, ncols, centers_dev, k, p.entries,
                   p.cshift, p.col_tiles, p.per_split, direct, out);
            LAUNCHCHK("k_cbdx_mfma");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbmm_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (cg_check("nnc_cbmm_dc_h16_workspace_bytes", m, kdim, ncols, label_bytes, k) != NNC_OK) return 0;
    return h16_dc_ws_bytes(dc_plan_h16(m, kdim, ncols, label_bytes, k, CB_PLAN_CUS, 0).path, k);
}

extern "C" int nnc_cbmm_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr,
                                    int64_t *out)
{
    int rc = h16_check("nnc_cbmm_dc_h16_plan", x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    const CgPlan p = dc_plan_h16(m, kdim, ncols, label_bytes, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out("nnc_cbmm_dc_h16_plan", h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, label_bytes, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case("nnc_cbmm_dc_h16_plan", kMfmaCases, kGradNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    const int64_t v[NNC_CBDC_H16_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_ZERO ? 0 : 1LL << p.rlog2, p.splits, p.per_split, p.aligned, p.lds,
                                              p.col_tiles, p.row_tiles, p.terms_log2, h16_dc_ws_bytes(p.path, k), x_dtype};
    for (int i = 0; i < NNC_CBDC_H16_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols,
                               int32_t k, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbmm_dc_h16";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbmm_dc_h16: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_dc_h16: x, g or labels is NULL");
    if (reinterpret_cast<uintptr_t>(x) % 2 || reinterpret_cast<uintptr_t>(g) % 2) return fail(NNC_EINVAL, "nnc_cbmm_dc_h16: x or g is not aligned to its element size");
    if (label_bytes == 2 && reinterpret_cast<uintptr_t>(labels) % 2) return fail(NNC_EINVAL, "nnc_cbmm_dc_h16: 2-byte labels on an odd address");
    const int64_t need = nnc_cbmm_dc_h16_workspace_bytes(m, kdim, ncols, label_bytes, k);
    if ((rc = cb_check_workspace(fn, "nnc_cbmm_dc_h16_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    const CgPlan p = dc_plan_h16(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, label_bytes, p.vb, p.mt, gc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kGradNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, (int)k, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dc(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, labels, ncols, k, p.rlog2,
                   p.terms_log2, p.rows_per_group, hdr, sums);
            LAUNCHCHK("k_cbdc_stream (h16)");
        } else {
            mc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, labels, ncols, k, p.rlog2, p.terms_log2,
                   p.col_tiles, p.per_split, hdr, sums);
            LAUNCHCHK("k_cbdc_mfma");
        }
        return NNC_OK;
    });
}
