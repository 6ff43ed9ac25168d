// nnc_cbgrad_grouped_h16.hip -- the backward pass of the group-wise codebook matmul on bf16 / fp16 activations, byte indices
// (include/nnc_cbgrad_grouped_h16.h, nnc_cbmm_grouped_dx_h16 / nnc_cbmm_grouped_dc_h16).
// W_h[i, o] = the centre centers[i / group_rows][labels[i, o]] rounded to the type of g, exactly the grouped forward's; products
// are exact in float32, every sum is float32, dc is binned as section 12's exact integers into G x K bins.
//
// The plans are the ungrouped half ones at label_bytes 1 (section 12's stream plans; nnc_cbh16plan.hpp's tiles and splits with the
// byte form's table and bins at m > 16) plus the group fields, as section 19 took the float32 ones: the path, the tiles, the splits,
// the order of every sum and the shift S of the dc sums are those of nnc_cbmm_dx_h16 / nnc_cbmm_dc_h16 on the same shape.  The
// two main loops are the ungrouped kernels' (hm_accumulate, dcm_accumulate), the pick of a row's table or set tile_group_of
// (nnc_cbgrad_grouped.hpp).
//   m <= 16   k_cbdx_stream_grouped<XT> / k_cbdc_stream_grouped<XT> of nnc_cbgrad_grouped.hpp: section 19's kernels with g and x
//             widened as they are loaded and, for dx, the tables of the rounded centres.
//   k_cbdx_mfma_grouped  m > 16.  k_cbdx_mfma (nnc_cbgrad_h16.hip) with the tables of the up to four groups the tile's 128 index rows
//             lie in.  Thread t decodes index row n0 + (t mod 128) for the whole kernel, so it resolves its table once; the tables
//             do not change along the o loop.  The LDS is the ungrouped kernel's: the 1 << cshift copies of the 256-entry per-bank
//             table are divided among the tables (32, 16 or 8 copies each at 1, 2 or 4 tables).
//   k_cbdc_mfma_grouped  m > 16.  dcm_accumulate (nnc_cbgrad_h16.hpp) unchanged, then the epilogue of k_cbdc_mfma with one set of
//             bins per group of the tile: accumulator (a, b) of a wave holds the 32 aligned index rows m0 + wm + 32 a .., which lie
//             in one group (group_rows is a multiple of 32), so the set is a scalar taken from blockIdx, the arguments and the
//             wave number.  The plan's copies of a bin are cut into 1, 2 or 4 sets (the LDS of k_cbdc_mfma); one binning pass, one
//             cbdc_flush per set into sums + (q0 + t) * k.
// Everything past m, kdim, ncols and the end of a split is zero in the images, never memory; no load leaves the label buffer.
// k_cbgrad_absmax, k_cbgrad_reduce and k_cbdc_finish (over G * K bins) are nnc_cbgrad.hip's.
#include "nnc_cbdxm.hpp"
#include "nnc_cbgrad_grouped.hpp"
#include "nnc_cbgrad_h16.hpp"
#include "nnc_cbh16plan.hpp"

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads; `out` and cols_per_split as k_cbdx_mfma.  LDS: 1 << tlog2 tables
// of entries << (cshift - tlog2) words (table t that of group n0 / group_rows + t; entries past k are 0, so a label >= k reads 0),
// the staging row, the two images.
template <typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbdx_mfma_grouped(const XT *__restrict__ g, long long m, long long kdim, const uint8_t *__restrict__ labels,
                                                                  long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                                  int tlog2, long long col_tiles, long long cols_per_split, long long group_rows,
                                                                  int direct, void *__restrict__ out_)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    float *cb = hm_smem;                                // entries << cshift: the tables, one after the other
    float *stage = cb + (entries << cshift);            // entries
    XT *gs = reinterpret_cast<XT *>(hm_smem + hm_table_words(entries, cshift));   // [HM_BM][HM_LD]: g tile, row-major in o
    XT *ws = gs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: W^T tile, [i][o]

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);   // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const int tcs = cshift - tlog2, tables = 1 << tlog2;          // the copies of one table (log2)
    const TileGroups G = tile_groups_at(T.n0, kdim, group_rows);
    for (int t = 0; t < tables; ++t) {                  // (uniform over the workgroup; a table past the last group repeats it, unread)
        if (t) __syncthreads();                         // the staging row of the table before has been copied
        cb_fill<XT>(cb + (long long)t * (entries << tcs), stage, centers + std::min(G.q0 + t, G.groups - 1) * k, k, entries, tcs);
    }

    const long long gi = T.n0 + T.wc;
    const bool row_ok = gi < kdim;
    const uint8_t *lrow = labels + gi * ncols;
    const float *tab = cb + tile_group_of(G, gi, group_rows, tables) * (entries << tcs) + (T.lane & ((1 << tcs) - 1));
    uint32_t lw[4];

    auto load_w = [&](long long ob) {
        const long long left = T.k_hi - (ob + T.wk0);
        dxm_load_labels<uint8_t>(lrow + ob + T.wk0, row_ok ? (int)std::max(0LL, std::min(16LL, left)) : 0, lw);
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t l = (lw[j / 4] >> (8 * (j % 4))) & 0xFFu;
            w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? tab[l << tcs] : 0.0f;
        }
        hm_store_w(ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(g, m, ncols, T, gs, ws, acc, load_w, store_w);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads.  LDS: the two images, then the k << rlog2 int64 bins, cut into
// 1 << sets_log2 sets of k << (rlog2 - sets_log2), set t for group m0 / group_rows + t.
template <typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbdc_mfma_grouped(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                                  const uint8_t *__restrict__ labels, long long ncols, int k, int rlog2, int sets_log2,
                                                                  int terms_log2, long long col_tiles, long long rows_per_split, long long group_rows,
                                                                  uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
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

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col): its 32 rows lie in one group, whose set is a scalar
    const int rl = rlog2 - sets_log2, sets = 1 << sets_log2;
    const TileGroups G = tile_groups_at(T.m0, kdim, group_rows);
    const long long row0 = tile_wave_row0(T.m0);
    const int rep = T.t & ((1 << rl) - 1);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int set = (int)tile_group_of(G, row0 + a * 32, group_rows, sets);
        unsigned long long *sb = bins + ((long long)set * k << rl);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const long long o = hm_acc_col(T.n0 + T.wn, b, T.lane);
            if (o >= ncols) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = hm_acc_row(T.m0 + T.wm, a, r, T.lane);
                if (i >= kdim) continue;
                const uint32_t l = (uint32_t)labels[i * ncols + o];
                if (l < (uint32_t)k) atomicAdd(&sb[(l << rl) + rep], cbdc_fix(acc[a][b][r], Sw));
            }
        }
    }
    for (int t = 0; t < sets && G.q0 + t < G.groups; ++t) cbdc_flush(bins + ((long long)t * k << rl), k, rl, sums + (G.q0 + t) * k);
}

// ------------------------------------------------------------------ plans (host)
// nnc_cbmm_dx_h16's / nnc_cbmm_dc_h16's plans at label_bytes 1.  m <= 16 and the empty shapes: section 12's plans (dx_plan, dc_plan).
// m > 16: nnc_cbh16plan.hpp's tiles and splits with the LDS of k_cbdx_mfma / k_cbdc_mfma, which the tables / sets of a tile divide.
static CgPlan gh_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int32_t cus, uintptr_t labels)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return dx_plan(m, kdim, ncols, 1, k, cus, labels);
    int entries = 0, cshift = 0;   // (cb_table_shape counts cshift up from 0)
    cb_table_shape(1, k, entries, cshift);
    CgPlan p = h16_mfma_plan<CgPlan>(h16_dx_tiles(m, kdim, ncols), (long long)hm_table_words(entries, cshift) * 4);
    p.entries = entries, p.cshift = cshift;
    return p;
}

static CgPlan gh_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int32_t cus, uintptr_t labels)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return dc_plan(m, kdim, ncols, 1, k, cus, labels);
    CgPlan p = h16_mfma_plan<CgPlan>(h16_dc_tiles(m, kdim, ncols), ((long long)k << dc_rlog2(k)) * 8);
    p.rlog2 = dc_rlog2(k);
    return p;
}

// ------------------------------------------------------------------ launches
template <typename XT, int VB, int MT>
static void launch_dx_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const void *labels, long long ncols,
                             const float *centers, int k, int entries, int cshift, long long rpg, long long group_rows, int direct, void *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    const XT *gp = reinterpret_cast<const XT *>(g);
    if (aligned)
        hipLaunchKernelGGL((k_cbdx_stream_grouped<XT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, gp, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, group_rows, direct, out);
    else
        hipLaunchKernelGGL((k_cbdx_stream_grouped<XT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, gp, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, group_rows, direct, out);
}

template <typename XT, int VB, int MT>
static void launch_dc_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const void *labels,
                             long long ncols, int k, int rlog2, int tl, long long rpg, long long group_rows, uint32_t *hdr, unsigned long long *sums)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    const XT *xp = reinterpret_cast<const XT *>(x), *gp = reinterpret_cast<const XT *>(g);
    if (aligned)
        hipLaunchKernelGGL((k_cbdc_stream_grouped<XT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, xp, gp, m, kdim, lab, ncols, k, rlog2, tl, rpg, group_rows, hdr, sums);
    else
        hipLaunchKernelGGL((k_cbdc_stream_grouped<XT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, xp, gp, m, kdim, lab, ncols, k, rlog2, tl, rpg, group_rows, hdr, sums);
}

template <typename XT>
static void launch_dx_mfma(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const void *labels, long long ncols,
                           const float *centers, int k, int entries, int cshift, int tlog2, long long col_tiles, long long cps, long long group_rows, int direct,
                           void *out)
{
    hm_launch(g, ncols, k_cbdx_mfma_grouped<XT, true>, k_cbdx_mfma_grouped<XT, false>, grid, lds, s, reinterpret_cast<const XT *>(g), m, kdim,
              reinterpret_cast<const uint8_t *>(labels), ncols, centers, k, entries, cshift, tlog2, col_tiles, cps, group_rows, direct, out);
}

template <typename XT>
static void launch_dc_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const void *labels,
                           long long ncols, int k, int rlog2, int sets_log2, int tl, long long col_tiles, long long rps, long long group_rows, uint32_t *hdr,
                           unsigned long long *sums)
{
    hipLaunchKernelGGL((dcm_xvec(x, g, kdim, ncols) ? k_cbdc_mfma_grouped<XT, true> : k_cbdc_mfma_grouped<XT, false>), grid, dim3(HM_THREADS), lds, s,
                       reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim, reinterpret_cast<const uint8_t *>(labels), ncols, k, rlog2,
                       sets_log2, tl, col_tiles, rps, group_rows, hdr, sums);
}

// every kernel instantiation of this unit: per dtype the uint8 stream list of nnc_cbgrad.hpp (one shared case list), and the MFMA pair
using DxLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, int, long long, const void *, long long, const float *, int, int, int, long long,
                          long long, int, void *);
using DcLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, const void *, int, long long, const void *, long long, int, int, int, long long,
                          long long, uint32_t *, unsigned long long *);
using DxMfma = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const void *, long long, const float *, int, int, int, int, long long,
                        long long, long long, int, void *);
using DcMfma = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const void *, long long, int, int, int, int, long long,
                        long long, long long, uint32_t *, unsigned long long *);
struct GradCase {
    int a, vb, mt;            // a: 0 (uint8 labels only)
    DxLaunch dx;
    DcLaunch dc;
};
struct MfmaCase {
    int dt, a;                // a: 0 (uint8 labels only)
    DxMfma dx;
    DcMfma dc;
};
#define BF_CASE(VB, MT) {0, VB, MT, launch_dx_stream<bf16_t, VB, MT>, launch_dc_stream<bf16_t, VB, MT>},
#define HF_CASE(VB, MT) {0, VB, MT, launch_dx_stream<f16_t, VB, MT>, launch_dc_stream<f16_t, VB, MT>},
static const GradCase kBf16Cases[] = {CBG_U8_STREAM_CASES(BF_CASE)};
static const GradCase kF16Cases[] = {CBG_U8_STREAM_CASES(HF_CASE)};
#undef BF_CASE
#undef HF_CASE
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 0, launch_dx_mfma<bf16_t>, launch_dc_mfma<bf16_t>},
    {NNC_DT_F16, 0, launch_dx_mfma<f16_t>, launch_dc_mfma<f16_t>},
};
static const CbgCaseNames kGradNames = {true, nullptr, true};

// ------------------------------------------------------------------ C ABI
static int gh_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    const int rc = h16_check_dtype(fn, x_dtype);
    return rc != NNC_OK ? rc : gg_check(fn, m, kdim, ncols, k, group_rows);
}

// the group fields behind the record of the ungrouped half plan (`rec`: its NNC_CBDX_H16_PLAN_LEN = NNC_CBDC_H16_PLAN_LEN values)
static void gh_plan_tail(const CgPlan &p, int64_t kdim, int64_t group_rows, int64_t *out)
{
    const bool mfma = p.path == NNC_CBMM_MFMA;
    cbg_grouped_plan_tail(mfma ? NNC_CBMM_TILED : p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out);
    out[4] = mfma ? tile_groups(group_rows) : 0;
}

extern "C" int64_t nnc_cbmm_grouped_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols)
{
    return nnc_cbmm_dx_h16_workspace_bytes(m, kdim, ncols, 1);
}

extern "C" int nnc_cbmm_grouped_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus,
                                            uint64_t labels_addr, int64_t *out)
{
    const char *fn = "nnc_cbmm_grouped_dx_h16_plan";
    int rc = gh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, std::string(fn) + ": cus < 1");
    if (!out) return fail(NNC_EINVAL, std::string(fn) + ": out is NULL");
    const CgPlan p = gh_dx_plan(m, kdim, ncols, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, 0, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    if ((rc = nnc_cbmm_dx_h16_plan(x_dtype, m, kdim, ncols, 1, k, cus, labels_addr, out)) != NNC_OK) return rc;   // the shared fields: the ungrouped record
    gh_plan_tail(p, kdim, group_rows, out + NNC_CBDX_H16_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbmm_grouped_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int64_t ncols, const float *centers_dev,
                                       int32_t k, int64_t group_rows, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbmm_grouped_dx_h16";
    int rc = gh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_h16: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_h16: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_h16: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_h16: g or labels is NULL");
    if (reinterpret_cast<uintptr_t>(g) % 2 || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_h16: g or dx is not aligned to its element size");
    const int64_t need = nnc_cbmm_grouped_dx_h16_workspace_bytes(m, kdim, ncols);
    if ((rc = cb_check_workspace(fn, "nnc_cbmm_grouped_dx_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace not 4-byte aligned")) != NNC_OK) return rc;
    const CgPlan p = gh_dx_plan(m, kdim, ncols, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, 0, p.vb, p.mt, gc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kGradNames, p.path, x_dtype, 0, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dx(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, labels, ncols, centers_dev, k,
                   p.entries, p.cshift, p.rows_per_group, group_rows, direct, out);
            LAUNCHCHK("k_cbdx_stream_grouped (h16)");
        } else {
            mc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, labels, ncols, centers_dev, k,
                                  p.entries, p.cshift, __builtin_ctz(tile_groups(group_rows)), p.col_tiles, p.per_split, group_rows, direct, out);
            LAUNCHCHK("k_cbdx_mfma_grouped");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbmm_grouped_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (gg_check("nnc_cbmm_grouped_dc_h16_workspace_bytes", m, kdim, ncols, k, group_rows) != NNC_OK) return 0;
    return h16_dc_ws_bytes(dc_plan(m, kdim, ncols, 1, k, CB_PLAN_CUS, 0).path, gg_groups(kdim, group_rows) * k);
}

extern "C" int nnc_cbmm_grouped_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus,
                                            uint64_t labels_addr, int64_t *out)
{
    const char *fn = "nnc_cbmm_grouped_dc_h16_plan";
    int rc = gh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, std::string(fn) + ": cus < 1");
    if (!out) return fail(NNC_EINVAL, std::string(fn) + ": out is NULL");
    const CgPlan p = gh_dc_plan(m, kdim, ncols, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, 0, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    if ((rc = nnc_cbmm_dc_h16_plan(x_dtype, m, kdim, ncols, 1, k, cus, labels_addr, out)) != NNC_OK) return rc;   // the shared fields: the ungrouped record
    out[NNC_CBDC_P_WORKSPACE] = h16_dc_ws_bytes(p.path, gg_groups(kdim, group_rows) * k);                                            // (G * k bins)
    gh_plan_tail(p, kdim, group_rows, out + NNC_CBDC_H16_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbmm_grouped_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int64_t ncols, int32_t k,
                                       int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbmm_grouped_dc_h16";
    int rc = gh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dc_h16: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dc_h16: x, g or labels is NULL");
    if (reinterpret_cast<uintptr_t>(x) % 2 || reinterpret_cast<uintptr_t>(g) % 2)
        return fail(NNC_EINVAL, "nnc_cbmm_grouped_dc_h16: x or g is not aligned to its element size");
    const int64_t need = nnc_cbmm_grouped_dc_h16_workspace_bytes(m, kdim, ncols, k, group_rows);
    if ((rc = cb_check_workspace(fn, "nnc_cbmm_grouped_dc_h16_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    const CgPlan p = gh_dc_plan(m, kdim, ncols, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kGradNames, p.path, 0, p.vb, p.mt, gc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kGradNames, p.path, x_dtype, 0, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const int nbins = (int)(gg_groups(kdim, group_rows) * k);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dc(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, labels, ncols, k, p.rlog2,
                   p.terms_log2, p.rows_per_group, group_rows, hdr, sums);
            LAUNCHCHK("k_cbdc_stream_grouped (h16)");
        } else {
            mc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, labels, ncols, k, p.rlog2,
                                  __builtin_ctz(tile_groups(group_rows)), p.terms_log2, p.col_tiles, p.per_split, group_rows, hdr, sums);
            LAUNCHCHK("k_cbdc_mfma_grouped");
        }
        return NNC_OK;
    });
}
