// nnc_cbgrad_grouped.hip -- the backward pass of the group-wise codebook matmul (nnc_cbmm_grouped.hip) from the codebooks and the
// indices, W never decoded (include/nnc.h, nnc_cbmm_grouped_dx_f32 / nnc_cbmm_grouped_dc_f32).
// W[i, o] = c[i / group_rows][L[i, o]], uint8 labels, y = x @ W, g = dL/dy:
//
//   dx[r, i]  = sum_o g[r, o] * c[i / group_rows][L[i, o]]                          a row i of dx reads one table only
//   dc[q, k]  = sum_{(i, o): i / group_rows = q, L[i, o] = k} sum_r x[r, i] * g[r, o]   G x K bins
//
// The plans are the ungrouped ones (dx_plan, dc_plan of nnc_cbgrad.hpp at label_bytes 1), so the path, the grids, the splits, the
// order in which every sum is formed and the shift S of the dc sums are those of nnc_cbmm_dx_f32 / nnc_cbmm_dc_f32 on the same
// shape.  The kernels are the ungrouped ones (nnc_cbgrad.hip) with one addition each; they are kernels of their own for the reason
// nnc_cbmm_grouped.hip gives (a shared body changes the instruction streams of the old instantiations).
//   k_cbdx_stream_grouped  m <= 16.  k_cbdx_stream; the workgroup's label rows are walked group by group as k_cbmm_stream_grouped
//                          walks a split: each stretch is divided among the four waves, the table is rewritten between two barriers.
//   k_cbdx_tiled_grouped   m > 16.  k_cbdx_tiled; an output tile's 128 index rows lie in at most four groups, whose tables are
//                          loaded once (they do not change along the o loop); a thread decodes one row, so it keeps one table.
//   k_cbdc_stream_grouped  m <= 16.  k_cbdc_stream with the same walk; the LDS bins are one group's, flushed into sums + q * k and
//                          cleared at every boundary.
//   k_cbdc_tiled_grouped   m > 16.  k_cbdc_tiled; a wave's 32 index rows lie in one group (group_rows is a multiple of 32), so the
//                          LDS bins are cut into one set per group of the tile with the copies divided among the sets: the LDS
//                          and the lanes per copy of k_cbdc_tiled, one binning pass, one flush per set.
// The integer sums are exact, so neither walk changes a bit of dc; which wave takes a row changes no bit of dx.  Everything that
// steers a walk comes from blockIdx and the wave number (a scalar): every wave of a workgroup reaches every barrier.
// k_cbgrad_absmax, k_cbgrad_reduce and k_cbdc_finish (over G * K bins) are nnc_cbgrad.hip's.
// What the kernels share with the ungrouped ones without changing an instruction of either is written once (DESIGN.md section
// 21): the label row loads (cb_row_words) and the step to the next group's rows (cb_group_step) in nnc_cbmm.hpp, the x load of the
// dc kernel (cbdc_load_x) in nnc_cbgrad.hpp.  So is the host side: the sequences of HIP calls of the two entry points
// (cbg_run_dx, cbg_run_dc), the lookup in the table of stream instantiations, the list that table is made from, the plan checks
// and the tail of the plan record (nnc_cbgrad.hpp), the group_rows checks (cb_check_group_rows, nnc_cbmm.hpp).
// The two stream kernels and gg_check live in nnc_cbgrad_grouped.hpp, templated on the element type: this unit instantiates them for
// float32, nnc_cbgrad_grouped_h16.hip for bf16 / fp16.
#include "nnc_cbgrad_grouped.hpp"

// ------------------------------------------------------------------ dx, m > 16
// k_cbdx_tiled<uint8_t> with centers[groups][k]: the same grid, tile and FMA order.  LDS holds `tables` tables of k + 1 entries
// (entry k = 0), table t that of group n0 / group_rows + t; index row n0 + lr reads the one its group has.
__global__ __launch_bounds__(256) void k_cbdx_tiled_grouped(const float *__restrict__ g, long long m, long long kdim, const uint8_t *__restrict__ labels,
                                                            long long ncols, const float *__restrict__ centers, int k, long long col_tiles,
                                                            long long cols_per_split, long long group_rows, int tables, int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: W^T[o, n0 + i] = c[group of n0 + i][L[n0 + i, o]]
    float *cb = ws + TB_K * TB_N;          // [tables][k + 1]

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    const long long q0 = T.n0 / group_rows, groups = (kdim + group_rows - 1) / group_rows;
    for (int j = threadIdx.x; j < tables * (k + 1); j += 256) {
        const int t = j / (k + 1), e = j - t * (k + 1);
        cb[j] = (e < k && q0 + t < groups) ? centers[(q0 + t) * k + e] : 0.0f;
    }
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lo = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lo..lo+3 (as the g tile: row lr, o lo..lo+3)
    const long long wi = T.n0 + lr;
    const float *tab = cb + std::min((long long)tables - 1, wi / group_rows - q0) * (k + 1);
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long go = ob + lo + j;
            ws[(lo + j) * TB_N + lr] = (wi < kdim && go < T.hi) ? tab[std::min((uint32_t)labels[wi * ncols + go], (uint32_t)k)] : 0.0f;
        }
        __syncthreads();
        tb_tile_fma(gs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_dx(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, kdim, direct, out);
}

// ------------------------------------------------------------------ dc, m > 16
// k_cbdc_tiled<uint8_t> with sums[groups][k]: the same grid, tiles and FMA order.  The k << rlog2 LDS bins are cut into
// 1 << sets_log2 sets of k << (rlog2 - sets_log2), set t for group m0 / group_rows + t.  Thread (tx, ty) bins index rows
// m0 + ty * 8 .. + 7, which lie in one group, into that group's set; every set then goes into its group's sums.
__global__ __launch_bounds__(256) void k_cbdc_tiled_grouped(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                            const uint8_t *__restrict__ labels, long long ncols, int k, int rlog2, int sets_log2,
                                                            int terms_log2, long long col_tiles, long long rows_per_split, long long group_rows,
                                                            uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]: x[r, i0 + i]
    float *gs = xs + TB_K * TB_M;          // [TB_K][TB_N]: g[r, o0 + o]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + TB_K * TB_N);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, k << rlog2, scx, scg, Sw)) return;

    const TbTile T = tb_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i
    float acc[8][8];
    tb_clear(acc);
    for (long long rb = T.lo; rb < T.hi; rb += TB_K) {
        __syncthreads();
        cbdc_load_tiles(xs, gs, x, g, kdim, ncols, T.m0, T.n0, rb, T.hi, scx, scg);
        __syncthreads();
        tb_tile_fma(xs, gs, T.tx, T.ty, acc);
    }
    const int rl = rlog2 - sets_log2, sets = 1 << sets_log2;
    const long long q0 = T.m0 / group_rows, groups = (kdim + group_rows - 1) / group_rows;
    const int set = (int)std::min((long long)sets - 1, (T.m0 + T.ty * 8) / group_rows - q0);
    cbdc_bin_tile(acc, T, kdim, ncols, k, Sw, bins + ((long long)set * k << rl), rl, threadIdx.x & ((1 << rl) - 1),
                  [&](long long i, long long o) { return (uint32_t)labels[i * ncols + o]; });
    for (int t = 0; t < sets && q0 + t < groups; ++t) cbdc_flush(bins + ((long long)t * k << rl), k, rl, sums + (q0 + t) * k);
}

// ------------------------------------------------------------------ launches
template <int VB, int MT>
static void launch_dx_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const float *g, int m, long long kdim, const void *labels, long long ncols,
                             const float *centers, int k, int entries, int cshift, long long rpg, long long group_rows, int direct, float *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (aligned)
        hipLaunchKernelGGL((k_cbdx_stream_grouped<float, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, group_rows, direct, out);
    else
        hipLaunchKernelGGL((k_cbdx_stream_grouped<float, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, group_rows, direct, out);
}

template <int VB, int MT>
static void launch_dc_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const float *x, const float *g, int m, long long kdim, const void *labels,
                             long long ncols, int k, int rlog2, int tl, long long rpg, long long group_rows, uint32_t *hdr, unsigned long long *sums)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (aligned)
        hipLaunchKernelGGL((k_cbdc_stream_grouped<float, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, lab, ncols, k, rlog2, tl, rpg, group_rows, hdr, sums);
    else
        hipLaunchKernelGGL((k_cbdc_stream_grouped<float, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, lab, ncols, k, rlog2, tl, rpg, group_rows, hdr, sums);
}

// every stream instantiation of this unit: the uint8 list of nnc_cbgrad.hpp, which nnc_cbgrad.hip's table is made from too
using DxLaunch = void (*)(bool, dim3, size_t, hipStream_t, const float *, int, long long, const void *, long long, const float *, int, int, int, long long,
                          long long, int, float *);
using DcLaunch = void (*)(bool, dim3, size_t, hipStream_t, const float *, const float *, int, long long, const void *, long long, int, int, int, long long,
                          long long, uint32_t *, unsigned long long *);
struct GradCase {
    int a, vb, mt;            // a: 0 (uint8 labels only)
    DxLaunch dx;
    DcLaunch dc;
};
#define GRAD_CASE(VB, MT) {0, VB, MT, launch_dx_stream<VB, MT>, launch_dc_stream<VB, MT>},
static const GradCase kGradCases[] = {CBG_U8_STREAM_CASES(GRAD_CASE)};
#undef GRAD_CASE
static const CbgCaseNames kGradNames = {true, nullptr, true};

// ------------------------------------------------------------------ C ABI
extern "C" int64_t nnc_cbmm_grouped_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols)
{
    if (cg_check("nnc_cbmm_grouped_dx_workspace_bytes", m, kdim, ncols, 1, 1) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(dx_plan(m, kdim, ncols, 1, 1, CB_PLAN_CUS, 0).splits, m, kdim);
}

extern "C" int nnc_cbmm_grouped_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, uint64_t labels_addr,
                                        int64_t *out)
{
    int rc = gg_check("nnc_cbmm_grouped_dx_plan", m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    const CgPlan p = dx_plan(m, kdim, ncols, 1, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out("nnc_cbmm_grouped_dx_plan", kGradCases, kGradNames, p.path, 0, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const bool tiled = p.path == NNC_CBMM_TILED;
    const int tables = tile_groups(group_rows);
    const int64_t v[NNC_CBDX_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (tiled ? tables : 0), p.entries, p.splits,
                                          p.per_split, p.aligned, p.lds + (tiled ? (long long)(tables - 1) * (k + 1) * 4 : 0), p.col_tiles, p.row_tiles,
                                          cbg_dx_ws_bytes(p.splits, m, kdim)};
    for (int i = 0; i < NNC_CBDX_PLAN_LEN; ++i) out[i] = v[i];
    cbg_grouped_plan_tail(p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out + NNC_CBDX_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbmm_grouped_dx_f32(const float *g, int64_t m, int64_t kdim, const void *labels, int64_t ncols, const float *centers_dev, int32_t k,
                                       int64_t group_rows, float *dx, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = gg_check("nnc_cbmm_grouped_dx_f32", m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_f32: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_f32: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dx_f32: g or labels is NULL");
    const int64_t need = nnc_cbmm_grouped_dx_workspace_bytes(m, kdim, ncols);
    if ((rc = cb_check_workspace("nnc_cbmm_grouped_dx_f32", "nnc_cbmm_grouped_dx_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    const CgPlan p = dx_plan(m, kdim, ncols, 1, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case("nnc_cbmm_grouped_dx_f32", kGradCases, kGradNames, p.path, 0, p.vb, p.mt, gc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, workspace, s, [&](int direct, float *out) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dx(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, labels, ncols, centers_dev, k,
                   p.entries, p.cshift, p.rows_per_group, group_rows, direct, out);
            LAUNCHCHK("k_cbdx_stream_grouped");
        } else {
            const int tables = tile_groups(group_rows);
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            hipLaunchKernelGGL(k_cbdx_tiled_grouped, grid, dim3(256), (size_t)(p.lds + (long long)(tables - 1) * (k + 1) * 4), s, g, (long long)m,
                               (long long)kdim, reinterpret_cast<const uint8_t *>(labels), (long long)ncols, centers_dev, (int)k, p.col_tiles, p.per_split,
                               (long long)group_rows, tables, direct, out);
            LAUNCHCHK("k_cbdx_tiled_grouped");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbmm_grouped_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (gg_check("nnc_cbmm_grouped_dc_workspace_bytes", m, kdim, ncols, k, group_rows) != NNC_OK) return 0;
    return cbg_dc_ws_bytes(dc_plan(m, kdim, ncols, 1, k, CB_PLAN_CUS, 0).path, (int)(gg_groups(kdim, group_rows) * k));
}

extern "C" int nnc_cbmm_grouped_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, uint64_t labels_addr,
                                        int64_t *out)
{
    int rc = gg_check("nnc_cbmm_grouped_dc_plan", m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    const CgPlan p = dc_plan(m, kdim, ncols, 1, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out("nnc_cbmm_grouped_dc_plan", kGradCases, kGradNames, p.path, 0, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const int sets_log2 = p.path == NNC_CBMM_TILED ? __builtin_ctz(tile_groups(group_rows)) : 0;
    const int64_t v[NNC_CBDC_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_ZERO ? 0 : 1LL << (p.rlog2 - sets_log2), p.splits, p.per_split, p.aligned, p.lds,
                                          p.col_tiles, p.row_tiles, p.terms_log2, cbg_dc_ws_bytes(p.path, (int)(gg_groups(kdim, group_rows) * k))};
    for (int i = 0; i < NNC_CBDC_PLAN_LEN; ++i) out[i] = v[i];
    cbg_grouped_plan_tail(p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out + NNC_CBDC_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbmm_grouped_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *labels, int64_t ncols, int32_t k,
                                       int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = gg_check("nnc_cbmm_grouped_dc_f32", m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dc_f32: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_grouped_dc_f32: x, g or labels is NULL");
    const int64_t need = nnc_cbmm_grouped_dc_workspace_bytes(m, kdim, ncols, k, group_rows);
    if ((rc = cb_check_workspace("nnc_cbmm_grouped_dc_f32", "nnc_cbmm_grouped_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    const CgPlan p = dc_plan(m, kdim, ncols, 1, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case("nnc_cbmm_grouped_dc_f32", kGradCases, kGradNames, p.path, 0, p.vb, p.mt, gc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const int nbins = (int)(gg_groups(kdim, group_rows) * k);
    return cbg_run_dc(p.path, x, g, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dc(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, labels, ncols, k, p.rlog2,
                   p.terms_log2, p.rows_per_group, group_rows, hdr, sums);
            LAUNCHCHK("k_cbdc_stream_grouped");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            hipLaunchKernelGGL(k_cbdc_tiled_grouped, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim,
                               reinterpret_cast<const uint8_t *>(labels), (long long)ncols, (int)k, p.rlog2, __builtin_ctz(tile_groups(group_rows)), p.terms_log2,
                               p.col_tiles, p.per_split, (long long)group_rows, hdr, sums);
            LAUNCHCHK("k_cbdc_tiled_grouped");
        }
        return NNC_OK;
    });
}
