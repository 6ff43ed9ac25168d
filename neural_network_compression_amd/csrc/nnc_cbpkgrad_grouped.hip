// nnc_cbpkgrad_grouped.hip -- the backward pass of the group-wise codebook matmul on 2- and 4-bit packed indices (nnc_cbpk_grouped.hip)
// from the (G, K) codebooks and the packed buffer of the whole index matrix: the indices are never unpacked, W and dW never built
// (include/nnc_cbpkgrad_grouped.h, nnc_cbpk_grouped_dx_f32 / nnc_cbpk_grouped_dc_f32).
// W[i, o] = c[i / group_rows][L[i, o]], L read from the packed rows, y = x @ W, g = dL/dy:
//
//   dx[r, i]  = sum_o g[r, o] * c[i / group_rows][L[i, o]]       a label >= K reads 0; a column past ncols forms no product
//   dc[q, k]  = sum_{(i, o): i / group_rows = q, L[i, o] = k} sum_r x[r, i] * g[r, o]   G x K bins; a padding field falls into none
//
// The plans are the ungrouped packed ones (pg_dx_plan, pg_dc_plan of nnc_cbpkgrad.hpp), so the path, the grids, the splits, the
// order in which every sum is formed and the shift S of the dc sums are those of nnc_cbpk_dx_f32 / nnc_cbpk_dc_f32 on the same
// shape.  The kernels are the ungrouped ones (nnc_cbpkgrad.hip) with the walk through the groups added; they are kernels of their
// own for the reason nnc_cbmm_grouped.hip gives (a shared body changes the instruction streams of the old instantiations).
//   k_cbpkdx_stream_grouped  m <= 16.  k_cbpkdx_stream with the per-wave table of k_cbpk_stream_grouped: every wave walks its own
//                            rows in stretches cut at the group's end and rewrites its table from the centres its lanes hold,
//                            loaded while the stretch before ran.  No workgroup barrier.
//   k_cbpkdx_tiled_grouped   m > 16.  k_cbpkdx_tiled with the up to four tables of the groups a 128-row tile lies in, loaded
//                            once; a thread decodes one index row throughout, so it keeps a pointer to that row's table.
//   k_cbpkdc_stream_grouped  m <= 16.  k_cbpkdc_stream with the workgroup walk of k_cbdc_stream_grouped: the [K][64] bins are
//                            one group's, flushed into sums + q * K and cleared at every boundary.
//   k_cbpkdc_tiled_grouped   m > 16.  k_cbpkdc_tiled with the per-group sets of k_cbdc_tiled_grouped: a wave's 32 index rows lie
//                            in one group, one binning pass, one flush per set; LDS unchanged.
// The integer sums are exact, so neither walk changes a bit of dc; which wave takes a row changes no bit of dx.  Everything that
// steers a walk comes from blockIdx, the kernel arguments and the readfirstlane'd wave number: every wave of a workgroup reaches
// every barrier, and no cross-lane read sits in a lane-dependent branch.
// k_cbgrad_absmax, k_cbgrad_reduce and k_cbdc_finish (over G * K bins) are nnc_cbgrad.hip's.  No float atomics; no host read.
// What the kernels share with the other units without changing an instruction of any is written once: the
// step to the next group's rows (cb_group_step, nnc_cbmm.hpp) and the x load of the dc kernel (cbdc_load_x, nnc_cbgrad.hpp).  So
// is the host side: the sequences of HIP calls of the two entry points (cbg_run_dx, cbg_run_dc), the lookup in the table of
// stream instantiations, the plan checks and the tail of the plan record (nnc_cbgrad.hpp), the list that table is made from
// (nnc_cbpkgrad.hpp), the group_rows checks (cb_check_group_rows, nnc_cbmm.hpp).
// The two stream kernels and pgg_check live in nnc_cbpkgrad_grouped.hpp, templated on the element type: this unit instantiates them
// for float32, nnc_cbpkgrad_grouped_h16.hip for bf16 / fp16.
#include "nnc_cbpkgrad_grouped.hpp"

// ------------------------------------------------------------------ dx, m > 16
// k_cbpkdx_tiled with centers[groups][k]: the same grid, tile, decode and FMA order.  LDS holds `tables` tables of 2^BITS entries
// (zeros from k on), table t that of group n0 / group_rows + t; index row n0 + lr reads the one its group has.
template <int BITS>
__global__ __launch_bounds__(256) void k_cbpkdx_tiled_grouped(const float *__restrict__ g, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                              long long row_bytes, long long ncols, const float *__restrict__ centers, int k,
                                                              long long col_tiles, long long cols_per_split, long long group_rows, int tables, int direct,
                                                              float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: W^T[o, n0 + i] = c[group of n0 + i][L[n0 + i, o]]
    float *cb = ws + TB_K * TB_N;          // [tables][2^BITS]

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    const long long q0 = T.n0 / group_rows, groups = (kdim + group_rows - 1) / group_rows;
    for (int j = threadIdx.x; j < tables * ENTRIES; j += 256) {
        const int t = j / ENTRIES, e = j % ENTRIES;
        cb[j] = (e < k && q0 + t < groups) ? centers[(q0 + t) * k + e] : 0.0f;
    }
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lo = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lo..lo+3 (as the g tile: row lr, o lo..lo+3)
    const long long wi = T.n0 + lr;
    const float *tab = cb + std::min((long long)tables - 1, wi / group_rows - q0) * ENTRIES;
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
        const long long bitpos = (ob + lo) * BITS;
        const bool live = wi < kdim && ob + lo < T.hi;                 // then the dword lies inside the padded row
        const uint32_t word = live ? *reinterpret_cast<const uint32_t *>(packed + wi * row_bytes + ((bitpos >> 5) << 2)) >> (bitpos & 31) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[(lo + j) * TB_N + lr] = (live && ob + lo + j < T.hi) ? tab[(word >> (BITS * j)) & MASK] : 0.0f;
        __syncthreads();
        tb_tile_fma(gs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_dx(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, kdim, direct, out);
}

// ------------------------------------------------------------------ dc, m > 16
// k_cbpkdc_tiled with sums[groups][k]: the same grid, tiles and FMA order.  The k << PKG_RLOG2 LDS bins are cut into
// 1 << sets_log2 sets of k << (PKG_RLOG2 - sets_log2), set t for group m0 / group_rows + t.  Thread (tx, ty) bins index rows
// m0 + ty * 8 .. + 7, which lie in one group, into that group's set; every set then goes into its group's sums.
template <int BITS>
__global__ __launch_bounds__(256) void k_cbpkdc_tiled_grouped(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                              const unsigned char *__restrict__ packed, long long row_bytes, long long ncols, int k,
                                                              int sets_log2, int terms_log2, long long col_tiles, long long rows_per_split,
                                                              long long group_rows, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]: x[r, i0 + i]
    float *gs = xs + TB_K * TB_M;          // [TB_K][TB_N]: g[r, o0 + o]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + TB_K * TB_N);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, k << PKG_RLOG2, scx, scg, Sw)) return;

    const TbTile T = tb_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i
    float acc[8][8];
    tb_clear(acc);
    for (long long rb = T.lo; rb < T.hi; rb += TB_K) {
        __syncthreads();
        cbdc_load_tiles(xs, gs, x, g, kdim, ncols, T.m0, T.n0, rb, T.hi, scx, scg);
        __syncthreads();
        tb_tile_fma(xs, gs, T.tx, T.ty, acc);
    }
    const int rl = PKG_RLOG2 - sets_log2, sets = 1 << sets_log2;
    const long long q0 = T.m0 / group_rows, groups = (kdim + group_rows - 1) / group_rows;
    const int set = (int)std::min((long long)sets - 1, (T.m0 + T.ty * 8) / group_rows - q0);
    // the 8 labels of a thread's row are 8 * BITS bits of one packed dword (a tile starts on a multiple of 128 columns), which
    // lies inside the padded row when its first column lies inside the matrix
    cbdc_bin_tile(acc, T, kdim, ncols, k, Sw, bins + ((long long)set * k << rl), rl, threadIdx.x & ((1 << rl) - 1), [&](long long i, long long o) {
        const long long bitpos = (o & ~7LL) * BITS;
        const uint32_t word = *reinterpret_cast<const uint32_t *>(packed + i * row_bytes + ((bitpos >> 5) << 2)) >> (bitpos & 31);
        return (word >> (BITS * (o & 7))) & MASK;
    });
    for (int t = 0; t < sets && q0 + t < groups; ++t) cbdc_flush(bins + ((long long)t * k << rl), k, rl, sums + (q0 + t) * k);
}

// ------------------------------------------------------------------ launches
template <int BITS, int VB, int MT>
static void launch_pgg_dx(dim3 grid, size_t lds, hipStream_t s, const float *g, int m, long long kdim, const unsigned char *packed, long long row_bytes,
                          long long ncols, const float *centers, int k, long long rpg, long long group_rows, int direct, float *out)
{
    hipLaunchKernelGGL((k_cbpkdx_stream_grouped<float, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, packed, row_bytes, ncols, centers, k, rpg, group_rows,
                       direct, out);
}

template <int BITS, int VB, int MT>
static void launch_pgg_dc(dim3 grid, size_t lds, hipStream_t s, const float *x, const float *g, int m, long long kdim, const unsigned char *packed,
                          long long row_bytes, long long ncols, int k, int tl, long long rpg, long long group_rows, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbpkdc_stream_grouped<float, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, packed, row_bytes, ncols, k, tl, rpg, group_rows,
                       hdr, sums);
}

// every stream instantiation of this unit: the list of nnc_cbpkgrad.hpp, which nnc_cbpkgrad.hip's table is made from too
using PggDxLaunch = void (*)(dim3, size_t, hipStream_t, const float *, int, long long, const unsigned char *, long long, long long, const float *, int,
                             long long, long long, int, float *);
using PggDcLaunch = void (*)(dim3, size_t, hipStream_t, const float *, const float *, int, long long, const unsigned char *, long long, long long, int, int,
                             long long, long long, uint32_t *, unsigned long long *);
struct PggCase {
    int a, vb, mt;            // a: bits
    PggDxLaunch dx;
    PggDcLaunch dc;
};
#define PGG_CASE(B, V, M) {B, V, M, launch_pgg_dx<B, V, M>, launch_pgg_dc<B, V, M>},
static const PggCase kPggCases[] = {PKG_STREAM_CASES(PGG_CASE)};
#undef PGG_CASE
static const CbgCaseNames kPggNames = {true, "bits", true};

// ------------------------------------------------------------------ C ABI
// the dx LDS: one table per wave (stream), or the tile's images and one table per group of the tile (tiled)
static void pgg_dx_lds(PgPlan &p, long long group_rows, int &tables)
{
    tables = 0;
    if (p.path == NNC_CBMM_STREAM) {
        tables = CB_WAVES;
        p.lds = (long long)CB_WAVES * p.entries * PK_COPIES * 4;
    } else if (p.path == NNC_CBMM_TILED) {
        tables = tile_groups(group_rows);
        p.lds += (long long)(tables - 1) * p.entries * 4;
    }
}

extern "C" int64_t nnc_cbpk_grouped_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (pg_check("nnc_cbpk_grouped_dx_workspace_bytes", m, kdim, ncols, bits, 1) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(pg_dx_plan(m, kdim, ncols, bits, CB_PLAN_CUS).splits, m, kdim);
}

extern "C" int nnc_cbpk_grouped_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbpk_grouped_dx_plan";
    int rc = pgg_check(fn, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    PgPlan p = pg_dx_plan(m, kdim, ncols, bits, std::max(cus, 1));
    if ((rc = cbg_plan_out(fn, kPggCases, kPggNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    int tables;
    pgg_dx_lds(p, group_rows, tables);
    const int64_t v[NNC_CBPKDX_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.copies, p.entries, p.splits, p.per_split, p.lds, p.col_tiles, p.row_tiles,
                                            cbg_dx_ws_bytes(p.splits, m, kdim)};
    for (int i = 0; i < NNC_CBPKDX_PLAN_LEN; ++i) out[i] = v[i];
    cbg_grouped_plan_tail(p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out + NNC_CBPKDX_PLAN_LEN);
    out[NNC_CBPKDX_PLAN_LEN + 4] = tables;
    return NNC_OK;
}

extern "C" int nnc_cbpk_grouped_dx_f32(const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                                       const float *centers_dev, int32_t k, int64_t group_rows, float *dx, void *workspace, int64_t workspace_bytes,
                                       void *stream)
{
    const char *fn = "nnc_cbpk_grouped_dx_f32";
    int rc = pgg_check(fn, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_f32: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_f32: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_f32: g is NULL");
    const int64_t need = nnc_cbpk_grouped_dx_workspace_bytes(m, kdim, ncols, bits);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_grouped_dx_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK)
        return rc;
    PgPlan p = pg_dx_plan(m, kdim, ncols, bits, CB_PLAN_CUS);
    const PggCase *pc;
    if ((rc = cbg_stream_case(fn, kPggCases, kPggNames, p.path, bits, p.vb, p.mt, pc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path != NNC_CBMM_NONE) p = pg_dx_plan(m, kdim, ncols, bits, cu_count());        // (the row groups of this device)
    int tables;
    pgg_dx_lds(p, group_rows, tables);
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, workspace, s, [&](int direct, float *out) {
        if (p.path == NNC_CBMM_STREAM) {
            pc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, pk, row_bytes, ncols, centers_dev, k,
                   p.rows_per_group, group_rows, direct, out);
            LAUNCHCHK("k_cbpkdx_stream_grouped");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            if (bits == 4)
                hipLaunchKernelGGL(k_cbpkdx_tiled_grouped<4>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim, pk, row_bytes,
                                   (long long)ncols, centers_dev, (int)k, p.col_tiles, p.per_split, (long long)group_rows, tables, direct, out);
            else
                hipLaunchKernelGGL(k_cbpkdx_tiled_grouped<2>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim, pk, row_bytes,
                                   (long long)ncols, centers_dev, (int)k, p.col_tiles, p.per_split, (long long)group_rows, tables, direct, out);
            LAUNCHCHK("k_cbpkdx_tiled_grouped");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbpk_grouped_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows)
{
    if (pgg_check("nnc_cbpk_grouped_dc_workspace_bytes", m, kdim, ncols, bits, k, group_rows) != NNC_OK) return 0;
    PgPlan p;
    if (pg_dc_plan(m, kdim, ncols, bits, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return cbg_dc_ws_bytes(p.path, (int)(gg_groups(kdim, group_rows) * k));
}

extern "C" int nnc_cbpk_grouped_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbpk_grouped_dc_plan";
    int rc = pgg_check(fn, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    PgPlan p;
    if ((rc = pg_dc_plan(m, kdim, ncols, bits, k, std::max(cus, 1), p)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out(fn, kPggCases, kPggNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const bool tiled = p.path == NNC_CBMM_TILED;
    const int sets = tiled ? tile_groups(group_rows) : (p.path == NNC_CBMM_STREAM ? 1 : 0);
    const int64_t v[NNC_CBPKDC_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.path == NNC_CBMM_ZERO ? 0 : p.copies / std::max(sets, 1), p.splits, p.per_split,
                                            p.lds, p.col_tiles, p.row_tiles, p.terms_log2,
                                            cbg_dc_ws_bytes(p.path, (int)(gg_groups(kdim, group_rows) * k))};
    for (int i = 0; i < NNC_CBPKDC_PLAN_LEN; ++i) out[i] = v[i];
    cbg_grouped_plan_tail(p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out + NNC_CBPKDC_PLAN_LEN);
    out[NNC_CBPKDC_PLAN_LEN + 4] = sets;
    return NNC_OK;
}

extern "C" int nnc_cbpk_grouped_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                                       int64_t ncols, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes,
                                       void *stream)
{
    const char *fn = "nnc_cbpk_grouped_dc_f32";
    int rc = pgg_check(fn, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dc_f32: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dc_f32: x or g is NULL");
    PgPlan p;
    if ((rc = pg_dc_plan(m, kdim, ncols, bits, k, CB_PLAN_CUS, p)) != NNC_OK) return rc;
    const int nbins = (int)(gg_groups(kdim, group_rows) * k);
    const int64_t need = cbg_dc_ws_bytes(p.path, nbins);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_grouped_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK)
        return rc;
    const PggCase *pc;
    if ((rc = cbg_stream_case(fn, kPggCases, kPggNames, p.path, bits, p.vb, p.mt, pc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path != NNC_CBMM_ZERO && (rc = pg_dc_plan(m, kdim, ncols, bits, k, cu_count(), p)) != NNC_OK) return rc;   // (the row groups of this device)
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dc(p.path, x, g, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            pc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, pk, row_bytes, ncols, k, p.terms_log2,
                   p.rows_per_group, group_rows, hdr, sums);
            LAUNCHCHK("k_cbpkdc_stream_grouped");
        } else {
            const int sets_log2 = __builtin_ctz(tile_groups(group_rows));
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            if (bits == 4)
                hipLaunchKernelGGL(k_cbpkdc_tiled_grouped<4>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim, pk, row_bytes,
                                   (long long)ncols, (int)k, sets_log2, p.terms_log2, p.col_tiles, p.per_split, (long long)group_rows, hdr, sums);
            else
                hipLaunchKernelGGL(k_cbpkdc_tiled_grouped<2>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim, pk, row_bytes,
                                   (long long)ncols, (int)k, sets_log2, p.terms_log2, p.col_tiles, p.per_split, (long long)group_rows, hdr, sums);
            LAUNCHCHK("k_cbpkdc_tiled_grouped");
        }
        return NNC_OK;
    });
}
