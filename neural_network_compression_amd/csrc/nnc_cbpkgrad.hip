// nnc_cbpkgrad.hip -- the backward pass of the 2- and 4-bit packed codebook matmul (nnc_cbpk.hip) from the packed indices: they
// are never unpacked and W is never decoded (include/nnc.h, nnc_cbpk_dx_f32 / nnc_cbpk_dc_f32).  With
// W[i, o] = c[L[i, o]] (a label >= K reads 0), y = x @ W and g = dL/dy:
//
//   dx[r, i] = sum_o g[r, o] * c[L[i, o]]     the conventions of nnc_cbmm_dx_f32: a label >= K reads 0, a column past ncols forms no
//                                             product (the padding fields hold label 0 and meet a 0, never g)
//   dc[k]    = nnc_cbmm_dc_f32 on the unpacked labels, bit for bit: every dW[i, o] is formed in float32 as k_cbdc_stream /
//              k_cbdc_tiled form it (from x and g scaled by the same powers of two, r ascending) and binned as rint(dW * 2^S)
//              with the same S (the same splits of m and T).  Integer sums do not depend on order.  A label >= K falls into no
//              bin; a padding field is never binned.
//
//   k_cbpkdx_stream  m <= 16.  A workgroup owns 64 lanes x E columns of g (E = 8 * VB / BITS, held in registers) and a group of
//                    packed rows; a wave takes one row at a time (CB_UNROLL rows in flight, k_cbpk_stream's aligned 1- to 16-byte
//                    loads), looks its columns up in the 2^BITS-entry per-bank table and reduces its m partials over the 64 lanes
//                    in a fixed order (wave_reduce_rows).  Column blocks are the splits, summed in block order by k_cbgrad_reduce.
//   k_cbpkdx_tiled   m > 16.  k_cbdx_tiled with the W^T tile decoded from packed dwords: all 256 threads decode 4 columns each.
//                    Both tiled kernels are the tile skeleton of nnc_cbtile.hpp around their label reads.
//   k_cbpkdc_stream  m <= 16.  The grid and loads of k_cbpkdx_stream; x[r, i] by vector load + v_readlane; dW'[i, o] as
//                    k_cbdc_stream forms it; the image goes into the lane's own copy of the K <= 16 LDS bins (64 copies: no two
//                    lanes of a wave ever meet on an address).
//   k_cbpkdc_tiled   m > 16.  k_cbdc_tiled's tiles and splits of m; a thread's 8 consecutive columns of a row come from one packed
//                    dword, loaded once.
// k_cbgrad_absmax, k_cbdc_finish and k_cbgrad_reduce are nnc_cbgrad.hip's.  No float atomics; no host read.
// The sequences of HIP calls of the two entry points (cbg_run_dx, cbg_run_dc), the lookup in the table of stream instantiations and
// the x load of k_cbpkdc_stream (cbdc_load_x) are nnc_cbgrad.hpp's; the list the table is made from is nnc_cbpkgrad.hpp's, and so
// are the two stream kernels, templates on the element type that this unit instantiates for float32 and nnc_cbpk_h16.hip for
// bf16 / fp16.
#include "nnc_cbpkgrad.hpp"

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), 256 threads; thread (tx, ty) owns rows ty*8.. (of g) and columns tx*8.. (i) of the
// tile.  Thread t decodes columns ob + (t & 1) * 4 .. + 3 of index row n0 + t / 2 from the dword that holds them (a split starts on a
// multiple of 16 columns, so the 4 fields never straddle two dwords); the two threads of a row load the same address.
template <int BITS>
__global__ __launch_bounds__(256) void k_cbpkdx_tiled(const float *__restrict__ g, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                      long long row_bytes, long long ncols, const float *__restrict__ centers, int k, long long col_tiles,
                                                      long long cols_per_split, int direct, float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: W^T[o, n0 + i] = c[L[n0 + i, o]]
    float *cb = ws + TB_K * TB_N;          // 2^BITS entries (zeros from k on)
    for (int j = threadIdx.x; j < ENTRIES; j += 256) cb[j] = j < k ? centers[j] : 0.0f;

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lo = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lo..lo+3 (as the g tile: row lr, o lo..lo+3)
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
        const long long wi = T.n0 + lr;
        const long long bitpos = (ob + lo) * BITS;
        const bool live = wi < kdim && ob + lo < T.hi;                 // then the dword lies inside the padded row
        const uint32_t word = live ? *reinterpret_cast<const uint32_t *>(packed + wi * row_bytes + ((bitpos >> 5) << 2)) >> (bitpos & 31) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[(lo + j) * TB_N + lr] = (live && ob + lo + j < T.hi) ? cb[(word >> (BITS * j)) & MASK] : 0.0f;
        __syncthreads();
        tb_tile_fma(gs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_dx(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, kdim, direct, out);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), 256 threads; thread (tx, ty) forms dW for index rows ty*8.. and columns tx*8.. of the
// 128 x 128 tile over its split's rows of m, then bins the 64 values: the 8 labels of a row are 8 * BITS bits of one packed dword
// (a tile starts on a multiple of 128 columns).
template <int BITS>
__global__ __launch_bounds__(256) void k_cbpkdc_tiled(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                      const unsigned char *__restrict__ packed, long long row_bytes, long long ncols, int k, int terms_log2,
                                                      long long col_tiles, long long rows_per_split, uint32_t *__restrict__ hdr,
                                                      unsigned long long *__restrict__ sums)
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
    // the 8 labels of a thread's row are 8 * BITS bits of one packed dword (a tile starts on a multiple of 128 columns), which
    // lies inside the padded row when its first column lies inside the matrix
    cbdc_bin_tile(acc, T, kdim, ncols, k, Sw, bins, PKG_RLOG2, threadIdx.x & ((1 << PKG_RLOG2) - 1), [&](long long i, long long o) {
        const long long bitpos = (o & ~7LL) * BITS;
        const uint32_t word = *reinterpret_cast<const uint32_t *>(packed + i * row_bytes + ((bitpos >> 5) << 2)) >> (bitpos & 31);
        return (word >> (BITS * (o & 7))) & MASK;
    });
    cbdc_flush(bins, k, PKG_RLOG2, sums);
}

// ------------------------------------------------------------------ C ABI
template <int BITS, int VB, int MT>
static void launch_pg_dx(dim3 grid, size_t lds, hipStream_t s, const float *g, int m, long long kdim, const unsigned char *packed, long long row_bytes,
                         long long ncols, const float *centers, int k, long long rpg, int direct, float *out)
{
    hipLaunchKernelGGL((k_cbpkdx_stream<float, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, packed, row_bytes, ncols, centers, k, rpg, direct,
                       static_cast<void *>(out));
}

template <int BITS, int VB, int MT>
static void launch_pg_dc(dim3 grid, size_t lds, hipStream_t s, const float *x, const float *g, int m, long long kdim, const unsigned char *packed,
                         long long row_bytes, long long ncols, int k, int tl, long long rpg, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbpkdc_stream<float, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, packed, row_bytes, ncols, k, tl, rpg, hdr, sums);
}

// every stream instantiation there is (the list of nnc_cbpkgrad.hpp); the plans are checked against this table, and the launches go through it
using PgDxLaunch = void (*)(dim3, size_t, hipStream_t, const float *, int, long long, const unsigned char *, long long, long long, const float *, int,
                            long long, int, float *);
using PgDcLaunch = void (*)(dim3, size_t, hipStream_t, const float *, const float *, int, long long, const unsigned char *, long long, long long, int, int,
                            long long, uint32_t *, unsigned long long *);
struct PgCase {
    int a, vb, mt;            // a: bits
    PgDxLaunch dx;
    PgDcLaunch dc;
};
#define PG_CASE(B, V, M) {B, V, M, launch_pg_dx<B, V, M>, launch_pg_dc<B, V, M>},
static const PgCase kPgCases[] = {PKG_STREAM_CASES(PG_CASE)};
#undef PG_CASE
static const CbgCaseNames kPgNames = {false, "bits", true};

extern "C" int64_t nnc_cbpk_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (pg_check("nnc_cbpk_dx_workspace_bytes", m, kdim, ncols, bits, 1) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(pg_dx_plan(m, kdim, ncols, bits, CB_PLAN_CUS).splits, m, kdim);
}

extern "C" int nnc_cbpk_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    int rc = pg_check("nnc_cbpk_dx_plan", m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    const PgPlan p = pg_dx_plan(m, kdim, ncols, bits, std::max(cus, 1));
    if ((rc = cbg_plan_out("nnc_cbpk_dx_plan", kPgCases, kPgNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const int64_t v[NNC_CBPKDX_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.copies, p.entries, p.splits, p.per_split, p.lds, p.col_tiles, p.row_tiles,
                                            cbg_dx_ws_bytes(p.splits, m, kdim)};
    for (int i = 0; i < NNC_CBPKDX_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbpk_dx_f32(const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                               const float *centers_dev, int32_t k, float *dx, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbpk_dx_f32";
    int rc = pg_check(fn, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbpk_dx_f32: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbpk_dx_f32: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbpk_dx_f32: g is NULL");
    const int64_t need = nnc_cbpk_dx_workspace_bytes(m, kdim, ncols, bits);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_dx_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK) return rc;
    PgPlan p = pg_dx_plan(m, kdim, ncols, bits, CB_PLAN_CUS);
    const PgCase *pc;
    if ((rc = cbg_stream_case(fn, kPgCases, kPgNames, p.path, bits, p.vb, p.mt, pc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path != NNC_CBMM_NONE) p = pg_dx_plan(m, kdim, ncols, bits, cu_count());        // (the row groups of this device)
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, workspace, s, [&](int direct, float *out) {
        if (p.path == NNC_CBMM_STREAM) {
            pc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, pk, row_bytes, ncols, centers_dev, k,
                   p.rows_per_group, direct, out);
            LAUNCHCHK("k_cbpkdx_stream");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            if (bits == 4)
                hipLaunchKernelGGL(k_cbpkdx_tiled<4>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim, pk, row_bytes, (long long)ncols,
                                   centers_dev, (int)k, p.col_tiles, p.per_split, direct, out);
            else
                hipLaunchKernelGGL(k_cbpkdx_tiled<2>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim, pk, row_bytes, (long long)ncols,
                                   centers_dev, (int)k, p.col_tiles, p.per_split, direct, out);
            LAUNCHCHK("k_cbpkdx_tiled");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbpk_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    if (pg_check("nnc_cbpk_dc_workspace_bytes", m, kdim, ncols, bits, k) != NNC_OK) return 0;
    PgPlan p;
    if (pg_dc_plan(m, kdim, ncols, bits, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return cbg_dc_ws_bytes(p.path, k);
}

extern "C" int nnc_cbpk_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    int rc = pg_check("nnc_cbpk_dc_plan", m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    PgPlan p;
    if ((rc = pg_dc_plan(m, kdim, ncols, bits, k, std::max(cus, 1), p)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out("nnc_cbpk_dc_plan", kPgCases, kPgNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const int64_t v[NNC_CBPKDC_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.path == NNC_CBMM_ZERO ? 0 : p.copies, p.splits, p.per_split, p.lds,
                                            p.col_tiles, p.row_tiles, p.terms_log2, cbg_dc_ws_bytes(p.path, k)};
    for (int i = 0; i < NNC_CBPKDC_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbpk_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                               int64_t ncols, int32_t k, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbpk_dc_f32";
    int rc = pg_check(fn, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbpk_dc_f32: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbpk_dc_f32: x or g is NULL");
    PgPlan p;
    if ((rc = pg_dc_plan(m, kdim, ncols, bits, k, CB_PLAN_CUS, p)) != NNC_OK) return rc;
    const int64_t need = cbg_dc_ws_bytes(p.path, k);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    const PgCase *pc;
    if ((rc = cbg_stream_case(fn, kPgCases, kPgNames, p.path, bits, p.vb, p.mt, pc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path != NNC_CBMM_ZERO && (rc = pg_dc_plan(m, kdim, ncols, bits, k, cu_count(), p)) != NNC_OK) return rc;   // (the row groups of this device)
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dc(p.path, x, g, m, kdim, ncols, (int)k, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            pc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, pk, row_bytes, ncols, k, p.terms_log2,
                   p.rows_per_group, hdr, sums);
            LAUNCHCHK("k_cbpkdc_stream");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            if (bits == 4)
                hipLaunchKernelGGL(k_cbpkdc_tiled<4>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim, pk, row_bytes, (long long)ncols,
                                   (int)k, p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
            else
                hipLaunchKernelGGL(k_cbpkdc_tiled<2>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim, pk, row_bytes, (long long)ncols,
                                   (int)k, p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
            LAUNCHCHK("k_cbpkdc_tiled");
        }
        return NNC_OK;
    });
}
