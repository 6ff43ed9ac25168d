// nnc_cbspgrad.hip -- the backward pass of the bitmap-sparse codebook matmul (nnc_cbsp.hip) from the packed form: the indices are
// never unpacked and W is never decoded (include/nnc.h, nnc_cbsp_dx_f32 / nnc_cbsp_dc_f32).  With the
// skipped symbol z, c_z = c[z] (0 if z >= K), d[s] = float32(c[s] - c_z) (-c_z for s >= K) and g = dL/dy:
//
//   dx[r, i] = c_z * sum_o g[r, o] + sum over the stored (i, o) of g[r, o] * d[L[i, o]]   the Jacobian of nnc_cbsp_f32; with
//                                                                                        c_z == 0 the rank-1 term is dropped
//   dc[k]    = nnc_cbmm_dc_f32 on the unpacked labels, bit for bit: every dW[i, o] is formed in float32 as k_cbdc_stream /
//              k_cbdc_tiled form it (from x and g scaled by the same powers of two) and binned as rint(dW * 2^S) with the same S
//              (the same splits of m and T); a skipped (i, o)
//              falls into bin z (none if z >= K).  Integer sums do not depend on order.
//
//   k_cbspdx_stream  m <= 16.  A workgroup owns a block of E segments (64 lanes x E columns of g in registers, E * MT <= 32) and
//                    a group of index rows.  A wave takes its rows in batches of 64 / E: the bitmap words and counts of a batch come
//                    in one vector load (lane = row x segment; the next batch's are in flight while this one is consumed) and are
//                    broadcast by v_readlane; a lane's symbol is at count + v_mbcnt(word), its d from the per-bank LDS table; the m
//                    partials of a row are reduced over the wave in a fixed order (wave_reduce_rows).  A skipped weight forms no
//                    product.  Column blocks are the splits, summed in block order by k_cbgrad_reduce.
//   k_cbspdx_tiled   m > 16.  128 (r) x 128 (i) output tiles; the W^T tile is decoded into LDS from bitmap and symbols (d where
//                    stored, 0 where skipped), then tb_tile_fma (the masked step for a g tile holding Inf / NaN).  ncols is split
//                    into whole segments by a count that depends on the shape alone.  The tile coordinates, the g tile load
//                    and the store are nnc_cbtile.hpp's.
//   k_cbspdx_rank1   dx += c_z * sum_o g[r, o], the row sums of g in a fixed order (k_cbsp_rowsum); nothing when c_z == 0.
//   k_cbspdc_stream  m <= 16.  The grid and loads of k_cbspdx_stream; x[r, i] by v_readlane; dW[i, o] as k_cbdc_stream forms it.
//                    A stored weight's image goes into the replicated LDS bins (64-bit integer atomics), a skipped one's into a
//                    per-lane int64 register for bin z, flushed once per lane at the end.
//   k_cbspdc_tiled   m > 16.  k_cbdc_tiled's tiles and splits of m (the prologue and tile fill of nnc_cbtile.hpp); each of a
//                    thread's 64 values takes its label from the bitmap word, the count and the popcount; the skipped ones are
//                    summed in a register.
// k_cbgrad_absmax, k_cbdc_finish and k_cbgrad_reduce are nnc_cbgrad.hip's.  No float atomics; no host read.
// The sequences of HIP calls of the two entry points (cbg_run_dx, cbg_run_dc) and the lookup in the table of stream instantiations
// are nnc_cbgrad.hpp's; the row sums and the rank-1 term of dx stay here, around that sequence.
// The plans, the checks, the stream kernels and k_cbspdx_rank1 are written in nnc_cbspgrad.hpp, with the element type as a template
// parameter, for the bf16 / fp16 unit (nnc_cbspgrad_h16.hip, section 24) to share; this unit instantiates them for float32.
#include "nnc_cbspgrad.hpp"
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), 256 threads; thread (tx, ty) owns rows ty*8.. (of g) and columns tx*8.. (i) of the tile.
template <typename LT>
__global__ __launch_bounds__(256) void k_cbspdx_tiled(const float *__restrict__ g, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                      const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const LT *__restrict__ sym,
                                                      long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k, int z,
                                                      long long col_tiles, long long cols_per_split, int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: d of the stored W[n0 + i, o], 0 where skipped
    float *tab = ws + TB_K * TB_N;         // k + 1 entries: d, then -c_z
    unsigned char *kept = reinterpret_cast<unsigned char *>(tab + k + 1);   // [TB_K][TB_N]: 1 where the weight is stored
    const float cz = sp_cz(centers, k, z);
    for (int j = threadIdx.x; j <= k; j += 256) tab[j] = (j < k ? centers[j] : 0.0f) - cz;

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lq = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lq..lq+3 (one segment), as the g tile
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        const int nonfinite = tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
        const long long wi = T.n0 + lr, go = ob + lq;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t keep = 0;
        if (wi < kdim && go < T.hi) {   // (bits past ncols are 0; a split ends on a segment boundary)
            const long long gi = wi * segs, sg = go >> 6;
            const int b0 = (int)(go & 63);
            const uint64_t word = bitmap[gi + sg];
            long long pos = sp_count(lo[gi + sg], lo[gi], hi[wi]) + __popcll(word & ((1ULL << b0) - 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((word >> (b0 + j)) & 1) {
                    if (pos < nnz) {
                        v[j] = tab[std::min((uint32_t)sym[pos], (uint32_t)k)];
                        keep |= 1u << j;
                    }
                    ++pos;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[(lq + j) * TB_N + lr] = v[j];
            kept[(lq + j) * TB_N + lr] = (unsigned char)((keep >> j) & 1);
        }
        // a skipped weight is absent: where the g tile holds an Inf or NaN the FMA must not form g * 0 at a skipped position
        if (__syncthreads_or(nonfinite)) tb_tile_fma_masked(gs, ws, kept, T.tx, T.ty, acc);
        else tb_tile_fma(gs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_dx(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, kdim, direct, out);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), 256 threads; the tiles and the FMA of k_cbdc_tiled, so the same 64 values per
// thread; their labels come from the bitmap: a thread's 8 columns tx*8.. lie in one segment.
template <typename LT>
__global__ __launch_bounds__(256) void k_cbspdc_tiled(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                      const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                      const LT *__restrict__ sym, long long nnz, long long ncols, long long segs, int k, int z, int rlog2,
                                                      int terms_log2, long long col_tiles, long long rows_per_split, uint32_t *__restrict__ hdr,
                                                      unsigned long long *__restrict__ sums)
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
    // the binning is not cbdc_bin_tile's: a row's labels are read off one running position, and the skipped weights go to bin z
    // through a register, not one atomic each
    const int rep = threadIdx.x & ((1 << rlog2) - 1);
    const long long ob = T.n0 + T.tx * 8, sg = ob >> 6;
    const int b0 = (int)(ob & 63);
    unsigned long long skip = 0;   // the images of the thread's skipped weights: bin z
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const long long i = T.m0 + T.ty * 8 + a;
        if (i >= kdim || ob >= ncols) continue;
        const long long gi = i * segs;
        const uint64_t word = bitmap[gi + sg];
        long long pos = sp_count(lo[gi + sg], lo[gi], hi[i]) + __popcll(word & ((1ULL << b0) - 1));
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (ob + b >= ncols) continue;
            const unsigned long long img = cbdc_fix(acc[a][b], Sw);
            if ((word >> (b0 + b)) & 1) {
                const uint32_t l = pos < nnz ? (uint32_t)sym[pos] : (uint32_t)z;   // (past nnz: skipped, as nnc_cbsp_unpack reads it)
                ++pos;
                if (l < (uint32_t)k) atomicAdd(&bins[(l << rlog2) + rep], img);
            } else {
                skip += img;
            }
        }
    }
    if (z < k && skip) atomicAdd(&bins[((uint32_t)z << rlog2) + rep], skip);
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ C ABI
template <typename LT, int MT>
static void launch_sg_dx(dim3 grid, size_t lds, hipStream_t s, const float *g, int m, long long kdim, const unsigned char *base, const SpLayout &L,
                         long long nnz, long long ncols, const float *centers, int k, int z, const SgPlan &p, int direct, float *out)
{
    hipLaunchKernelGGL((k_cbspdx_stream<float, LT, MT>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, reinterpret_cast<const uint64_t *>(base),
                       reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi),
                       reinterpret_cast<const LT *>(base + L.off_sym), nnz, ncols, L.segs, centers, k, z, p.entries, p.cshift, p.rows_per_group, direct,
                       out);
}

template <typename LT, int MT>
static void launch_sg_dc(dim3 grid, size_t lds, hipStream_t s, const float *x, const float *g, int m, long long kdim, const unsigned char *base,
                         const SpLayout &L, long long nnz, long long ncols, int k, int z, const SgPlan &p, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbspdc_stream<float, LT, MT>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, reinterpret_cast<const uint64_t *>(base),
                       reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi),
                       reinterpret_cast<const LT *>(base + L.off_sym), nnz, ncols, L.segs, k, z, p.rlog2, p.terms_log2, p.rows_per_group, hdr, sums);
}

// every stream instantiation there is; the plans are checked against this table, and the launches go through it
using SgDxLaunch = void (*)(dim3, size_t, hipStream_t, const float *, int, long long, const unsigned char *, const SpLayout &, long long, long long,
                            const float *, int, int, const SgPlan &, int, float *);
using SgDcLaunch = void (*)(dim3, size_t, hipStream_t, const float *, const float *, int, long long, const unsigned char *, const SpLayout &, long long,
                            long long, int, int, const SgPlan &, uint32_t *, unsigned long long *);
struct SgCase {
    int a, vb, mt;            // a: label_bytes; vb: 0 (a lane's columns are fixed by mt)
    SgDxLaunch dx;
    SgDcLaunch dc;
};
#define SG_CASE(LT, LB, MT) {LB, 0, MT, launch_sg_dx<LT, MT>, launch_sg_dc<LT, MT>}
static const SgCase kSgCases[] = {
    SG_CASE(uint8_t, 1, 1),  SG_CASE(uint8_t, 1, 2),  SG_CASE(uint8_t, 1, 4),  SG_CASE(uint8_t, 1, 8),  SG_CASE(uint8_t, 1, 16),
    SG_CASE(uint16_t, 2, 1), SG_CASE(uint16_t, 2, 2), SG_CASE(uint16_t, 2, 4), SG_CASE(uint16_t, 2, 8), SG_CASE(uint16_t, 2, 16),
};
#undef SG_CASE
static const CbgCaseNames kSgNames = {false, "label_bytes", false};

extern "C" int64_t nnc_cbsp_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (sg_check("nnc_cbsp_dx_workspace_bytes", m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    return sg_dx_ws_bytes(sg_dx_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS), m, kdim);
}

extern "C" int nnc_cbsp_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out)
{
    int rc = sg_check("nnc_cbsp_dx_plan", m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    const SgPlan p = sg_dx_plan(m, kdim, ncols, label_bytes, k, cus);
    if ((rc = cbg_plan_out("nnc_cbsp_dx_plan", kSgCases, kSgNames, p.path, label_bytes, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const int64_t v[NNC_CBSPDX_PLAN_LEN] = {p.path, p.mt, p.segs, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries,
                                            p.splits, p.per_split, p.lds, p.col_tiles, p.row_tiles, sg_dx_ws_bytes(p, m, kdim)};
    for (int i = 0; i < NNC_CBSPDX_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbsp_dx_f32(const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes, int64_t ncols,
                               int32_t zero_symbol, int64_t nnz, const float *centers_dev, int32_t k, float *dx, void *workspace, int64_t workspace_bytes,
                               void *stream)
{
    const char *fn = "nnc_cbsp_dx_f32";
    int rc = sg_check(fn, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if ((rc = sg_check_form(fn, m, kdim, ncols, label_bytes, zero_symbol, nnz, packed, packed_bytes)) != NNC_OK) return rc;
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbsp_dx_f32: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbsp_dx_f32: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbsp_dx_f32: g is NULL");
    const int64_t need = nnc_cbsp_dx_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_dx_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK) return rc;
    const SgPlan p = sg_dx_plan(m, kdim, ncols, label_bytes, k, cu_count());
    const SgCase *sc;
    if ((rc = cbg_stream_case(fn, kSgCases, kSgNames, p.path, label_bytes, 0, p.mt, sc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SpLayout L = sp_layout(kdim, ncols, label_bytes, nnz);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    float *rs = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sg_part_bytes(p, m, kdim));   // behind the partials
    // the row sums of g ahead of the kernel, the rank-1 term behind the reduce: the two steps the other forms do not have
    rc = cbg_run_dx(p.path, p.splits, m, kdim, dx, workspace, s, [&](int direct, float *out) {
        const int rr = cbsp_rowsum(g, m, ncols, rs, s);
        if (rr != NNC_OK) return rr;
        if (p.path == NNC_CBMM_STREAM) {
            sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, base, L, nnz, ncols, centers_dev, k, zero_symbol, p,
                   direct, out);
            LAUNCHCHK("k_cbspdx_stream");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            const uint64_t *bm = reinterpret_cast<const uint64_t *>(base);
            const uint32_t *lo = reinterpret_cast<const uint32_t *>(base + L.off_lo), *hi = reinterpret_cast<const uint32_t *>(base + L.off_hi);
            if (label_bytes == 1)
                hipLaunchKernelGGL(k_cbspdx_tiled<uint8_t>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim, bm, lo, hi,
                                   reinterpret_cast<const uint8_t *>(base + L.off_sym), (long long)nnz, (long long)ncols, L.segs, centers_dev, (int)k,
                                   (int)zero_symbol, p.col_tiles, p.per_split, direct, out);
            else
                hipLaunchKernelGGL(k_cbspdx_tiled<uint16_t>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim, bm, lo, hi,
                                   reinterpret_cast<const uint16_t *>(base + L.off_sym), (long long)nnz, (long long)ncols, L.segs, centers_dev, (int)k,
                                   (int)zero_symbol, p.col_tiles, p.per_split, direct, out);
            LAUNCHCHK("k_cbspdx_tiled");
        }
        return NNC_OK;
    });
    if (rc != NNC_OK || (p.path != NNC_CBMM_STREAM && p.path != NNC_CBMM_TILED)) return rc;
    const int rgrid = (int)std::max(1LL, std::min(cdiv(m * kdim, 256), 8192LL));
    hipLaunchKernelGGL(k_cbspdx_rank1<float>, dim3(rgrid), dim3(256), 0, s, dx, (long long)m, (long long)kdim, rs, centers_dev, (int)k, (int)zero_symbol);
    LAUNCHCHK("k_cbspdx_rank1");
    return NNC_OK;
}

extern "C" int64_t nnc_cbsp_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (sg_check("nnc_cbsp_dc_workspace_bytes", m, kdim, ncols, label_bytes, k) != NNC_OK) return 0;
    SgPlan p;
    if (sg_dc_plan(m, kdim, ncols, label_bytes, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return cbg_dc_ws_bytes(p.path, k);
}

extern "C" int nnc_cbsp_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out)
{
    int rc = sg_check("nnc_cbsp_dc_plan", m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    SgPlan p;
    if ((rc = sg_dc_plan(m, kdim, ncols, label_bytes, k, cus, p)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out("nnc_cbsp_dc_plan", kSgCases, kSgNames, p.path, label_bytes, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const int64_t v[NNC_CBSPDC_PLAN_LEN] = {p.path, p.mt, p.segs, p.path == NNC_CBMM_ZERO ? 0 : 1LL << p.rlog2, p.splits, p.per_split, p.lds,
                                            p.col_tiles, p.row_tiles, p.terms_log2, cbg_dc_ws_bytes(p.path, k)};
    for (int i = 0; i < NNC_CBSPDC_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbsp_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes,
                               int64_t ncols, int32_t zero_symbol, int64_t nnz, int32_t k, void *dc, int32_t out_f64, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_dc_f32";
    int rc = sg_check(fn, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if ((rc = sg_check_form(fn, m, kdim, ncols, label_bytes, zero_symbol, nnz, packed, packed_bytes)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbsp_dc_f32: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbsp_dc_f32: x or g is NULL");
    const int64_t need = nnc_cbsp_dc_workspace_bytes(m, kdim, ncols, label_bytes, k);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    SgPlan p;
    if ((rc = sg_dc_plan(m, kdim, ncols, label_bytes, k, cu_count(), p)) != NNC_OK) return rc;
    const SgCase *sc;
    if ((rc = cbg_stream_case(fn, kSgCases, kSgNames, p.path, label_bytes, 0, p.mt, sc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SpLayout L = sp_layout(kdim, ncols, label_bytes, nnz);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    return cbg_run_dc(p.path, x, g, m, kdim, ncols, (int)k, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, base, L, nnz, ncols, k, zero_symbol, p, hdr, sums);
            LAUNCHCHK("k_cbspdc_stream");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            const uint64_t *bm = reinterpret_cast<const uint64_t *>(base);
            const uint32_t *lo = reinterpret_cast<const uint32_t *>(base + L.off_lo), *hi = reinterpret_cast<const uint32_t *>(base + L.off_hi);
            if (label_bytes == 1)
                hipLaunchKernelGGL(k_cbspdc_tiled<uint8_t>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim, bm, lo, hi,
                                   reinterpret_cast<const uint8_t *>(base + L.off_sym), (long long)nnz, (long long)ncols, L.segs, (int)k, (int)zero_symbol,
                                   p.rlog2, p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
            else
                hipLaunchKernelGGL(k_cbspdc_tiled<uint16_t>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim, bm, lo, hi,
                                   reinterpret_cast<const uint16_t *>(base + L.off_sym), (long long)nnz, (long long)ncols, L.segs, (int)k, (int)zero_symbol,
                                   p.rlog2, p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
            LAUNCHCHK("k_cbspdc_tiled");
        }
        return NNC_OK;
    });
}
