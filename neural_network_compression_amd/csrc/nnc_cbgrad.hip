// nnc_cbgrad.hip -- the backward pass of the codebook matmul (nnc_cbmm.hip) from the codebook and the indices, W never decoded
// (include/nnc.h, nnc_cbmm_dx_f32 / nnc_cbmm_dc_f32).  W[i, o] = c[L[i, o]], y = x @ W, g = dL/dy:
//
//   dx[r, i] = sum_o g[r, o] * c[L[i, o]]                      a codebook matmul against W^T, read from the same row-major indices
//   dc[k]    = sum_{(i, o): L[i, o] = k} sum_r x[r, i] * g[r, o]  x^T g binned by index as it is formed; no kdim x ncols dW is written
//
//   k_cbdx_stream  m <= 16.  A workgroup owns 64 lanes x E columns of g (held in registers) and a group of label rows; a wave takes one
//                  row i at a time (CB_UNROLL rows in flight, the loads of k_cbmm_stream), looks the centres up in the per-bank LDS
//                  table and reduces its m partials over the 64 lanes in a fixed order.  Column blocks are the splits: their partials
//                  are summed in block order by k_cbgrad_reduce.
//   k_cbdx_tiled   m > 16.  128 (r) x 128 (i) output tiles; the W^T tile (128 rows i x TB_K columns o) is decoded into LDS from the
//                  row-major indices, then the register-blocked FMA of k_cbmm_tiled.  ncols is split by a count that depends on the
//                  shape alone; the partials go through k_cbgrad_reduce.  Around the decode: the tile skeleton of nnc_cbtile.hpp.
//   k_cbdc_stream  m <= 16.  A lane holds g[0..m-1, o] for its columns; x[r, i] is broadcast by v_readlane; dW[i, o] is formed in
//                  float32 with r ascending and binned at once.  Both dc kernels scale x by 2^scx and g by 2^scg as they load
//                  them (cbdc_scales: the maxima to [0.5, 1)), so dW' = dW * 2^(scx + scg) stays in float32's normal range.
//   k_cbdc_tiled   m > 16.  128 (i) x 128 (o) tiles of x^T g, the reduction over m split by a count that depends on the shape alone:
//                  the prologue, the tile fill and the binning loop of nnc_cbtile.hpp with the label read labels[i * ncols + o].
//   Binning: every dW' (or every m-split's partial) becomes rint(v * 2^(S - scx - scg)) = rint(dW * 2^S) in int64 and is added into K LDS bins (replicated across
//   banks) with integer atomics, then into a global int64[K] with integer atomics: exact, so the result depends on the shape and the
//   data only.  S = 62 - ceil(log2(terms)) - P, 2^P > m * max|x| * max|g|, terms = kdim * ncols * splits; max|x| and max|g| come
//   from k_cbgrad_absmax on the device, the dc kernel derives S itself and writes it next to the sums, and k_cbdc_finish writes
//   dc = ldexp(sum, -S).  No host read anywhere.
// An index >= K reads 0 in dx and falls into no bin in dc, as in the forward pass.  No float atomics.
// The two stream kernels, k_cbgrad_absmax and k_cbgrad_reduce are templates in nnc_cbgrad.hpp (the element type of x and g: this unit
// instantiates them for float32, nnc_cbgrad_h16.hip for bf16 / fp16).
// The plans (CgPlan, dx_plan, dc_plan) and cg_check are in nnc_cbgrad.hpp, where nnc_cbgrad_grouped.hip finds them too; so are the
// sequences of HIP calls of the two entry points (cbg_run_dx, cbg_run_dc) and the list of stream instantiations.  The label row
// loads (cb_row_words) are nnc_cbmm.hpp's, the x load of k_cbdc_stream (cbdc_load_x) nnc_cbgrad.hpp's.
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), 256 threads; thread (tx, ty) owns rows ty*8.. (of g) and columns tx*8.. (i) of the tile.
template <typename LT>
__global__ __launch_bounds__(256) void k_cbdx_tiled(const float *__restrict__ g, long long m, long long kdim, const LT *__restrict__ labels, long long ncols,
                                                    const float *__restrict__ centers, int k, long long col_tiles, long long cols_per_split, int direct,
                                                    float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: W^T[o, n0 + i] = c[L[n0 + i, o]]
    float *cb = ws + TB_K * TB_N;          // k + 1 entries (entry k = 0)
    for (int j = threadIdx.x; j <= k; j += 256) cb[j] = j < k ? centers[j] : 0.0f;

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lo = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lo..lo+3 (as the g tile: row lr, o lo..lo+3)
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
        const long long wi = T.n0 + lr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long go = ob + lo + j;
            ws[(lo + j) * TB_N + lr] = (wi < kdim && go < T.hi) ? cb[std::min((uint32_t)labels[wi * ncols + go], (uint32_t)k)] : 0.0f;
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
// grid (ncols tiles * kdim tiles, splits of m), 256 threads; thread (tx, ty) forms dW for index rows ty*8.. and columns tx*8.. of the
// 128 x 128 tile over its split's rows of m, then bins the 64 values.
template <typename LT>
__global__ __launch_bounds__(256) void k_cbdc_tiled(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                    const LT *__restrict__ labels, long long ncols, int k, int rlog2, int terms_log2, long long col_tiles,
                                                    long long rows_per_split, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
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
    cbdc_bin_tile(acc, T, kdim, ncols, k, Sw, bins, rlog2, threadIdx.x & ((1 << rlog2) - 1),
                  [&](long long i, long long o) { return (uint32_t)labels[i * ncols + o]; });
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ dc = ldexp(sum, -S)
__global__ __launch_bounds__(256) void k_cbdc_finish(const uint32_t *__restrict__ hdr, const long long *__restrict__ sums, int k, int f64, void *__restrict__ out)
{
    const int S = (int)hdr[2], flag = (int)hdr[3];
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += gridDim.x * blockDim.x) {
        const double v = flag == CBG_FLAG_NONFINITE ? __builtin_nan("") : ldexp((double)sums[j], -S);
        if (f64) reinterpret_cast<double *>(out)[j] = v;
        else reinterpret_cast<float *>(out)[j] = (float)v;
    }
}

// ------------------------------------------------------------------ the launches every backward unit shares (nnc_cbgrad.hpp)
template <typename XT>
static void launch_absmax(int agrid, hipStream_t s, const void *x, long long nx, const void *g, long long ng, uint32_t *amax)
{
    hipLaunchKernelGGL(k_cbgrad_absmax<XT>, dim3(agrid), dim3(256), 0, s, reinterpret_cast<const XT *>(x), nx, reinterpret_cast<const XT *>(g), ng, amax);
}

int cbgrad_absmax_dt(const void *x, long long nx, const void *g, long long ng, int dtype, uint32_t *amax, hipStream_t s)
{
    const int agrid = (int)std::max(1LL, std::min(cdiv(std::max(nx, ng), 256 * 8), 4LL * cu_count()));
    if (dtype == NNC_DT_BF16) launch_absmax<bf16_t>(agrid, s, x, nx, g, ng, amax);
    else if (dtype == NNC_DT_F16) launch_absmax<f16_t>(agrid, s, x, nx, g, ng, amax);
    else launch_absmax<float>(agrid, s, x, nx, g, ng, amax);
    LAUNCHCHK("k_cbgrad_absmax");
    return NNC_OK;
}

int cbgrad_reduce_dt(const float *part, long long splits, long long mn, void *out, int out_dtype, hipStream_t s)
{
    const int rgrid = (int)std::max(1LL, std::min(cdiv(mn, 256), 8192LL));
    if (out_dtype == NNC_DT_BF16) hipLaunchKernelGGL(k_cbgrad_reduce<bf16_t>, dim3(rgrid), dim3(256), 0, s, part, splits, mn, reinterpret_cast<bf16_t *>(out));
    else if (out_dtype == NNC_DT_F16) hipLaunchKernelGGL(k_cbgrad_reduce<f16_t>, dim3(rgrid), dim3(256), 0, s, part, splits, mn, reinterpret_cast<f16_t *>(out));
    else hipLaunchKernelGGL(k_cbgrad_reduce<float>, dim3(rgrid), dim3(256), 0, s, part, splits, mn, reinterpret_cast<float *>(out));
    LAUNCHCHK("k_cbgrad_reduce");
    return NNC_OK;
}

int cbdc_finish(const uint32_t *hdr, const long long *sums, int k, int f64, void *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_cbdc_finish, dim3((unsigned)cdiv(k, 256)), dim3(256), 0, s, hdr, sums, k, f64, out);
    LAUNCHCHK("k_cbdc_finish");
    return NNC_OK;
}

// ------------------------------------------------------------------ C ABI
template <typename LT, int VB, int MT>
static void launch_dx_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const float *g, int m, long long kdim, const void *labels, long long ncols,
                             const float *centers, int k, int entries, int cshift, long long rpg, int direct, float *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (aligned)
        hipLaunchKernelGGL((k_cbdx_stream<float, LT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, direct, out);
    else
        hipLaunchKernelGGL((k_cbdx_stream<float, LT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, lab, ncols, centers, k, entries, cshift, rpg, direct, out);
}

template <typename LT, int VB, int MT>
static void launch_dc_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const float *x, const float *g, int m, long long kdim, const void *labels,
                             long long ncols, int k, int rlog2, int tl, long long rpg, uint32_t *hdr, unsigned long long *sums)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (aligned)
        hipLaunchKernelGGL((k_cbdc_stream<float, LT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, lab, ncols, k, rlog2, tl, rpg, hdr, sums);
    else
        hipLaunchKernelGGL((k_cbdc_stream<float, LT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, lab, ncols, k, rlog2, tl, rpg, hdr, sums);
}

// every stream instantiation there is (the lists of nnc_cbgrad.hpp); the plans are checked against this table, and the launches go through it
using DxLaunch = void (*)(bool, dim3, size_t, hipStream_t, const float *, int, long long, const void *, long long, const float *, int, int, int, long long,
                          int, float *);
using DcLaunch = void (*)(bool, dim3, size_t, hipStream_t, const float *, const float *, int, long long, const void *, long long, int, int, int, long long,
                          uint32_t *, unsigned long long *);
struct GradCase {
    int a, vb, mt;            // a: label_bytes
    DxLaunch dx;
    DcLaunch dc;
};
#define U8_CASE(VB, MT) {1, VB, MT, launch_dx_stream<uint8_t, VB, MT>, launch_dc_stream<uint8_t, VB, MT>},
#define U16_CASE(VB, MT) {2, VB, MT, launch_dx_stream<uint16_t, VB, MT>, launch_dc_stream<uint16_t, VB, MT>},
static const GradCase kGradCases[] = {CBG_U8_STREAM_CASES(U8_CASE) CBG_U16_STREAM_CASES(U16_CASE)};
#undef U8_CASE
#undef U16_CASE
static const CbgCaseNames kGradNames = {false, "label_bytes", true};

extern "C" int64_t nnc_cbmm_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (cg_check("nnc_cbmm_dx_workspace_bytes", m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(dx_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS, 0).splits, m, kdim);
}

extern "C" int nnc_cbmm_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr, int64_t *out)
{
    int rc = cg_check("nnc_cbmm_dx_plan", m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    const CgPlan p = dx_plan(m, kdim, ncols, label_bytes, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out("nnc_cbmm_dx_plan", kGradCases, kGradNames, p.path, label_bytes, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const int64_t v[NNC_CBDX_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries, p.splits,
                                          p.per_split, p.aligned, p.lds, p.col_tiles, p.row_tiles, cbg_dx_ws_bytes(p.splits, m, kdim)};
    for (int i = 0; i < NNC_CBDX_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_dx_f32(const float *g, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols, const float *centers_dev,
                               int32_t k, float *dx, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = cg_check("nnc_cbmm_dx_f32", m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbmm_dx_f32: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbmm_dx_f32: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_dx_f32: g or labels is NULL");
    const int64_t need = nnc_cbmm_dx_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace("nnc_cbmm_dx_f32", "nnc_cbmm_dx_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    const CgPlan p = dx_plan(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case("nnc_cbmm_dx_f32", kGradCases, kGradNames, p.path, label_bytes, p.vb, p.mt, gc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, workspace, s, [&](int direct, float *out) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dx(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, labels, ncols, centers_dev, k,
                   p.entries, p.cshift, p.rows_per_group, direct, out);
            LAUNCHCHK("k_cbdx_stream");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            if (label_bytes == 1)
                hipLaunchKernelGGL(k_cbdx_tiled<uint8_t>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim,
                                   reinterpret_cast<const uint8_t *>(labels), (long long)ncols, centers_dev, (int)k, p.col_tiles, p.per_split, direct, out);
            else
                hipLaunchKernelGGL(k_cbdx_tiled<uint16_t>, grid, dim3(256), (size_t)p.lds, s, g, (long long)m, (long long)kdim,
                                   reinterpret_cast<const uint16_t *>(labels), (long long)ncols, centers_dev, (int)k, p.col_tiles, p.per_split, direct, out);
            LAUNCHCHK("k_cbdx_tiled");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbmm_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (cg_check("nnc_cbmm_dc_workspace_bytes", m, kdim, ncols, label_bytes, k) != NNC_OK) return 0;
    return cbg_dc_ws_bytes(dc_plan(m, kdim, ncols, label_bytes, k, CB_PLAN_CUS, 0).path, k);
}

extern "C" int nnc_cbmm_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr, int64_t *out)
{
    int rc = cg_check("nnc_cbmm_dc_plan", m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    const CgPlan p = dc_plan(m, kdim, ncols, label_bytes, k, cus, (uintptr_t)labels_addr);
    if ((rc = cbg_plan_out("nnc_cbmm_dc_plan", kGradCases, kGradNames, p.path, label_bytes, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    const int64_t v[NNC_CBDC_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_ZERO ? 0 : 1LL << p.rlog2, p.splits, p.per_split, p.aligned, p.lds,
                                          p.col_tiles, p.row_tiles, p.terms_log2, cbg_dc_ws_bytes(p.path, k)};
    for (int i = 0; i < NNC_CBDC_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols, int32_t k,
                               void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = cg_check("nnc_cbmm_dc_f32", m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbmm_dc_f32: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g || !labels)) return fail(NNC_EINVAL, "nnc_cbmm_dc_f32: x, g or labels is NULL");
    const int64_t need = nnc_cbmm_dc_workspace_bytes(m, kdim, ncols, label_bytes, k);
    if ((rc = cb_check_workspace("nnc_cbmm_dc_f32", "nnc_cbmm_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    const CgPlan p = dc_plan(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    const GradCase *gc;
    if ((rc = cbg_stream_case("nnc_cbmm_dc_f32", kGradCases, kGradNames, p.path, label_bytes, p.vb, p.mt, gc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    return cbg_run_dc(p.path, x, g, m, kdim, ncols, (int)k, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            gc->dc(p.aligned != 0, dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, labels, ncols, k, p.rlog2,
                   p.terms_log2, p.rows_per_group, hdr, sums);
            LAUNCHCHK("k_cbdc_stream");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            if (label_bytes == 1)
                hipLaunchKernelGGL(k_cbdc_tiled<uint8_t>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim,
                                   reinterpret_cast<const uint8_t *>(labels), (long long)ncols, (int)k, p.rlog2, p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
            else
                hipLaunchKernelGGL(k_cbdc_tiled<uint16_t>, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim,
                                   reinterpret_cast<const uint16_t *>(labels), (long long)ncols, (int)k, p.rlog2, p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
            LAUNCHCHK("k_cbdc_tiled");
        }
        return NNC_OK;
    });
}
