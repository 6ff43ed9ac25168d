// nnc_cbmm_h16.hip -- the codebook matmul of nnc_cbmm.hip on bf16 / fp16 activations (include/nnc.h, nnc_cbmm_h16; DESIGN.md
// section 16): y = x @ W_h + bias, W_h[i, o] = the centre of labels[i, o] rounded to x's type.  A product of two bf16 or two fp16
// values is exact in float32; every sum is float32.
//
//   k_cbmm_stream<XT>  m <= 16: nnc_cbmm.hpp's stream kernel with x read as XT and widened and the table holding the rounded
//                      centres widened: the float32 path's fmaf chain on half the x bytes.
//   k_cbmm_mfma        m > 16: a workgroup of 4 waves owns a 128 x 128 output tile, each wave a 64 x 64 quarter as 2 x 2
//                      v_mfma_f32_32x32x16_{bf16,f16} accumulators.  Per k step of HM_BK = 32 the W tile is looked up through the
//                      per-bank LDS table (the stream kernel's) and written as XT into a [column][k] LDS image (labels are row-major
//                      (kdim, ncols): a thread reads 16 rows of one column, coalesced over the wave, and writes them as two 16-byte
//                      runs of k); x goes into a [row][k] image as 16-byte fragments (XVEC: x 16-byte aligned, kdim a multiple of 8)
//                      or element by element.  A lane's A / B fragment is then one 16-byte LDS read.  The labels and x of the next
//                      step are loaded into registers before the MFMAs of this one.  Everything past kdim (or past the split), past
//                      m and past ncols is zero in both images, never memory: a NaN there would reach valid outputs as NaN * 0.
//                      The tile itself (LDS carve-up, coordinates, x fragments, both image stores, the lookup into the W image, the
//                      MFMA step, the C / D epilogue) is nnc_cbmfma.hpp's, shared with the other four forward units and the dx
//                      kernels; the kernel keeps its table, the label load, the lookup and, alone among them, its own copy of
//                      the k loop (hm_accumulate's barriers and order, written out).
//   k_cbmm_reduce      the split-K partials (float32) in split order, + bias, ReLU, rounded once to the output type.
#include "nnc_cbmfma.hpp"

// grid (col_tiles * row_tiles, splits), HM_THREADS threads.  `out` is y (direct 1: float32, 2: XT; + bias, ReLU here) or the float32
// partials [split][m][ncols] (direct 0).  rows_per_split is a multiple of HM_BK.
template <typename XT, typename LT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbmm_mfma(const XT *__restrict__ x, long long m, long long kdim, const LT *__restrict__ labels,
                                                          long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                          long long col_tiles, long long rows_per_split, const float *__restrict__ bias, int relu,
                                                          int direct, void *__restrict__ out_)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, entries, cshift);
    cb_fill<XT>(L.cb, L.stage, centers, k, entries, cshift);

    const HmTile T = hm_tile(col_tiles, rows_per_split, kdim);
    const long long gc = T.n0 + T.wc;
    const bool col_ok = gc < ncols;
    uint32_t lab[16];
    uint4 xf[2];

    auto load = [&](long long kb) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long gk = kb + T.wk0 + j;
            lab[j] = (col_ok && gk < T.k_hi) ? (uint32_t)labels[gk * ncols + gc] : 0u;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) xf[i] = hm_load_x<XT, XVEC>(x, m, kdim, T.m0, kb, T.k_hi, T.t + i * HM_THREADS);
    };
    auto store = [&](long long kb) {
        hm_lookup_w(L.ws, L.cb, T, col_ok, kb, lab, [&](uint32_t l) { return CbTable<LT>::index(l, k, cshift, T.lane); });
#pragma unroll
        for (int i = 0; i < 2; ++i) hm_store_x(L.xs, T.t + i * HM_THREADS, xf[i]);
    };

    // hm_accumulate's loop, written out: through the shared loop this kernel compiles to a slower instruction stream (DESIGN.md
    // section 31)
    typename HFrag<XT>::C acc[2][2];
    hm_clear<XT>(acc);
    load(T.k_lo);
    for (long long kb = T.k_lo; kb < T.k_hi; kb += HM_BK) {
        __syncthreads();   // the table is filled (first step); the images of the step before have been read
        store(kb);
        __syncthreads();
        if (kb + HM_BK < T.k_hi) load(kb + HM_BK);
        hm_step(L.xs, L.ws, T.wm, T.wn, T.fr, T.fh, acc);
    }
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, ncols, bias, relu, direct, out_);
}

// ------------------------------------------------------------------ launches
template <typename XT, typename LT, int VB, int MT>
static void launch_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const void *x, int m, long long kdim, const void *labels, long long ncols,
                          const float *centers, int k, int entries, int cshift, long long rps, const float *bias, int relu, int direct, void *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    const XT *xp = reinterpret_cast<const XT *>(x);
    if (aligned)
        hipLaunchKernelGGL((k_cbmm_stream<XT, LT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, xp, m, kdim, lab, ncols, centers, k, entries, cshift, rps, bias, relu, direct, out);
    else
        hipLaunchKernelGGL((k_cbmm_stream<XT, LT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, xp, m, kdim, lab, ncols, centers, k, entries, cshift, rps, bias, relu, direct, out);
}

template <typename XT, typename LT>
static void launch_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const void *labels, long long ncols,
                        const float *centers, int k, int entries, int cshift, long long col_tiles, long long rps, const float *bias, int relu, int direct,
                        void *out)
{
    hm_launch(x, kdim, k_cbmm_mfma<XT, LT, true>, k_cbmm_mfma<XT, LT, false>, grid, lds, s, reinterpret_cast<const XT *>(x), m, kdim,
              reinterpret_cast<const LT *>(labels), ncols, centers, k, entries, cshift, col_tiles, rps, bias, relu, direct, out);
}

// every kernel instantiation of this unit; the plan is checked against these tables, and the launches go through them
using StreamLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, int, long long, const void *, long long, const float *, int, int, int,
                              long long, const float *, int, int, void *);
using MfmaLaunch = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const void *, long long, const float *, int, int, int,
                            long long, long long, const float *, int, int, void *);
struct StreamCase {
    int dt, lb, vb, mt;
    StreamLaunch fn;
};
struct MfmaCase {
    int dt, lb;
    MfmaLaunch fn;
};
#define H16_STREAM_CASES(DT, XT)                                                                                                        \
    {DT, 1, 16, 1, launch_stream<XT, uint8_t, 16, 1>}, {DT, 1, 16, 2, launch_stream<XT, uint8_t, 16, 2>},                               \
    {DT, 1, 16, 4, launch_stream<XT, uint8_t, 16, 4>}, {DT, 1, 8, 8, launch_stream<XT, uint8_t, 8, 8>},                                 \
    {DT, 1, 4, 16, launch_stream<XT, uint8_t, 4, 16>}, {DT, 2, 16, 1, launch_stream<XT, uint16_t, 16, 1>},                              \
    {DT, 2, 16, 2, launch_stream<XT, uint16_t, 16, 2>}, {DT, 2, 16, 4, launch_stream<XT, uint16_t, 16, 4>},                             \
    {DT, 2, 16, 8, launch_stream<XT, uint16_t, 16, 8>}, {DT, 2, 8, 16, launch_stream<XT, uint16_t, 8, 16>}
static const StreamCase kStreamCases[] = {H16_STREAM_CASES(NNC_DT_BF16, bf16_t), H16_STREAM_CASES(NNC_DT_F16, f16_t)};
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 1, launch_mfma<bf16_t, uint8_t>}, {NNC_DT_BF16, 2, launch_mfma<bf16_t, uint16_t>},
    {NNC_DT_F16, 1, launch_mfma<f16_t, uint8_t>},   {NNC_DT_F16, 2, launch_mfma<f16_t, uint16_t>},
};

static StreamLaunch find_stream(int dt, int lb, int vb, int mt)
{
    for (const StreamCase &c : kStreamCases)
        if (c.dt == dt && c.lb == lb && c.vb == vb && c.mt == mt) return c.fn;
    return nullptr;
}

static MfmaLaunch find_mfma(int dt, int lb)
{
    for (const MfmaCase &c : kMfmaCases)
        if (c.dt == dt && c.lb == lb) return c.fn;
    return nullptr;
}

// NNC_OK if the library holds the kernel the plan names
static int have_kernel(const CbPlan &p, int dt, int lb)
{
    if (p.path == NNC_CBMM_STREAM && !find_stream(dt, lb, p.vb, p.mt))
        return fail(NNC_EINVAL, "nnc_cbmm_h16: no k_cbmm_stream instantiation for dtype " + std::to_string(dt) + ", label_bytes " + std::to_string(lb) +
                                    ", vb " + std::to_string(p.vb) + ", mt " + std::to_string(p.mt));
    if (p.path == NNC_CBMM_MFMA && !find_mfma(dt, lb))
        return fail(NNC_EINVAL, "nnc_cbmm_h16: no k_cbmm_mfma instantiation for dtype " + std::to_string(dt) + ", label_bytes " + std::to_string(lb));
    return NNC_OK;
}

// ------------------------------------------------------------------ C ABI
static int h16_check(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: x_dtype must be NNC_DT_BF16 or NNC_DT_F16");
    if (m < 0 || kdim < 0 || ncols < 0) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: negative size");
    if (label_bytes != 1 && label_bytes != 2) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: label_bytes must be 1 or 2");
    if (k < 1 || k > NNC_KMAX) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: k outside 1..NNC_KMAX");
    if (label_bytes == 1 && k > 256) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: k > 256 needs 2-byte labels");
    if (m > (1LL << 40) || kdim > (1LL << 40) || ncols > (1LL << 40)) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: size too large");
    return NNC_OK;
}

extern "C" int64_t nnc_cbmm_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || h16_check(NNC_DT_BF16, m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    return cb_ws_bytes(cb_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS, 0, true), m, ncols);
}

extern "C" int nnc_cbmm_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr,
                                 int64_t *out)
{
    int rc = h16_check(x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16_plan: cus < 1");
    if (!out) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16_plan: out is NULL");
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cus, (uintptr_t)labels_addr, true);
    rc = have_kernel(p, x_dtype, label_bytes);
    if (rc != NNC_OK) return rc;
    const int64_t v[NNC_CBMM_H16_PLAN_LEN] = {p.path, p.vb, p.mt, p.entries ? 1LL << p.cshift : 0, p.entries, p.splits, p.rows_per_split, p.aligned,
                                              p.lds, p.col_tiles, p.row_tiles, cb_ws_bytes(p, m, ncols), x_dtype};
    for (int i = 0; i < NNC_CBMM_H16_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_h16(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols,
                            const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, void *y, int y_dtype, void *workspace,
                            int64_t workspace_bytes, void *stream)
{
    int rc = h16_check(x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if ((rc = cb_check_operands("nnc_cbmm_h16", x, x_dtype, y, y_dtype, centers_dev, m, kdim, ncols, !x || !labels, "x or labels")) != NNC_OK) return rc;
    const int64_t need = nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace("nnc_cbmm_h16", "nnc_cbmm_h16_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels), true);
    if (p.path == NNC_CBMM_BIAS) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // kdim = 0: y = bias
    rc = have_kernel(p, x_dtype, label_bytes);
    if (rc != NNC_OK) return rc;
    const int direct = cb_direct(p.splits, y_dtype);
    void *out = direct ? y : workspace;
    if (p.path == NNC_CBMM_STREAM) {
        const dim3 grid((unsigned)p.col_tiles, (unsigned)p.splits);
        find_stream(x_dtype, label_bytes, p.vb, p.mt)(p.aligned != 0, grid, (size_t)p.lds, s, x, (int)m, kdim, labels, ncols, centers_dev, k, p.entries,
                                                      p.cshift, p.rows_per_split, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbmm_stream (h16)");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        find_mfma(x_dtype, label_bytes)(grid, (size_t)p.lds, s, x, m, kdim, labels, ncols, centers_dev, k, p.entries, p.cshift, p.col_tiles, p.rows_per_split,
                                        bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbmm_mfma");
    }
    return cb_finish(direct, workspace, p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
}
