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
//   k_cbmm_reduce      the split-K partials (float32) in split order, + bias, ReLU, rounded once to the output type.
#include "nnc_cbmm.hpp"

// grid (col_tiles * row_tiles, splits), HM_THREADS threads.  `out` is y (direct 1: float32, 2: XT; + bias, ReLU here) or the float32
// partials [split][m][ncols] (direct 0).  rows_per_split is a multiple of HM_BK.
template <typename XT, typename LT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbmm_mfma(const XT *__restrict__ x, long long m, long long kdim, const LT *__restrict__ labels,
                                                          long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                          long long col_tiles, long long rows_per_split, const float *__restrict__ bias, int relu,
                                                          int direct, void *__restrict__ out_)
{
    using F = HFrag<XT>;
    using V = typename F::V;
    using C = typename F::C;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    float *cb = hm_smem;                                // entries << cshift
    float *stage = cb + (entries << cshift);            // entries
    XT *xs = reinterpret_cast<XT *>(hm_smem + hm_table_words(entries, cshift));   // [HM_BM][HM_LD]: x tile, row-major in k
    XT *ws = xs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: W tile, column-major (k contiguous)
    cb_fill<XT>(cb, stage, centers, k, entries, cshift);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long n0 = (blockIdx.x % col_tiles) * HM_BN, m0 = (blockIdx.x / col_tiles) * HM_BM;
    const long long k_lo = (long long)blockIdx.y * rows_per_split, k_hi = std::min(kdim, k_lo + rows_per_split);

    // W: thread t owns column wc of the tile and its 16 rows wk0 .. wk0 + 15 of the k step
    const int wc = t & (HM_BN - 1), wk0 = (t >> 7) * 16;
    const long long gc = n0 + wc;
    const bool col_ok = gc < ncols;
    // x: fragments f = t and t + 256 of the 128 rows x 4 fragments of 8
    uint32_t lab[16];
    uint4 xf[2];

    auto load = [&](long long kb) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long gk = kb + wk0 + j;
            lab[j] = (col_ok && gk < k_hi) ? (uint32_t)labels[gk * ncols + gc] : 0u;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = t + i * HM_THREADS;
            const long long gr = m0 + (f >> 2), gk = kb + (f & 3) * 8;
            xf[i] = make_uint4(0u, 0u, 0u, 0u);
            if (gr < m) {
                if constexpr (XVEC) {   // kdim, k_lo and gk are multiples of 8: the fragment lies wholly before k_hi or wholly past it
                    if (gk < k_hi) xf[i] = *reinterpret_cast<const uint4 *>(x + gr * kdim + gk);
                } else {
                    const unsigned short *xr = reinterpret_cast<const unsigned short *>(x + gr * kdim);
                    uint32_t h[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) h[e] = gk + e < k_hi ? (uint32_t)xr[gk + e] : 0u;
                    xf[i] = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
                }
            }
        }
    };
    auto store = [&](long long kb) {
        V w0, w1;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float v = (col_ok && kb + wk0 + j < k_hi) ? cb[CbTable<LT>::index(lab[j], k, cshift, lane)] : 0.0f;
            if (j < 8) w0[j] = (XT)v;   // exact: the table holds values of XT
            else w1[j - 8] = (XT)v;
        }
        *reinterpret_cast<V *>(ws + wc * HM_LD + wk0) = w0;
        *reinterpret_cast<V *>(ws + wc * HM_LD + wk0 + 8) = w1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = t + i * HM_THREADS;
            *reinterpret_cast<uint4 *>(xs + (f >> 2) * HM_LD + (f & 3) * 8) = xf[i];
        }
    };

    C acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // lane l of a 32x32x16 MFMA holds A[row l & 31][k = 8 (l >> 5) + e] and B[k = 8 (l >> 5) + e][col l & 31], e = 0..7
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, fr = lane & 31, fh = (lane >> 5) * 8;
    load(k_lo);
    for (long long kb = k_lo; kb < k_hi; kb += HM_BK) {
        __syncthreads();   // the table is filled (first step); the images of the step before have been read
        store(kb);
        __syncthreads();
        if (kb + HM_BK < k_hi) load(kb + HM_BK);
#pragma unroll
        for (int s = 0; s < HM_BK; s += 16) {
            V a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const V *>(xs + (wm + i * 32 + fr) * HM_LD + s + fh);
                b[i] = *reinterpret_cast<const V *>(ws + (wn + i * 32 + fr) * HM_LD + s + fh);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = F::mfma(a[i], b[j], acc[i][j]);
        }
    }

    // C / D: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
    float *outf = reinterpret_cast<float *>(out_);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long c = n0 + wn + j * 32 + fr;
            if (c >= ncols) continue;
            const float bv = (direct && bias) ? bias[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row >= m) continue;
                float v = acc[i][j][r];
                if (direct) {
                    if (bias) v += bv;
                    if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
                    if (direct == 2)
                        reinterpret_cast<XT *>(out_)[row * ncols + c] = (XT)v;
                    else
                        outf[row * ncols + c] = v;
                } else {
                    outf[((long long)blockIdx.y * m + row) * ncols + c] = v;
                }
            }
        }
    }
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
static void launch_mfma(bool xvec, dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const void *labels, long long ncols,
                        const float *centers, int k, int entries, int cshift, long long col_tiles, long long rps, const float *bias, int relu, int direct,
                        void *out)
{
    const XT *xp = reinterpret_cast<const XT *>(x);
    const LT *lab = reinterpret_cast<const LT *>(labels);
    if (xvec)
        hipLaunchKernelGGL((k_cbmm_mfma<XT, LT, true>), grid, dim3(HM_THREADS), lds, s, xp, m, kdim, lab, ncols, centers, k, entries, cshift, col_tiles, rps, bias, relu, direct, out);
    else
        hipLaunchKernelGGL((k_cbmm_mfma<XT, LT, false>), grid, dim3(HM_THREADS), lds, s, xp, m, kdim, lab, ncols, centers, k, entries, cshift, col_tiles, rps, bias, relu, direct, out);
}

// every kernel instantiation of this unit; the plan is checked against these tables, and the launches go through them
using StreamLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, int, long long, const void *, long long, const float *, int, int, int,
                              long long, const float *, int, int, void *);
using MfmaLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, long long, long long, const void *, long long, const float *, int, int, int,
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
    if (y_dtype != NNC_DT_F32 && y_dtype != x_dtype) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: y_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: centers is NULL");
    if (m > 0 && ncols > 0 && !y) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: y is NULL");
    if (m > 0 && ncols > 0 && kdim > 0 && (!x || !labels)) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: x or labels is NULL");
    if (reinterpret_cast<uintptr_t>(x) % 2 || reinterpret_cast<uintptr_t>(y) % (y_dtype == NNC_DT_F32 ? 4 : 2))
        return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_h16: x or y is not aligned to its element size");
    const int64_t need = nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace("nnc_cbmm_h16", "nnc_cbmm_h16_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels), true);
    if (p.path == NNC_CBMM_BIAS) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // kdim = 0: y = bias
    rc = have_kernel(p, x_dtype, label_bytes);
    if (rc != NNC_OK) return rc;
    const int direct = p.splits == 1 ? (y_dtype == NNC_DT_F32 ? 1 : 2) : 0;
    void *out = direct ? y : workspace;
    if (p.path == NNC_CBMM_STREAM) {
        const dim3 grid((unsigned)p.col_tiles, (unsigned)p.splits);
        find_stream(x_dtype, label_bytes, p.vb, p.mt)(p.aligned != 0, grid, (size_t)p.lds, s, x, (int)m, kdim, labels, ncols, centers_dev, k, p.entries,
                                                      p.cshift, p.rows_per_split, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbmm_stream (h16)");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        const bool xvec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && kdim % 8 == 0;
        find_mfma(x_dtype, label_bytes)(xvec, grid, (size_t)p.lds, s, x, m, kdim, labels, ncols, centers_dev, k, p.entries, p.cshift, p.col_tiles,
                                        p.rows_per_split, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbmm_mfma");
    }
    if (!direct) return cbmm_reduce_dt(reinterpret_cast<const float *>(workspace), p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
    return NNC_OK;
}
