// nnc_cbmm.hip -- the quantized layer run from its codebook and centroid indices: y[m, ncols] = x[m, kdim] @ W + bias (then
// ReLU if asked), W[i, o] = centers[labels[i * ncols + o]], the fp32 W never stored (include/nnc.h, nnc_cbmm_f32).
//
// Two regimes ("Running the compressed layer"); the plan and k_cbmm_stream are in nnc_cbmm.hpp, shared with the
// bf16 / fp16 unit nnc_cbmm_h16.hip:
//   k_cbmm_stream  m <= 16: bound by the index stream.  A wave owns 64 lanes x VB bytes of a label row (VB = 16, 8 or 4: the
//                  widest load that keeps the m x (VB / label_bytes) accumulators of a lane within 64 registers), loaded straight
//                  to VGPRs, CB_UNROLL rows in flight; x[r, i] is uniform over the wave (vector load + v_readlane).  The codebook sits in LDS
//                  with one copy per bank: entry j of lane l at word j * C + (l mod C), C = 32 where it fits (K <= 256: every
//                  lane always hits its own bank, 2 LDS cycles per 64 lookups), fewer copies for K > 256.  The 4 waves of a
//                  workgroup split its rows and are summed in LDS in wave order; workgroups split K.
//   k_cbmm_tiled   m > 16: bound by compute.  128 x 128 output tiles, the W tile dequantized from its indices into LDS once per
//                  workgroup and reused by all 128 rows of x (register-blocked FMA, 8 x 8 outputs per thread).  The kernel is
//                  the decode; the tile coordinates, the x tile load and the store are nnc_cbtile.hpp's, as for every tiled
//                  kernel of the other forms.
//   k_cbmm_reduce  the split-K partials summed in split order, + bias, ReLU.  No float atomics anywhere: the number of splits
//                  depends only on the shape and the CU count, so the same call gives the same bits.
// Label rows need not be aligned (any ncols, any storage offset): a lane loads the two aligned VB-byte chunks around its window
// and funnel-shifts them (v_alignbyte) by the row's misalignment, which is uniform over the wave.  An aligned chunk that holds
// one byte of the tensor lies in the tensor's page, so no load leaves the allocation; lanes past the last column load their
// row's first chunk and store nothing.  An index >= K reads 0, as nnc_gather_f32 does.
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ tiled: m > 16
// grid (col_tiles * row_tiles, splits), 256 threads; thread (tx, ty) = (t % 16, t / 16) owns rows ty*8.. and columns tx*8.. of
// the 128 x 128 tile.
template <typename LT>
__global__ __launch_bounds__(256) void k_cbmm_tiled(const float *__restrict__ x, long long m, long long kdim, const LT *__restrict__ labels, long long ncols,
                                                    const float *__restrict__ centers, int k, long long col_tiles, long long rows_per_split,
                                                    const float *__restrict__ bias, int relu, int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // k + 1 entries (entry k = 0)
    for (int j = threadIdx.x; j <= k; j += 256) cb[j] = j < k ? centers[j] : 0.0f;

    const TbTile T = tb_tile(col_tiles, rows_per_split, kdim);
    float acc[8][8];
    tb_clear(acc);

    const int wk = threadIdx.x >> 5, wc = (threadIdx.x & 31) * 4;      // W tile: k wk, columns wc..wc+3
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        __syncthreads();
        tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long gc = T.n0 + wc + j;
            float v = 0.0f;
            if (gk < T.hi && gc < ncols) v = cb[std::min((uint32_t)labels[gk * ncols + gc], (uint32_t)k)];
            ws[wk * TB_N + wc + j] = v;
        }
        __syncthreads();
        tb_tile_fma(xs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_y(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, ncols, bias, relu, direct, out);
}

// ------------------------------------------------------------------ split-K combine
// y = ((q0 + q1) + q2) + q3 + bias, q = the in-order sum of a quarter of the splits: 64 outputs per workgroup, a quarter per wave
// (one thread per output summing all splits serially was 25-37 us at m = 1 with ~100 splits).  The order depends on `splits` only.
// OT = float, or bf16_t / f16_t for nnc_cbmm_h16: the float32 value rounded once.
#define RED_Q 4
template <typename OT>
__global__ __launch_bounds__(256) void k_cbmm_reduce(const float *__restrict__ part, long long splits, long long mn, long long ncols,
                                                     const float *__restrict__ bias, int relu, OT *__restrict__ y)
{
    __shared__ float qs[RED_Q - 1][64];
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long per_q = (splits + RED_Q - 1) / RED_Q;
    const long long s0 = std::min(splits, q * per_q), s1 = std::min(splits, s0 + per_q);
    for (long long base = (long long)blockIdx.x * 64; base < mn; base += (long long)gridDim.x * 64) {
        const long long idx = base + o;
        float v = 0.0f;
        if (idx < mn) {
#pragma unroll 8
            for (long long s = s0; s < s1; ++s) v += part[s * mn + idx];
        }
        __syncthreads();
        if (q > 0) qs[q - 1][o] = v;
        __syncthreads();
        if (q == 0 && idx < mn) {
#pragma unroll
            for (int j = 0; j < RED_Q - 1; ++j) v += qs[j][o];
            if (bias) v += bias[idx % ncols];
            if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
            y[idx] = (OT)v;
        }
    }
}

int cbmm_reduce_dt(const float *part, long long splits, long long mn, long long ncols, const float *bias, int relu, void *y, int y_dtype, hipStream_t s)
{
    const int rgrid = (int)std::max(1LL, std::min(cdiv(mn, 64), 8192LL));
    if (y_dtype == NNC_DT_F32)
        hipLaunchKernelGGL(k_cbmm_reduce<float>, dim3(rgrid), dim3(256), 0, s, part, splits, mn, ncols, bias, relu, reinterpret_cast<float *>(y));
    else if (y_dtype == NNC_DT_BF16)
        hipLaunchKernelGGL(k_cbmm_reduce<bf16_t>, dim3(rgrid), dim3(256), 0, s, part, splits, mn, ncols, bias, relu, reinterpret_cast<bf16_t *>(y));
    else if (y_dtype == NNC_DT_F16)
        hipLaunchKernelGGL(k_cbmm_reduce<f16_t>, dim3(rgrid), dim3(256), 0, s, part, splits, mn, ncols, bias, relu, reinterpret_cast<f16_t *>(y));
    else
        return fail(NNC_EINVAL, "k_cbmm_reduce: no instantiation for output dtype " + std::to_string(y_dtype));
    LAUNCHCHK("k_cbmm_reduce");
    return NNC_OK;
}

int cbmm_reduce(const float *part, long long splits, long long mn, long long ncols, const float *bias, int relu, float *y, hipStream_t s)
{
    return cbmm_reduce_dt(part, splits, mn, ncols, bias, relu, y, NNC_DT_F32, s);
}

// ------------------------------------------------------------------ C ABI
static int cb_check(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (m < 0 || kdim < 0 || ncols < 0) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: negative size");
    if (label_bytes != 1 && label_bytes != 2) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: label_bytes must be 1 or 2");
    if (k < 1 || k > NNC_KMAX) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: k outside 1..NNC_KMAX");
    if (label_bytes == 1 && k > 256) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: k > 256 needs 2-byte labels");
    if (m > (1LL << 40) || kdim > (1LL << 40) || ncols > (1LL << 40)) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: size too large");
    return NNC_OK;
}

extern "C" int64_t nnc_cbmm_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || (label_bytes != 1 && label_bytes != 2) || cb_check(m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    return cb_ws_bytes(cb_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS, 0), m, ncols);
}

template <typename LT, int VB, int MT>
static void launch_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const float *x, int m, long long kdim, const void *labels, long long ncols,
                          const float *centers, int k, int entries, int cshift, long long rps, const float *bias, int relu, int direct, float *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (aligned)
        hipLaunchKernelGGL((k_cbmm_stream<float, LT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, lab, ncols, centers, k, entries, cshift, rps, bias, relu, direct, out);
    else
        hipLaunchKernelGGL((k_cbmm_stream<float, LT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, lab, ncols, centers, k, entries, cshift, rps, bias, relu, direct, out);
}

// every k_cbmm_stream instantiation there is; the plan is checked against this table, and the launch goes through it
using StreamLaunch = void (*)(bool, dim3, size_t, hipStream_t, const float *, int, long long, const void *, long long, const float *, int, int, int,
                              long long, const float *, int, int, float *);
struct StreamCase {
    int lb, vb, mt;
    StreamLaunch fn;
};
static const StreamCase kStreamCases[] = {
    {1, 16, 1, launch_stream<uint8_t, 16, 1>},  {1, 16, 2, launch_stream<uint8_t, 16, 2>},  {1, 16, 4, launch_stream<uint8_t, 16, 4>},
    {1, 8, 8, launch_stream<uint8_t, 8, 8>},    {1, 4, 16, launch_stream<uint8_t, 4, 16>},
    {2, 16, 1, launch_stream<uint16_t, 16, 1>}, {2, 16, 2, launch_stream<uint16_t, 16, 2>}, {2, 16, 4, launch_stream<uint16_t, 16, 4>},
    {2, 16, 8, launch_stream<uint16_t, 16, 8>}, {2, 8, 16, launch_stream<uint16_t, 8, 16>},
};

static StreamLaunch find_stream(int lb, int vb, int mt)
{
    for (const StreamCase &c : kStreamCases)
        if (c.lb == lb && c.vb == vb && c.mt == mt) return c.fn;
    return nullptr;
}

static int no_stream_case(int lb, int vb, int mt)
{
    return fail(NNC_EINVAL, "nnc_cbmm: no k_cbmm_stream instantiation for label_bytes " + std::to_string(lb) + ", vb " + std::to_string(vb) +
                                ", mt " + std::to_string(mt));
}

static int dispatch_stream(const CbPlan &p, int lb, dim3 grid, hipStream_t s, const float *x, int m, long long kdim, const void *labels, long long ncols,
                           const float *centers, int k, const float *bias, int relu, int direct, float *out)
{
    const StreamLaunch fn = find_stream(lb, p.vb, p.mt);
    if (!fn) return no_stream_case(lb, p.vb, p.mt);
    fn(p.aligned != 0, grid, (size_t)p.lds, s, x, m, kdim, labels, ncols, centers, k, p.entries, p.cshift, p.rows_per_split, bias, relu, direct, out);
    return NNC_OK;
}

extern "C" int nnc_cbmm_plan(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr, int64_t *out)
{
    const int rc = cb_check(m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_plan: cus < 1");
    if (!out) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_plan: out is NULL");
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cus, (uintptr_t)labels_addr);
    if (p.path == NNC_CBMM_STREAM && !find_stream(label_bytes, p.vb, p.mt)) return no_stream_case(label_bytes, p.vb, p.mt);
    const int64_t v[NNC_CBMM_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries,
                                          p.splits, p.rows_per_split, p.aligned, p.lds, p.col_tiles, p.row_tiles, cb_ws_bytes(p, m, ncols)};
    for (int i = 0; i < NNC_CBMM_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_f32(const float *x, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols, const float *centers_dev,
                            int32_t k, const float *bias_dev, int32_t relu, float *y, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = cb_check(m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (!centers_dev) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: centers is NULL");
    if (m > 0 && ncols > 0 && !y) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: y is NULL");
    if (m > 0 && ncols > 0 && kdim > 0 && (!x || !labels)) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: x or labels is NULL");
    const int64_t need = nnc_cbmm_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace("nnc_cbmm_f32", "nnc_cbmm_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    if (p.path == NNC_CBMM_BIAS) {   // kdim = 0: y = bias (zeros without one)
        return cbmm_reduce(nullptr, 0, mn, ncols, bias_dev, relu, y, s);
    }
    const int direct = p.splits == 1;
    float *out = direct ? y : reinterpret_cast<float *>(workspace);
    if (p.path == NNC_CBMM_STREAM) {
        const dim3 grid((unsigned)p.col_tiles, (unsigned)p.splits);
        rc = dispatch_stream(p, label_bytes, grid, s, x, (int)m, kdim, labels, ncols, centers_dev, k, bias_dev, relu, direct, out);
        if (rc != NNC_OK) return rc;
        LAUNCHCHK("k_cbmm_stream");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        if (label_bytes == 1)
            hipLaunchKernelGGL(k_cbmm_tiled<uint8_t>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, reinterpret_cast<const uint8_t *>(labels),
                               (long long)ncols, centers_dev, (int)k, p.col_tiles, p.rows_per_split, bias_dev, (int)relu, direct, out);
        else
            hipLaunchKernelGGL(k_cbmm_tiled<uint16_t>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, reinterpret_cast<const uint16_t *>(labels),
                               (long long)ncols, centers_dev, (int)k, p.col_tiles, p.rows_per_split, bias_dev, (int)relu, direct, out);
        LAUNCHCHK("k_cbmm_tiled");
    }
    if (!direct) {
        return cbmm_reduce(reinterpret_cast<const float *>(workspace), p.splits, mn, ncols, bias_dev, relu, y, s);
    }
    return NNC_OK;
}
