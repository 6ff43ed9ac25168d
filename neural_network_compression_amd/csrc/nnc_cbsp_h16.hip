// nnc_cbsp_h16.hip -- the bitmap-sparse codebook matmul of nnc_cbsp.hip on bf16 / fp16 activations (include/nnc_cbsp_h16.h,
// nnc_cbsp_h16): y = x @ W_h + bias, W_h[i, o] = the centre of labels[i, o] rounded to x's type, the label of a
// skipped position being zero_symbol.  A product of two bf16 or two fp16 values is exact in float32; every sum is float32.
//
//   k_cbsp_stream<XT>  m <= 16: nnc_cbsp.hpp's stream kernel with x read as XT and widened and the d table built from the rounded
//                      centres widened: the float32 path's fmaf chain (and its plan, sp_plan) on half the x bytes.  A skipped weight
//                      stays absent when rn(c_z) == 0.  k_cbsp_reduce<XT, YT> combines its splits.
//   k_cbsp_mfma        m > 16: k_cbmm_mfma's tile and k loop (nnc_cbmfma.hpp), table (cb_fill<XT>, the per-bank copies) and plan
//                      (cb_plan's half plan), with the label of a thread's 16 k rows of its column decoded from the form by
//                      SpTileDecode (nnc_cbsp.hpp): a wave owns one 64-column segment, 16 lanes load one row's word and count each,
//                      v_readlane broadcasts them, a lane's symbol sits at count + v_mbcnt(word).  A skipped position takes the
//                      table entry of zero_symbol: W_h holds c_z there, no rank-1 term, no row sums.  The words and counts run two
//                      k steps ahead of the MFMAs (the loop's `ahead`), the symbols and x one.  Everything past kdim (or past the
//                      split), past m and past ncols is zero in both images, never memory; no load leaves the packed buffer.
//                      k_cbmm_reduce combines the splits: y is nnc_cbmm_h16's on the unpacked labels bit for bit.
#include "nnc_cbsp.hpp"

// grid (col_tiles * row_tiles, splits), HM_THREADS threads; out, direct and rows_per_split as k_cbmm_mfma
template <typename XT, typename LT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbsp_mfma(const XT *__restrict__ x, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                          const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const LT *__restrict__ sym,
                                                          long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                          int z, int entries, int cshift, long long col_tiles, long long rows_per_split,
                                                          const float *__restrict__ bias, int relu, int direct, void *__restrict__ out_)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, entries, cshift);
    cb_fill<XT>(L.cb, L.stage, centers, k, entries, cshift);

    const HmTile T = hm_tile(col_tiles, rows_per_split, kdim);
    const bool col_ok = T.n0 + T.wc < ncols;
    SpTileDecode<LT> D(bitmap, lo, hi, sym, nnz, segs, T);
    uint32_t lab[16];

    auto load_w = [&](long long) { D.decode((uint32_t)z, lab); };   // the step whose words load_words brought last
    auto store_w = [&](long long kb) {
        hm_lookup_w(L.ws, L.cb, T, col_ok, kb, lab, [&](uint32_t l) { return CbTable<LT>::index(l, k, cshift, T.lane); });
    };

    typename HFrag<XT>::C acc[2][2];
    D.load_words(T.k_lo);
    hm_accumulate<XT, XVEC>(x, m, kdim, T, L.xs, L.ws, acc, load_w, store_w, [&](long long kb) { D.load_words(kb + HM_BK); });
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, ncols, bias, relu, direct, out_);
}

// ------------------------------------------------------------------ launches
struct SpForm {   // the parts of the packed buffer
    const uint64_t *bitmap;
    const uint32_t *lo, *hi;
    const void *sym;
    long long nnz, segs;
};

template <typename XT, typename LT, int MT>
static void launch_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, int m, long long kdim, const SpForm &f, long long ncols, const float *centers,
                          int k, int z, int entries, int cshift, long long rps, const float *bias, int relu, int direct, void *out, float *rs_out)
{
    hipLaunchKernelGGL((k_cbsp_stream<XT, LT, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), m, kdim, f.bitmap, f.lo, f.hi,
                       reinterpret_cast<const LT *>(f.sym), f.nnz, ncols, f.segs, centers, k, z, entries, cshift, rps, bias, relu, direct, out, rs_out);
}

template <typename XT, typename LT>
static void launch_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const SpForm &f, long long ncols,
                        const float *centers, int k, int z, int entries, int cshift, long long col_tiles, long long rps, const float *bias, int relu,
                        int direct, void *out)
{
    hm_launch(x, kdim, k_cbsp_mfma<XT, LT, true>, k_cbsp_mfma<XT, LT, false>, grid, lds, s, reinterpret_cast<const XT *>(x), m, kdim, f.bitmap, f.lo, f.hi,
              reinterpret_cast<const LT *>(f.sym), f.nnz, ncols, f.segs, centers, k, z, entries, cshift, col_tiles, rps, bias, relu, direct, out);
}

// k_cbsp_reduce for the stream path's splits: c_z rounded to XT, y float32 or XT
template <typename XT>
static void launch_reduce(int rgrid, hipStream_t s, const float *part, long long splits, long long m, long long ncols, const float *rsp, long long rsplits,
                          const float *centers, int k, int z, const float *bias, int relu, void *y, int y_dtype)
{
    if (y_dtype == NNC_DT_F32)
        hipLaunchKernelGGL((k_cbsp_reduce<XT, float>), dim3(rgrid), dim3(256), 0, s, part, splits, m, ncols, rsp, rsplits, centers, k, z, bias, relu,
                           reinterpret_cast<float *>(y));
    else
        hipLaunchKernelGGL((k_cbsp_reduce<XT, XT>), dim3(rgrid), dim3(256), 0, s, part, splits, m, ncols, rsp, rsplits, centers, k, z, bias, relu,
                           reinterpret_cast<XT *>(y));
}

// every kernel instantiation of this unit; the plan is checked against these tables, and the launches go through them
using StreamLaunch = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const SpForm &, long long, const float *, int, int, int, int, long long,
                              const float *, int, int, void *, float *);
using MfmaLaunch = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const SpForm &, long long, const float *, int, int, int, int,
                            long long, long long, const float *, int, int, void *);
struct StreamCase {
    int dt, lb, mt;
    StreamLaunch fn;
};
struct MfmaCase {
    int dt, lb;
    MfmaLaunch fn;
};
#define SP_H16_STREAM_CASES(DT, XT)                                                                                                     \
    {DT, 1, 1, launch_stream<XT, uint8_t, 1>}, {DT, 1, 2, launch_stream<XT, uint8_t, 2>}, {DT, 1, 4, launch_stream<XT, uint8_t, 4>},    \
    {DT, 1, 8, launch_stream<XT, uint8_t, 8>}, {DT, 1, 16, launch_stream<XT, uint8_t, 16>}, {DT, 2, 1, launch_stream<XT, uint16_t, 1>}, \
    {DT, 2, 2, launch_stream<XT, uint16_t, 2>}, {DT, 2, 4, launch_stream<XT, uint16_t, 4>}, {DT, 2, 8, launch_stream<XT, uint16_t, 8>}, \
    {DT, 2, 16, launch_stream<XT, uint16_t, 16>}
static const StreamCase kStreamCases[] = {SP_H16_STREAM_CASES(NNC_DT_BF16, bf16_t), SP_H16_STREAM_CASES(NNC_DT_F16, f16_t)};
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 1, launch_mfma<bf16_t, uint8_t>}, {NNC_DT_BF16, 2, launch_mfma<bf16_t, uint16_t>},
    {NNC_DT_F16, 1, launch_mfma<f16_t, uint8_t>},   {NNC_DT_F16, 2, launch_mfma<f16_t, uint16_t>},
};

static StreamLaunch find_stream(int dt, int lb, int mt)
{
    for (const StreamCase &c : kStreamCases)
        if (c.dt == dt && c.lb == lb && c.mt == mt) return c.fn;
    return nullptr;
}

static MfmaLaunch find_mfma(int dt, int lb)
{
    for (const MfmaCase &c : kMfmaCases)
        if (c.dt == dt && c.lb == lb) return c.fn;
    return nullptr;
}

static int no_stream_case(int dt, int lb, int mt)
{
    return fail(NNC_EINVAL, "nnc_cbsp_h16: no k_cbsp_stream instantiation for dtype " + std::to_string(dt) + ", label_bytes " + std::to_string(lb) + ", mt " +
                                std::to_string(mt));
}

static int no_mfma_case(int dt, int lb)
{
    return fail(NNC_EINVAL, "nnc_cbsp_h16: no k_cbsp_mfma instantiation for dtype " + std::to_string(dt) + ", label_bytes " + std::to_string(lb));
}

// ------------------------------------------------------------------ C ABI
static int h16_check(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16) return fail(NNC_EINVAL, "nnc_cbsp_h16: x_dtype must be NNC_DT_BF16 or NNC_DT_F16");
    if (m < 0 || kdim < 0 || ncols < 0) return fail(NNC_EINVAL, "nnc_cbsp_h16: negative size");
    if (label_bytes != 1 && label_bytes != 2) return fail(NNC_EINVAL, "nnc_cbsp_h16: label_bytes must be 1 or 2");
    if (!sp_size_ok(kdim, ncols) || m > (1LL << 40))
        return fail(NNC_EINVAL, "nnc_cbsp_h16: size too large (m <= 2^40, ncols < 2^32, kdim * ceil(ncols / 64) <= 2^40)");
    if (k < 1 || k > NNC_KMAX) return fail(NNC_EINVAL, "nnc_cbsp_h16: k outside 1..NNC_KMAX");
    if (label_bytes == 1 && k > 256) return fail(NNC_EINVAL, "nnc_cbsp_h16: k > 256 needs 2-byte labels");
    return NNC_OK;
}

// m <= 16 follows sp_plan (its stream plan), m > 16 cb_plan's half plan
static bool h16_skinny(int64_t m) { return m <= CB_SKINNY_M; }

extern "C" int64_t nnc_cbsp_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || h16_check(NNC_DT_BF16, m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    if (h16_skinny(m)) return sp_ws_bytes(sp_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS), m, ncols);
    return cb_ws_bytes(cb_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS, 0, true), m, ncols);
}

extern "C" int nnc_cbsp_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out)
{
    int rc = h16_check(x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbsp_h16_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbsp_h16_plan: out is NULL");
    if (h16_skinny(m)) {
        const SpPlan p = sp_plan(m, kdim, ncols, label_bytes, k, cus);
        if (p.path == NNC_CBMM_STREAM && !find_stream(x_dtype, label_bytes, p.mt)) return no_stream_case(x_dtype, label_bytes, p.mt);
        const int64_t v[NNC_CBSP_H16_PLAN_LEN] = {p.path, p.mt, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : 0, p.entries, p.splits, p.rows_per_split,
                                                  p.rowsum, p.lds, p.col_tiles, p.row_tiles, sp_ws_bytes(p, m, ncols), x_dtype};
        std::copy(v, v + NNC_CBSP_H16_PLAN_LEN, out);
        return NNC_OK;
    }
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cus, 0, true);
    if (p.path == NNC_CBMM_MFMA && !find_mfma(x_dtype, label_bytes)) return no_mfma_case(x_dtype, label_bytes);
    const int64_t v[NNC_CBSP_H16_PLAN_LEN] = {p.path, p.mt, p.entries ? 1LL << p.cshift : 0, p.entries, p.splits, p.rows_per_split, NNC_CBSP_ROWSUM_NONE,
                                              p.lds, p.col_tiles, p.row_tiles, cb_ws_bytes(p, m, ncols), x_dtype};
    std::copy(v, v + NNC_CBSP_H16_PLAN_LEN, out);
    return NNC_OK;
}

extern "C" int nnc_cbsp_h16(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes, int64_t ncols,
                            int32_t zero_symbol, int64_t nnz, const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, void *y, int y_dtype,
                            void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = h16_check(x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if ((rc = sp_check_z("nnc_cbsp_h16", zero_symbol, label_bytes)) != NNC_OK) return rc;
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, "nnc_cbsp_h16: nnz outside 0..kdim * ncols");
    const SpLayout L = sp_layout(kdim, ncols, label_bytes, nnz);
    if (packed_bytes < L.bytes) return fail(NNC_EINVAL, "nnc_cbsp_h16: packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, label_bytes, nnz)");
    if ((rc = cb_check_operands("nnc_cbsp_h16", x, x_dtype, y, y_dtype, centers_dev, m, kdim, ncols, !x || !packed, "x or packed")) != NNC_OK) return rc;
    if (m > 0 && ncols > 0 && kdim > 0 && reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, "nnc_cbsp_h16: packed must be 256-byte aligned");
    const int64_t need = nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, label_bytes);
    rc = cb_check_workspace("nnc_cbsp_h16", "nnc_cbsp_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned");
    if (rc != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    const SpForm f = {reinterpret_cast<const uint64_t *>(base), reinterpret_cast<const uint32_t *>(base + L.off_lo),
                      reinterpret_cast<const uint32_t *>(base + L.off_hi), base + L.off_sym, nnz, L.segs};
    if (!h16_skinny(m)) {
        const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cu_count(), 0, true);
        if (p.path == NNC_CBMM_BIAS) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // kdim = 0: y = bias, as nnc_cbmm_h16
        const MfmaLaunch fn = find_mfma(x_dtype, label_bytes);
        if (!fn) return no_mfma_case(x_dtype, label_bytes);
        const int direct = cb_direct(p.splits, y_dtype);
        fn(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, m, kdim, f, ncols, centers_dev, k, zero_symbol, p.entries,
           p.cshift, p.col_tiles, p.rows_per_split, bias_dev, relu, direct, direct ? y : workspace);
        LAUNCHCHK("k_cbsp_mfma");
        return cb_finish(direct, workspace, p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
    }

    const SpPlan p = sp_plan(m, kdim, ncols, label_bytes, k, cu_count());
    const int rgrid = (int)std::max(1LL, std::min(cdiv(mn, 64), 8192LL));
    float *part = reinterpret_cast<float *>(workspace);
    float *rsp = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sp_part_bytes(p, m, ncols));
    const int direct = cb_direct(p.splits, y_dtype);   // 0 where kdim = 0: the plan then has no split at all
    if (p.path == NNC_CBMM_STREAM) {
        const StreamLaunch fn = find_stream(x_dtype, label_bytes, p.mt);
        if (!fn) return no_stream_case(x_dtype, label_bytes, p.mt);
        fn(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, f, ncols, centers_dev, k, zero_symbol, p.entries, p.cshift,
           p.rows_per_split, bias_dev, relu, direct, direct ? y : (void *)part, direct ? nullptr : rsp);
        LAUNCHCHK("k_cbsp_stream (h16)");
        if (direct) return NNC_OK;
    }
    // the splits in split order, as nnc_cbsp_f32 ends (kdim = 0: the plan has no split and no row sum, so y = bias)
    (x_dtype == NNC_DT_BF16 ? launch_reduce<bf16_t> : launch_reduce<f16_t>)(rgrid, s, part, p.splits, m, ncols, rsp, sp_rsplits(p), centers_dev, k, zero_symbol,
                                                                            bias_dev, relu, y, y_dtype);
    LAUNCHCHK("k_cbsp_reduce (h16)");
    return NNC_OK;
}
