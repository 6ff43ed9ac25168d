// nnc_cbspgrad_h16.hip -- the backward pass of nnc_cbsp_h16 (nnc_cbsp_h16.hip) from the same packed form: the bitmap-sparse codebook
// layer trained on bf16 / fp16 activations (include/nnc_cbspgrad_h16.h, nnc_cbsp_dx_h16 / nnc_cbsp_dc_h16).
// W_h[i, o] = the centre of label[i, o] rounded to the type of g, the label of a skipped position being zero_symbol: the forward's W_h.
// A product of two bf16 or two fp16 values is exact in float32, every sum is float32, dc is binned as section 12's exact integers.
//
//   m <= 16   k_cbspdx_stream<XT> / k_cbspdc_stream<XT> of nnc_cbspgrad.hpp: section 13's stream plan and kernels with g and x widened
//             as they are loaded and, for dx, the d table of the rounded centres (sp_fill<XT>).  dx: the row sums of g
//             (k_cbsp_rowsum<XT>) come first; the rank-1 term c_z * rs is added in float32 before the one rounding of a half dx, by
//             the stream kernel itself where a single column block writes dx, by k_cbspdx_finish behind the split partials.  Bit
//             for bit the float32 entry points on the widened inputs.
//   k_cbspdx_mfma  m > 16.  k_cbdx_mfma's tile, table, main loop (hm_accumulate, nnc_cbmfma.hpp), tiles and splits (nnc_cbh16plan.hpp);
//             g is the A operand.  The B operand W^T is
//             decoded from the form: thread t owns index row n0 + (t mod 128) and 16 consecutive o of the step, which are 16 aligned
//             bits of one bitmap word; their stored symbols are one run of the symbol stream starting at the segment's count plus
//             the popcount of the word below the 16 bits.  A skipped position takes the table entry of zero_symbol, so there is no
//             rank-1 term and no row sum on this path.  The word and the count of a step are requested two steps ahead of the MFMAs
//             that consume them, the symbols and g one.
//   k_cbspdc_mfma  m > 16.  k_cbdc_mfma's main loop (dcm_accumulate, nnc_cbgrad_h16.hpp), so the same accumulators; the epilogue takes an
//             accumulator's label from the bitmap word of its row and segment, the count and a popcount.  A stored weight's image
//             goes into the replicated LDS bins, a skipped one's into a per-lane int64 register flushed into bin z once.
// No load leaves the packed buffer: rows past kdim load no word, columns past the split none, a symbol is loaded only below nnz.
// Everything past m, kdim, ncols and the end of a split is zero in the images, never memory.  No float atomics; no host read.
#include "nnc_cbgrad_h16.hpp"
#include "nnc_cbh16plan.hpp"
#include "nnc_cbspgrad.hpp"

// ------------------------------------------------------------------ dx, m <= 16
// the split partials summed in split order (as k_cbgrad_reduce sums them), then + c_z * rs (as k_cbspdx_rank1 adds it), then the
// one rounding to OT
template <typename RT, typename OT>
__global__ __launch_bounds__(256) void k_cbspdx_finish(const float *__restrict__ part, long long splits, long long m, long long kdim,
                                                       const float *__restrict__ rs, const float *__restrict__ centers, int k, int z, OT *__restrict__ dx)
{
    const float cz = sp_cz<RT>(centers, k, z);
    const long long mn = m * kdim;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < mn; idx += (long long)gridDim.x * blockDim.x) {
        float v = part[idx];
        for (long long s = 1; s < splits; ++s) v += part[s * mn + idx];
        if (cz != 0.0f) v = cz * rs[idx / kdim] + v;
        dx[idx] = (OT)v;
    }
}

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads; out, direct and cols_per_split as k_cbdx_mfma
template <typename XT, typename LT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbspdx_mfma(const XT *__restrict__ g, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                            const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const LT *__restrict__ sym,
                                                            long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                            int z, int entries, int cshift, long long col_tiles, long long cols_per_split, int direct,
                                                            void *__restrict__ out_)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    float *cb = hm_smem;                                // entries << cshift
    float *stage = cb + (entries << cshift);            // entries
    XT *gs = reinterpret_cast<XT *>(hm_smem + hm_table_words(entries, cshift));   // [HM_BM][HM_LD]: g tile, row-major in o
    XT *ws = gs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: W^T tile, [i][o]
    cb_fill<XT>(cb, stage, centers, k, entries, cshift);

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);   // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const long long gi = T.n0 + T.wc;
    const bool row_ok = gi < kdim;
    const long long wrow = gi * segs;
    uint32_t lo0 = 0, hrow = 0;                         // the row's own count: lo[i * segs], hi[i]
    if (row_ok) {
        lo0 = lo[wrow];
        hrow = hi[gi];
    }
    uint64_t word = 0;                                  // of the step load_w() decodes next
    long long cnt = 0;
    uint32_t lab[16];

    // the word holding columns ob + wk0 .. + 15 and the count of its segment; rows past kdim and columns past the split load nothing
    auto load_words = [&](long long ob) {
        const long long o0 = ob + T.wk0;
        word = 0;
        cnt = 0;
        if (row_ok && o0 < T.k_hi) {
            const long long sg = o0 >> 6;
            word = bitmap[wrow + sg];
            cnt = sp_count(lo[wrow + sg], lo0, hrow);
        }
    };
    auto load_w = [&](long long ob) {                   // from the word load_words(ob) brought
        const int b0 = (int)((ob + T.wk0) & 63);        // 0, 16, 32 or 48: steps and splits are multiples of 32
        const uint32_t bits = (uint32_t)(word >> b0) & 0xFFFFu;
        const long long start = cnt + __popcll(word & ((1ULL << b0) - 1));
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long pos = start + __popc(bits & ((1u << j) - 1));
            lab[j] = (uint32_t)z;                       // a skipped position (every position of an empty word)
            if (((bits >> j) & 1u) && pos < nnz) lab[j] = (uint32_t)sym[pos];
        }
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? cb[CbTable<LT>::index(lab[j], k, cshift, T.lane)] : 0.0f;
        hm_store_w(ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    load_words(T.k_lo);
    hm_accumulate<XT, XVEC>(g, m, ncols, T, gs, ws, acc, load_w, store_w, [&](long long ob) { load_words(ob + HM_BK); });
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads; LDS, rows_per_split and XVEC as k_cbdc_mfma
template <typename XT, typename LT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbspdc_mfma(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                            const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo,
                                                            const uint32_t *__restrict__ hi, const LT *__restrict__ sym, long long nnz, long long ncols,
                                                            long long segs, int k, int z, int rlog2, int terms_log2, long long col_tiles,
                                                            long long rows_per_split, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
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

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col): the 32 lanes of a row lie in the wave's one segment (n0 + wn is a
    // multiple of 64), so one word and one count serve each half of the wave for both b; a lane's label is the symbol at count +
    // popcount(word below its column)
    const int rep = T.t & ((1 << rlog2) - 1);
    const long long sg = (T.n0 + T.wn) >> 6;
    const bool seg_ok = sg < segs;                      // (else every column of the wave lies past ncols)
    unsigned long long skip = 0;                        // the images of the lane's skipped weights: bin z
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long i = hm_acc_row(T.m0 + T.wm, a, r, T.lane);
            if (i >= kdim || !seg_ok) continue;
            const long long wrow = i * segs;
            const uint64_t word = bitmap[wrow + sg];
            const long long cnt = sp_count(lo[wrow + sg], lo[wrow], hi[i]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int c = (int)hm_acc_col(0, b, T.lane);   // the lane's column inside the segment
                if (T.n0 + T.wn + c >= ncols) continue;
                const unsigned long long img = cbdc_fix(acc[a][b][r], Sw);
                const long long pos = cnt + __popcll(word & ((1ULL << c) - 1));
                if (((word >> c) & 1) && pos < nnz) {   // (a symbol past nnz: skipped, as nnc_cbsp_unpack reads it)
                    const uint32_t l = (uint32_t)sym[pos];
                    if (l < (uint32_t)k) atomicAdd(&bins[(l << rlog2) + rep], img);
                } else {
                    skip += img;
                }
            }
        }
    }
    if (z < k && skip) atomicAdd(&bins[((uint32_t)z << rlog2) + rep], skip);
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ plans (host)
// m <= 16 and the empty shapes: section 13's plans (sg_dx_plan, sg_dc_plan) field for field.  m > 16: nnc_cbh16plan.hpp's tiles and
// splits with the byte form's table and bins, so the tiles, the splits, S and every image are those of nnc_cbmm_dx_h16 /
// nnc_cbmm_dc_h16 on the same shape.
static SgPlan h16_dx_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return sg_dx_plan(m, kdim, ncols, lb, k, cus);
    int entries = 0, cshift = 0;   // (cb_table_shape counts cshift up from 0)
    cb_table_shape(lb, k, entries, cshift);
    SgPlan p = h16_mfma_plan<SgPlan>(h16_dx_tiles(m, kdim, ncols), (long long)hm_table_words(entries, cshift) * 4);
    p.entries = entries, p.cshift = cshift;
    return p;
}

static int64_t h16_dx_ws_bytes(const SgPlan &p, long long m, long long kdim)
{
    return p.path == NNC_CBMM_MFMA ? cbg_dx_ws_bytes(p.splits, m, kdim) : sg_dx_ws_bytes(p, m, kdim);
}

static int h16_dc_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus, SgPlan &p)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return sg_dc_plan(m, kdim, ncols, lb, k, cus, p);
    p = h16_mfma_plan<SgPlan>(h16_dc_tiles(m, kdim, ncols), ((long long)k << dc_rlog2(k)) * 8);
    p.rlog2 = dc_rlog2(k);
    return NNC_OK;
}

// ------------------------------------------------------------------ launches
struct SgForm {   // the parts of the packed buffer
    const uint64_t *bitmap;
    const uint32_t *lo, *hi;
    const void *sym;
    long long nnz, segs;
};

template <typename XT, typename LT, int MT>
static void launch_dx_stream(dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const SgForm &f, long long ncols, const float *centers,
                             int k, int z, const SgPlan &p, int direct, void *out, const float *rs)
{
    hipLaunchKernelGGL((k_cbspdx_stream<XT, LT, MT, const float *>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(g), m, kdim, f.bitmap, f.lo, f.hi,
                       reinterpret_cast<const LT *>(f.sym), f.nnz, ncols, f.segs, centers, k, z, p.entries, p.cshift, p.rows_per_group, direct, out, rs);
}

template <typename XT, typename LT, int MT>
static void launch_dc_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const SgForm &f, long long ncols, int k,
                             int z, const SgPlan &p, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbspdc_stream<XT, LT, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim,
                       f.bitmap, f.lo, f.hi, reinterpret_cast<const LT *>(f.sym), f.nnz, ncols, f.segs, k, z, p.rlog2, p.terms_log2, p.rows_per_group, hdr, sums);
}

template <typename XT, typename LT>
static void launch_dx_mfma(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const SgForm &f, long long ncols,
                           const float *centers, int k, int z, const SgPlan &p, int direct, void *out)
{
    hm_launch(g, ncols, k_cbspdx_mfma<XT, LT, true>, k_cbspdx_mfma<XT, LT, false>, grid, lds, s, reinterpret_cast<const XT *>(g), m, kdim, f.bitmap, f.lo, f.hi,
              reinterpret_cast<const LT *>(f.sym), f.nnz, ncols, f.segs, centers, k, z, p.entries, p.cshift, p.col_tiles, p.per_split, direct, out);
}

template <typename XT, typename LT>
static void launch_dc_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const SgForm &f, long long ncols,
                           int k, int z, const SgPlan &p, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((dcm_xvec(x, g, kdim, ncols) ? k_cbspdc_mfma<XT, LT, true> : k_cbspdc_mfma<XT, LT, false>), grid, dim3(HM_THREADS), lds, s,
                       reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim, f.bitmap, f.lo, f.hi, reinterpret_cast<const LT *>(f.sym), f.nnz,
                       ncols, f.segs, k, z, p.rlog2, p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
}

template <typename XT>
static void launch_dx_finish(int rgrid, hipStream_t s, const float *part, long long splits, long long m, long long kdim, const float *rs, const float *centers,
                             int k, int z, void *dx, int dx_dtype)
{
    if (dx_dtype == NNC_DT_F32)
        hipLaunchKernelGGL((k_cbspdx_finish<XT, float>), dim3(rgrid), dim3(256), 0, s, part, splits, m, kdim, rs, centers, k, z, reinterpret_cast<float *>(dx));
    else
        hipLaunchKernelGGL((k_cbspdx_finish<XT, XT>), dim3(rgrid), dim3(256), 0, s, part, splits, m, kdim, rs, centers, k, z, reinterpret_cast<XT *>(dx));
}

// every kernel instantiation of this unit, a table of the stream ones per dtype; the plans are checked against these tables, and the
// launches go through them
using DxStream = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const SgForm &, long long, const float *, int, int, const SgPlan &, int,
                          void *, const float *);
using DcStream = void (*)(dim3, size_t, hipStream_t, const void *, const void *, int, long long, const SgForm &, long long, int, int, const SgPlan &, uint32_t *,
                          unsigned long long *);
using DxMfma = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const SgForm &, long long, const float *, int, int, const SgPlan &, int,
                        void *);
using DcMfma = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const SgForm &, long long, int, int, const SgPlan &,
                        uint32_t *, unsigned long long *);
struct StreamCase {
    int a, vb, mt;            // a: label_bytes; vb: 0 (a lane's columns are fixed by mt)
    DxStream dx;
    DcStream dc;
};
struct MfmaCase {
    int dt, a;                // a: label_bytes
    DxMfma dx;
    DcMfma dc;
};
#define SGH_CASE(XT, LT, LB, MT) {LB, 0, MT, launch_dx_stream<XT, LT, MT>, launch_dc_stream<XT, LT, MT>}
#define SGH_CASES(XT)                                                                                                                     \
    SGH_CASE(XT, uint8_t, 1, 1), SGH_CASE(XT, uint8_t, 1, 2), SGH_CASE(XT, uint8_t, 1, 4), SGH_CASE(XT, uint8_t, 1, 8),                     \
        SGH_CASE(XT, uint8_t, 1, 16), SGH_CASE(XT, uint16_t, 2, 1), SGH_CASE(XT, uint16_t, 2, 2), SGH_CASE(XT, uint16_t, 2, 4),             \
        SGH_CASE(XT, uint16_t, 2, 8), SGH_CASE(XT, uint16_t, 2, 16)
static const StreamCase kBf16Cases[] = {SGH_CASES(bf16_t)};
static const StreamCase kF16Cases[] = {SGH_CASES(f16_t)};
#undef SGH_CASES
#undef SGH_CASE
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 1, launch_dx_mfma<bf16_t, uint8_t>, launch_dc_mfma<bf16_t, uint8_t>}, {NNC_DT_BF16, 2, launch_dx_mfma<bf16_t, uint16_t>, launch_dc_mfma<bf16_t, uint16_t>},
    {NNC_DT_F16, 1, launch_dx_mfma<f16_t, uint8_t>, launch_dc_mfma<f16_t, uint8_t>},   {NNC_DT_F16, 2, launch_dx_mfma<f16_t, uint16_t>, launch_dc_mfma<f16_t, uint16_t>},
};
static const CbgCaseNames kSgNames = {false, "label_bytes", false};

// ------------------------------------------------------------------ C ABI
static int h16_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    const int rc = h16_check_dtype(fn, x_dtype);
    return rc != NNC_OK ? rc : sg_check(fn, m, kdim, ncols, label_bytes, k);
}

static SgForm sg_form(const void *packed, const SpLayout &L, long long nnz)
{
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    return {reinterpret_cast<const uint64_t *>(base), reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi),
            base + L.off_sym, nnz, L.segs};
}

extern "C" int64_t nnc_cbsp_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (sg_check("nnc_cbsp_dx_h16_workspace_bytes", m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    return h16_dx_ws_bytes(h16_dx_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS), m, kdim);
}

extern "C" int nnc_cbsp_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbsp_dx_h16_plan";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    const SgPlan p = h16_dx_plan(m, kdim, ncols, label_bytes, k, cus);
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgNames, p.path, label_bytes, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    const bool table = p.path == NNC_CBMM_STREAM || p.path == NNC_CBMM_MFMA;
    const int64_t v[NNC_CBSPDX_H16_PLAN_LEN] = {p.path, p.mt, p.segs, table ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries, p.splits, p.per_split, p.lds,
                                                p.col_tiles, p.row_tiles, h16_dx_ws_bytes(p, m, kdim), x_dtype};
    for (int i = 0; i < NNC_CBSPDX_H16_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbsp_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes, int64_t ncols,
                               int32_t zero_symbol, int64_t nnz, const float *centers_dev, int32_t k, void *dx, int dx_dtype, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_dx_h16";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if ((rc = sg_check_form(fn, m, kdim, ncols, label_bytes, zero_symbol, nnz, packed, packed_bytes)) != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbsp_dx_h16: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbsp_dx_h16: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbsp_dx_h16: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbsp_dx_h16: g is NULL");
    if (reinterpret_cast<uintptr_t>(g) % 2 || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbsp_dx_h16: g or dx is not aligned to its element size");
    const int64_t need = nnc_cbsp_dx_h16_workspace_bytes(m, kdim, ncols, label_bytes);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_dx_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK) return rc;
    const SgPlan p = h16_dx_plan(m, kdim, ncols, label_bytes, k, cu_count());
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgNames, p.path, label_bytes, 0, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SgForm f = sg_form(packed, sp_layout(kdim, ncols, label_bytes, nnz), nnz);
    if (p.path != NNC_CBMM_STREAM)   // nothing, dx = 0, or the MFMA tile: W_h holds c_z at a skipped position, so no row sums and no rank-1 term
        return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
            mc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, f, ncols, centers_dev, k, zero_symbol, p, direct,
                   out);
            LAUNCHCHK("k_cbspdx_mfma");
            return NNC_OK;
        });
    // The stream path is not cbg_run_dx's sequence: the rank-1 term has to meet the float32 sum before a half dx is rounded, so the
    // row sums of g come first, and the kernel (one column block) or k_cbspdx_finish (behind the partials) adds it and rounds once.
    float *rs = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sg_part_bytes(p, m, kdim));   // behind the partials
    if ((rc = cbsp_rowsum_dt(g, x_dtype, m, ncols, rs, s)) != NNC_OK) return rc;
    const int direct = cb_direct(p.splits, dx_dtype);
    sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, f, ncols, centers_dev, k, zero_symbol, p, direct,
           direct ? dx : workspace, rs);
    LAUNCHCHK("k_cbspdx_stream (h16)");
    if (direct) return NNC_OK;
    const int rgrid = (int)std::max(1LL, std::min(cdiv(m * kdim, 256), 8192LL));
    (x_dtype == NNC_DT_BF16 ? launch_dx_finish<bf16_t> : launch_dx_finish<f16_t>)(rgrid, s, reinterpret_cast<const float *>(workspace), p.splits, m, kdim, rs,
                                                                                  centers_dev, k, zero_symbol, dx, dx_dtype);
    LAUNCHCHK("k_cbspdx_finish");
    return NNC_OK;
}

extern "C" int64_t nnc_cbsp_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (sg_check("nnc_cbsp_dc_h16_workspace_bytes", m, kdim, ncols, label_bytes, k) != NNC_OK) return 0;
    SgPlan p;
    if (h16_dc_plan(m, kdim, ncols, label_bytes, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return h16_dc_ws_bytes(p.path, k);
}

extern "C" int nnc_cbsp_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbsp_dc_h16_plan";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    SgPlan p;
    if ((rc = h16_dc_plan(m, kdim, ncols, label_bytes, k, cus, p)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgNames, p.path, label_bytes, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    const int64_t v[NNC_CBSPDC_H16_PLAN_LEN] = {p.path, p.mt, p.segs, p.path == NNC_CBMM_ZERO ? 0 : 1LL << p.rlog2, p.splits, p.per_split, p.lds, p.col_tiles,
                                                p.row_tiles, p.terms_log2, h16_dc_ws_bytes(p.path, k), x_dtype};
    for (int i = 0; i < NNC_CBSPDC_H16_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbsp_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes,
                               int64_t ncols, int32_t zero_symbol, int64_t nnz, int32_t k, void *dc, int32_t out_f64, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_dc_h16";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if ((rc = sg_check_form(fn, m, kdim, ncols, label_bytes, zero_symbol, nnz, packed, packed_bytes)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbsp_dc_h16: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbsp_dc_h16: x or g is NULL");
    if (reinterpret_cast<uintptr_t>(x) % 2 || reinterpret_cast<uintptr_t>(g) % 2) return fail(NNC_EINVAL, "nnc_cbsp_dc_h16: x or g is not aligned to its element size");
    const int64_t need = nnc_cbsp_dc_h16_workspace_bytes(m, kdim, ncols, label_bytes, k);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_dc_h16_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    SgPlan p;
    if ((rc = h16_dc_plan(m, kdim, ncols, label_bytes, k, cu_count(), p)) != NNC_OK) return rc;
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgNames, p.path, label_bytes, 0, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgNames, p.path, x_dtype, label_bytes, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SgForm f = sg_form(packed, sp_layout(kdim, ncols, label_bytes, nnz), nnz);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, (int)k, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, f, ncols, k, zero_symbol, p, hdr, sums);
            LAUNCHCHK("k_cbspdc_stream (h16)");
        } else {
            mc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, f, ncols, k, zero_symbol, p, hdr, sums);
            LAUNCHCHK("k_cbspdc_mfma");
        }
        return NNC_OK;
    });
}
