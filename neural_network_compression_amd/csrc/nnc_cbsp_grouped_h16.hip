// nnc_cbsp_grouped_h16.hip -- the pruned group-wise codebook layer of nnc_cbsp_grouped.hip on bf16 / fp16 activations
// (include/nnc_cbsp_grouped_h16.h, nnc_cbsp_grouped_h16): y = x @ W_h + bias, W_h[i, o] = the centre
// centers[i / group_rows][label[i, o]] rounded to x's type, the label of a skipped position being zero_symbols[i / group_rows].  A
// product of two bf16 or two fp16 values is exact in float32; every sum is float32.  Forward and inference only.
//
//   m <= 16: the kernels of nnc_cbsp_grouped.hpp with XT = bf16_t / f16_t: k_cbspg_rowterm, k_cbspg_stream, k_cbspg_combine under
//            nnc_cbsp_grouped_plan's stream plan (sp_plan).  x is read as XT and widened, c_{z_g} is rn(c) widened, the d table is
//            rn(c_g[s]) - rn(c_{z_g}): section 28's float32 arithmetic on half the x bytes.  A skipped weight stays absent when
//            rn(c_{z_g}) == 0.
//   m > 16:  k_cbspg_mfma, the combination of k_cbsp_mfma's decode (SpTileDecode, nnc_cbsp.hpp: a wave owns one 64-column segment, 16
//            lanes load a row's bitmap word and count, v_readlane broadcasts them, a lane's symbol sits at count + v_mbcnt(word)) and
//            k_cbmm_mfma_grouped's table walk (nnc_cbmm_grouped.hip: a k step of HM_BK lies in one group, the step that opens a group
//            refills the table ahead of its first barrier), on the tile and the k loop of nnc_cbmfma.hpp under the grouped byte
//            form's half plan (cb_plan).  Its own: the skipped label changes with the group.  It is the z of the step being loaded (the next step's
//            group when the loop loads ahead), loaded with that step's words, made uniform over the wave by readfirstlane when the
//            step is decoded, and looked up like any stored label after the refill: W_h holds rn(c_{z_g}) at a
//            skipped position (0 for z_g >= k), no rank-1 term, no row sums.  k_cbmm_reduce combines the splits: y is nnc_cbmm_grouped's
//            on the unpacked labels bit for bit.
#include "nnc_cbsp_grouped.hpp"

// grid (col_tiles * row_tiles, splits), HM_THREADS threads; out, direct and rows_per_split as k_cbmm_mfma_grouped.  What steers the
// walk (the k steps, the two group counters, z) comes from blockIdx and the arguments or is made uniform by readfirstlane; every
// wave reaches every barrier.  No load leaves its buffer: SpTileDecode argues it for the form, and both group counters follow a k
// step below k_hi <= kdim, so they stay at or below (kdim - 1) / group_rows = G - 1.  No readlane / readfirstlane sits inside a
// lane-dependent branch.
template <typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbspg_mfma(const XT *__restrict__ x, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                           const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym,
                                                           long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                           const uint8_t *__restrict__ zsym, long long group_rows, int entries, int cshift,
                                                           long long col_tiles, long long rows_per_split, const float *__restrict__ bias, int relu,
                                                           int direct, void *__restrict__ out_)
{
    using LT = uint8_t;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, entries, cshift);
    long long group = (long long)blockIdx.y * rows_per_split / group_rows;   // the group whose table is in LDS
    cb_fill<XT>(L.cb, L.stage, centers + group * k, k, entries, cshift);

    const HmTile T = hm_tile(col_tiles, rows_per_split, kdim);
    const bool col_ok = T.n0 + T.wc < ncols;
    SpTileDecode<LT> D(bitmap, lo, hi, sym, nnz, segs, T);
    long long zgroup = group;                           // the group of the step whose words were loaded last, two steps ahead of `group`
    uint32_t zraw = 0;                                  // its z as loaded
    uint32_t lab[16];

    auto load_words = [&](long long kb) {
        D.load_words(kb);
        if (kb < T.k_hi) {                              // uniform; the step's group is at most G - 1, and its z comes with its words
            if (kb >= (zgroup + 1) * group_rows) ++zgroup;
            zraw = zsym[zgroup];
        }
    };
    // a step kb < k_hi, from the words and the z load_words(kb) brought: the z made uniform here, outside every lane-dependent branch
    auto load_w = [&](long long) { D.decode((uint32_t)__builtin_amdgcn_readfirstlane((int)zraw), lab); };
    auto store_w = [&](long long kb) {                  // the labels of this step, its group's z among them, in its group's table
        hm_lookup_w(L.ws, L.cb, T, col_ok, kb, lab, [&](uint32_t l) { return CbTable<LT>::index(l, k, cshift, T.lane); });
    };
    auto open = [&](long long kb) {                     // this step opens a group
        if (kb >= (group + 1) * group_rows) cb_refill<XT>(L.cb, centers + ++group * k, k, cshift);
    };

    typename HFrag<XT>::C acc[2][2];
    load_words(T.k_lo);
    hm_accumulate<XT, XVEC>(x, m, kdim, T, L.xs, L.ws, acc, load_w, store_w, [&](long long kb) { load_words(kb + HM_BK); }, open);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, ncols, bias, relu, direct, out_);
}

// ------------------------------------------------------------------ launches
template <typename XT>
static void launch_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const SpgForm &f, long long ncols, int entries,
                        int cshift, long long col_tiles, long long rps, const float *bias, int relu, int direct, void *out)
{
    hm_launch(x, kdim, k_cbspg_mfma<XT, true>, k_cbspg_mfma<XT, false>, grid, lds, s, reinterpret_cast<const XT *>(x), m, kdim, f.bitmap, f.lo, f.hi, f.sym,
              f.nnz, ncols, f.segs, f.centers, f.k, f.zsym, f.group_rows, entries, cshift, col_tiles, rps, bias, relu, direct, out);
}

// every kernel instantiation of this unit; the plan is checked against these tables, and the launches go through them
using MfmaLaunch = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const SpgForm &, long long, int, int, long long, long long,
                            const float *, int, int, void *);
using RunStream = int (*)(SpgStreamLaunch, const SpPlan &, hipStream_t, const void *, long long, long long, const SpgForm &, long long, const float *, int,
                          void *, int, void *);
struct MfmaCase {
    int dt;
    MfmaLaunch fn;
};
static const SpgStreamCase kStreamCases[] = {SPG_STREAM_CASES(NNC_DT_BF16, bf16_t), SPG_STREAM_CASES(NNC_DT_F16, f16_t)};
static const MfmaCase kMfmaCases[] = {{NNC_DT_BF16, launch_mfma<bf16_t>}, {NNC_DT_F16, launch_mfma<f16_t>}};

static SpgStreamLaunch find_stream(int dt, int mt)
{
    for (const SpgStreamCase &c : kStreamCases)
        if (c.dt == dt && c.mt == mt) return c.fn;
    return nullptr;
}

static MfmaLaunch find_mfma(int dt)
{
    for (const MfmaCase &c : kMfmaCases)
        if (c.dt == dt) return c.fn;
    return nullptr;
}

static int no_stream_case(int dt, int mt)
{
    return fail(NNC_EINVAL, "nnc_cbsp_grouped_h16: no k_cbspg_stream instantiation for dtype " + std::to_string(dt) + ", mt " + std::to_string(mt));
}

static int no_mfma_case(int dt) { return fail(NNC_EINVAL, "nnc_cbsp_grouped_h16: no k_cbspg_mfma instantiation for dtype " + std::to_string(dt)); }

// ------------------------------------------------------------------ C ABI
static int h16_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16) return fail(NNC_EINVAL, std::string(fn) + ": x_dtype must be NNC_DT_BF16 or NNC_DT_F16");
    return spg_check(fn, m, kdim, ncols, k, group_rows);
}

// m <= 16 follows sp_plan (its stream plan, as nnc_cbsp_grouped_f32), m > 16 cb_plan's half plan (as nnc_cbmm_grouped)
static bool h16_skinny(int64_t m) { return m <= CB_SKINNY_M; }

extern "C" int64_t nnc_cbsp_grouped_h16_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols)
{
    if (x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16) return 0;
    if (m <= 0 || kdim <= 0 || ncols <= 0 || m > (1LL << 40) || !sp_size_ok(kdim, ncols)) return 0;
    if (h16_skinny(m)) return spg_ws_bytes(sp_plan(m, kdim, ncols, 1, 1, CB_PLAN_CUS), m, ncols);
    return cb_ws_bytes(cb_plan(m, kdim, ncols, 1, 1, CB_PLAN_CUS, 0, true), m, ncols);
}

extern "C" int nnc_cbsp_grouped_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbsp_grouped_h16_plan";
    const int rc = h16_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, std::string(fn) + ": cus < 1");
    if (!out) return fail(NNC_EINVAL, std::string(fn) + ": out is NULL");
    const int64_t groups = kdim > 0 ? cdiv(kdim, group_rows) : 0;
    if (h16_skinny(m)) {
        const SpPlan p = sp_plan(m, kdim, ncols, 1, k, cus);
        if (p.path == NNC_CBMM_STREAM && !find_stream(x_dtype, p.mt)) return no_stream_case(x_dtype, p.mt);
        const bool product = p.path == NNC_CBMM_STREAM;
        const int64_t v[NNC_CBSP_GROUPED_H16_PLAN_LEN] = {p.path, p.mt, product ? 1LL << p.cshift : 0, p.entries, p.splits, p.rows_per_split,
                                                          product ? NNC_CBSP_ROWSUM_PASS : NNC_CBSP_ROWSUM_NONE, p.lds, p.col_tiles, p.row_tiles,
                                                          product ? spg_ws_bytes(p, m, ncols) : 0, group_rows, groups,
                                                          p.splits > 0 ? max_groups_per_split(p.splits, p.rows_per_split, kdim, group_rows) : 0, x_dtype};
        std::copy(v, v + NNC_CBSP_GROUPED_H16_PLAN_LEN, out);
        return NNC_OK;
    }
    const CbPlan p = cb_plan(m, kdim, ncols, 1, k, cus, 0, true);
    if (p.path == NNC_CBMM_MFMA && !find_mfma(x_dtype)) return no_mfma_case(x_dtype);
    const int64_t v[NNC_CBSP_GROUPED_H16_PLAN_LEN] = {p.path, p.mt, p.entries ? 1LL << p.cshift : 0, p.entries, p.splits, p.rows_per_split, NNC_CBSP_ROWSUM_NONE,
                                                      p.lds, p.col_tiles, p.row_tiles, cb_ws_bytes(p, m, ncols), group_rows, groups,
                                                      p.splits > 0 ? max_groups_per_split(p.splits, p.rows_per_split, kdim, group_rows) : 0, x_dtype};
    std::copy(v, v + NNC_CBSP_GROUPED_H16_PLAN_LEN, out);
    return NNC_OK;
}

extern "C" int nnc_cbsp_grouped_h16(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                                    const void *zero_symbols_dev, int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, const float *bias_dev,
                                    int32_t relu, void *y, int y_dtype, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_h16";
    int rc = h16_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, std::string(fn) + ": nnz outside 0..kdim * ncols");
    const SpLayout L = sp_layout(kdim, ncols, 1, nnz);
    if (packed_bytes < L.bytes) return fail(NNC_EINVAL, std::string(fn) + ": packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz)");
    rc = cb_check_operands(fn, x, x_dtype, y, y_dtype, centers_dev, m, kdim, ncols, !x || !packed || !zero_symbols_dev, "x, packed or zero_symbols");
    if (rc != NNC_OK) return rc;
    if (m > 0 && ncols > 0 && kdim > 0 && reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, std::string(fn) + ": packed must be 256-byte aligned");
    const int64_t need = nnc_cbsp_grouped_h16_workspace_bytes(x_dtype, m, kdim, ncols);
    rc = cb_check_workspace(fn, "nnc_cbsp_grouped_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned");
    if (rc != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    if (kdim == 0) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // y = bias, as nnc_cbmm_grouped
    const SpgForm f = spg_form(packed, L, nnz, zero_symbols_dev, group_rows, centers_dev, k);
    if (!h16_skinny(m)) {
        const CbPlan p = cb_plan(m, kdim, ncols, 1, k, cu_count(), 0, true);
        const MfmaLaunch mfma = find_mfma(x_dtype);
        if (!mfma) return no_mfma_case(x_dtype);
        const int direct = cb_direct(p.splits, y_dtype);
        mfma(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, m, kdim, f, ncols, p.entries, p.cshift, p.col_tiles,
             p.rows_per_split, bias_dev, relu, direct, direct ? y : workspace);
        LAUNCHCHK("k_cbspg_mfma");
        return cb_finish(direct, workspace, p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
    }
    const SpPlan p = sp_plan(m, kdim, ncols, 1, k, cu_count());
    const SpgStreamLaunch stream_fn = find_stream(x_dtype, p.mt);
    if (!stream_fn) return no_stream_case(x_dtype, p.mt);
    const RunStream run = x_dtype == NNC_DT_BF16 ? spg_run_stream<bf16_t> : spg_run_stream<f16_t>;
    return run(stream_fn, p, s, x, m, kdim, f, ncols, bias_dev, relu, y, y_dtype, workspace);
}
