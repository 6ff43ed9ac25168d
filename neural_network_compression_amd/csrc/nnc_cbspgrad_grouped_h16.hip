// nnc_cbspgrad_grouped_h16.hip -- the backward pass of the pruned group-wise codebook layer on bf16 / fp16 activations, from the
// bitmap-sparse form of its indices (include/nnc_cbspgrad_grouped_h16.h, nnc_cbsp_grouped_dx_h16 / nnc_cbsp_grouped_dc_h16; DESIGN.md
// section 35): the backward of nnc_cbsp_grouped_h16 (nnc_cbsp_grouped_h16.hip).  Group q = i / group_rows has the table c_q and the
// skipped symbol z_q; W_h[i, o] = rn(c_q[label[i, o]]) rounded to the type of g, the label of a skipped position being z_q: the
// forward's W_h.  A product of two bf16 or two fp16 values is exact in float32, every sum is float32, dc is binned as section 12's
// exact integers into G x K bins.
//
// The plans are the ungrouped sparse half ones at label_bytes 1 (nnc_cbspgrad_h16.hip: section 13's stream plans at m <= 16,
// nnc_cbh16plan.hpp's tiles and splits with the byte form's table and bins above), so the path, the tiles, the splits, the order of
// every sum and the shift S of the dc sums are those of nnc_cbsp_dx_h16 / nnc_cbsp_dc_h16, and at m > 16 those of
// nnc_cbmm_grouped_dx_h16 / nnc_cbmm_grouped_dc_h16, on the same shape.
//   m <= 16   k_cbspgdx_stream<XT> / k_cbspgdc_stream<XT> of nnc_cbspgrad_grouped.hpp: section 32's kernels with g and x widened as
//             they are loaded and, for dx, the d tables of the rounded centres.  dx: the kernel always writes its float32 sums as
//             partials (one block of them with one column block); k_cbspgdx_finish sums them in split order, adds the rank-1 term
//             rn(c_{z_q}) * rs[r] in float32 and rounds once.
//   k_cbspgdx_mfma  m > 16.  k_cbdx_mfma_grouped's tile, plan and LDS (the tables of the up to four groups of the tile's 128 index
//             rows divide the copies of the per-bank table) with k_cbspdx_mfma's decode of the B operand: thread t owns index row
//             n0 + (t mod 128) and 16 aligned bits of one bitmap word per step, whose symbols are one run of the stream starting at
//             the segment's count plus the popcount below the bits; word and count are requested two steps ahead.  Its own: a
//             thread resolves its row's table pointer and its row's z_q once, ahead of the loop; a skipped position takes the
//             table entry of z_q (0 where z_q >= k: the entries past k are 0), so there is no rank-1 term and no row sum.
//   k_cbspgdc_mfma  m > 16.  dcm_accumulate unchanged, then the epilogue of k_cbspdc_mfma with k_cbdc_mfma_grouped's sets of bins:
//             the 32 rows of accumulator half a lie in one group, so the set and z_q are scalars per a; a stored weight's image
//             goes into the set's replicated LDS bins, a skipped one's into a per-lane int64 register flushed into bin
//             (set, z_q) once per a (not at all if z_q >= k); one cbdc_flush per live set into sums + (q0 + t) * k.
// No load leaves the packed buffer: rows past kdim load no word, columns past the split none, a symbol is loaded only below nnz, z_q
// only of a group below G.  Everything past m, kdim, ncols and the end of a split is zero in the images, never memory.  No float
// atomics; no host read.
#include "nnc_cbgrad_grouped.hpp"
#include "nnc_cbgrad_h16.hpp"
#include "nnc_cbh16plan.hpp"
#include "nnc_cbspgrad_grouped.hpp"

// ------------------------------------------------------------------ dx, m <= 16
// the split partials summed in split order (as k_cbgrad_reduce sums them), then + c_{z_q} * rs where c_{z_q} != 0 (as
// k_cbspgdx_rank1 adds it; RT: the type the centre is rounded to), then the one rounding to OT.  grid (column blocks, row strides): a
// thread owns column i and looks its group's centre up once.
template <typename RT, typename OT>
__global__ __launch_bounds__(256) void k_cbspgdx_finish(const float *__restrict__ part, long long splits, long long m, long long kdim,
                                                        const float *__restrict__ rs, const float *__restrict__ centers, int k,
                                                        const uint8_t *__restrict__ zsym, long long group_rows, OT *__restrict__ dx)
{
    const long long mn = m * kdim;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < kdim; i += (long long)gridDim.x * blockDim.x) {
        const float cz = spg_cz<RT>(centers, k, zsym, i / group_rows);
        for (long long r = blockIdx.y; r < m; r += gridDim.y) {
            const long long idx = r * kdim + i;
            float v = part[idx];
            for (long long s = 1; s < splits; ++s) v += part[s * mn + idx];
            if (cz != 0.0f) v = cz * rs[r] + v;   // (a NaN centre counts)
            dx[idx] = (OT)v;
        }
    }
}

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads; `out`, direct and cols_per_split as k_cbdx_mfma.  LDS as
// k_cbdx_mfma_grouped: 1 << tlog2 tables of entries << (cshift - tlog2) words (table t that of group n0 / group_rows + t; entries
// past k are 0, so a symbol or a z_q >= k reads 0), the staging row, the two images.
template <typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbspgdx_mfma(const XT *__restrict__ g, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                             const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                             const uint8_t *__restrict__ sym, long long nnz, long long ncols, long long segs,
                                                             const float *__restrict__ centers, int k, const uint8_t *__restrict__ zsym,
                                                             long long group_rows, int entries, int cshift, int tlog2, long long col_tiles,
                                                             long long cols_per_split, int direct, void *__restrict__ out_)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    float *cb = hm_smem;                                // entries << cshift: the tables, one after the other
    float *stage = cb + (entries << cshift);            // entries
    XT *gs = reinterpret_cast<XT *>(hm_smem + hm_table_words(entries, cshift));   // [HM_BM][HM_LD]: g tile, row-major in o
    XT *ws = gs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: W^T tile, [i][o]

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);   // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const int tcs = cshift - tlog2, tables = 1 << tlog2;          // the copies of one table (log2)
    const TileGroups G = tile_groups_at(T.n0, kdim, group_rows);
    for (int t = 0; t < tables; ++t) {                  // (uniform over the workgroup; a table past the last group repeats it, unread)
        if (t) __syncthreads();                         // the staging row of the table before has been copied
        cb_fill<XT>(cb + (long long)t * (entries << tcs), stage, centers + std::min(G.q0 + t, G.groups - 1) * k, k, entries, tcs);
    }

    const long long gi = T.n0 + T.wc;
    const bool row_ok = gi < kdim;
    const long long wrow = gi * segs;
    const float *tab = cb + tile_group_of(G, gi, group_rows, tables) * (entries << tcs) + (T.lane & ((1 << tcs) - 1));
    uint32_t lo0 = 0, hrow = 0, zq = 0;                 // the row's own count (lo[i * segs], hi[i]) and its group's skipped symbol
    if (row_ok) {
        lo0 = lo[wrow];
        hrow = hi[gi];
        zq = zsym[gi / group_rows];
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
            lab[j] = zq;                                // a skipped position (every position of an empty word)
            if (((bits >> j) & 1u) && pos < nnz) lab[j] = (uint32_t)sym[pos];
        }
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? tab[lab[j] << tcs] : 0.0f;
        hm_store_w(ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    load_words(T.k_lo);
    hm_accumulate<XT, XVEC>(g, m, ncols, T, gs, ws, acc, load_w, store_w, [&](long long ob) { load_words(ob + HM_BK); });
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads.  LDS as k_cbdc_mfma_grouped: the two images, then the k << rlog2
// int64 bins, cut into 1 << sets_log2 sets of k << (rlog2 - sets_log2), set t for group m0 / group_rows + t.
template <typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbspgdc_mfma(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                             const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo,
                                                             const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym, long long nnz,
                                                             long long ncols, long long segs, int k, const uint8_t *__restrict__ zsym,
                                                             long long group_rows, int rlog2, int sets_log2, int terms_log2, long long col_tiles,
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

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col).  The 32 rows of a lie in one group: its set of bins and its z_q are
    // scalars.  The 32 lanes of a row lie in the wave's one segment (n0 + wn is a multiple of 64), so one word and one count serve
    // both b; a lane's label is the symbol at count + popcount(word below its column).
    const int rl = rlog2 - sets_log2, sets = 1 << sets_log2;
    const TileGroups G = tile_groups_at(T.m0, kdim, group_rows);
    const long long row0 = tile_wave_row0(T.m0);
    const int rep = T.t & ((1 << rl) - 1);
    const long long sg = (T.n0 + T.wn) >> 6;
    const bool seg_ok = sg < segs;                      // (else every column of the wave lies past ncols)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int set = (int)tile_group_of(G, row0 + a * 32, group_rows, sets);
        unsigned long long *sb = bins + ((long long)set * k << rl);
        const uint32_t z = G.q0 + set < G.groups ? (uint32_t)zsym[G.q0 + set] : (uint32_t)k;   // (rows past kdim: nothing is binned)
        unsigned long long skip = 0;                    // the images of the lane's skipped weights in these rows: bin (set, z)
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
                if (((word >> c) & 1) && pos < nnz) {   // (a symbol past nnz: skipped, as nnc_cbsp_grouped_unpack reads it)
                    const uint32_t l = (uint32_t)sym[pos];
                    if (l < (uint32_t)k) atomicAdd(&sb[(l << rl) + rep], img);
                } else {
                    skip += img;
                }
            }
        }
        if (z < (uint32_t)k && skip) atomicAdd(&sb[(z << rl) + rep], skip);
    }
    for (int t = 0; t < sets && G.q0 + t < G.groups; ++t) cbdc_flush(bins + ((long long)t * k << rl), k, rl, sums + (G.q0 + t) * k);   // (count: blockIdx alone)
}

// ------------------------------------------------------------------ plans (host)
// nnc_cbsp_dx_h16's / nnc_cbsp_dc_h16's plans at label_bytes 1.  m <= 16 and the empty shapes: section 13's plans (sg_dx_plan,
// sg_dc_plan).  m > 16: nnc_cbh16plan.hpp's tiles and splits with the LDS of k_cbdx_mfma / k_cbdc_mfma, which the tables / sets of a
// tile divide.
static SgPlan sgh_dx_plan(long long m, long long kdim, long long ncols, int k, int cus)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return sg_dx_plan(m, kdim, ncols, 1, k, cus);
    int entries = 0, cshift = 0;   // (cb_table_shape counts cshift up from 0)
    cb_table_shape(1, k, entries, cshift);
    SgPlan p = h16_mfma_plan<SgPlan>(h16_dx_tiles(m, kdim, ncols), (long long)hm_table_words(entries, cshift) * 4);
    p.entries = entries, p.cshift = cshift;
    return p;
}

// the dx workspace.  MFMA: the partials of a split call.  Stream: [partials: max(splits, 1) x m x kdim floats, 256-byte aligned][row
// sums of g: m floats] -- the stream kernel writes partials also with one column block, for k_cbspgdx_finish to round once
static long long sgh_part_bytes(const SgPlan &p, long long m, long long kdim) { return (std::max(p.splits, 1LL) * m * kdim * 4 + 255) / 256 * 256; }
static int64_t sgh_dx_ws_bytes(const SgPlan &p, long long m, long long kdim)
{
    if (p.path == NNC_CBMM_MFMA) return cbg_dx_ws_bytes(p.splits, m, kdim);
    return p.path == NNC_CBMM_STREAM ? sgh_part_bytes(p, m, kdim) + m * 4 : 0;
}

static int sgh_dc_plan(long long m, long long kdim, long long ncols, int k, int cus, SgPlan &p)
{
    if (!h16_mfma_shape(m, kdim, ncols)) return sg_dc_plan(m, kdim, ncols, 1, k, cus, p);
    p = h16_mfma_plan<SgPlan>(h16_dc_tiles(m, kdim, ncols), ((long long)k << dc_rlog2(k)) * 8);
    p.rlog2 = dc_rlog2(k);
    return NNC_OK;
}

// ------------------------------------------------------------------ launches
// (SpgForm, nnc_cbsp_grouped.hpp: the parts of the packed buffer and the group-wise operands every kernel takes)
template <typename XT, int MT>
static void launch_dx_stream(dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const SpgForm &f, long long ncols, const SgPlan &p,
                             float *part)
{
    hipLaunchKernelGGL((k_cbspgdx_stream<XT, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(g), m, kdim, f.bitmap, f.lo, f.hi, f.sym, f.nnz,
                       ncols, f.segs, f.centers, f.k, f.zsym, f.group_rows, p.entries, p.cshift, p.rows_per_group, 0, part);
}

template <typename XT, int MT>
static void launch_dc_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const SpgForm &f, long long ncols,
                             const SgPlan &p, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbspgdc_stream<XT, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim,
                       f.bitmap, f.lo, f.hi, f.sym, f.nnz, ncols, f.segs, f.k, f.zsym, f.group_rows, p.rlog2, p.terms_log2, p.rows_per_group, hdr, sums);
}

template <typename XT>
static void launch_dx_mfma(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const SpgForm &f, long long ncols, const SgPlan &p,
                           int direct, void *out)
{
    hm_launch(g, ncols, k_cbspgdx_mfma<XT, true>, k_cbspgdx_mfma<XT, false>, grid, lds, s, reinterpret_cast<const XT *>(g), m, kdim, f.bitmap, f.lo, f.hi, f.sym,
              f.nnz, ncols, f.segs, f.centers, f.k, f.zsym, f.group_rows, p.entries, p.cshift, __builtin_ctz(tile_groups(f.group_rows)), p.col_tiles, p.per_split,
              direct, out);
}

template <typename XT>
static void launch_dc_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const SpgForm &f, long long ncols,
                           const SgPlan &p, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((dcm_xvec(x, g, kdim, ncols) ? k_cbspgdc_mfma<XT, true> : k_cbspgdc_mfma<XT, false>), grid, dim3(HM_THREADS), lds, s,
                       reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim, f.bitmap, f.lo, f.hi, f.sym, f.nnz, ncols, f.segs, f.k, f.zsym,
                       f.group_rows, p.rlog2, __builtin_ctz(tile_groups(f.group_rows)), p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
}

template <typename XT>
static void launch_dx_finish(hipStream_t s, const float *part, long long splits, long long m, long long kdim, const float *rs, const SpgForm &f, void *dx,
                             int dx_dtype)
{
    const long long gx = std::min(cdiv(kdim, 256), 8192LL), gy = std::max(1LL, std::min(m, 8192LL / gx));
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (dx_dtype == NNC_DT_F32)
        hipLaunchKernelGGL((k_cbspgdx_finish<XT, float>), grid, dim3(256), 0, s, part, splits, m, kdim, rs, f.centers, f.k, f.zsym, f.group_rows,
                           reinterpret_cast<float *>(dx));
    else
        hipLaunchKernelGGL((k_cbspgdx_finish<XT, XT>), grid, dim3(256), 0, s, part, splits, m, kdim, rs, f.centers, f.k, f.zsym, f.group_rows,
                           reinterpret_cast<XT *>(dx));
}

// every kernel instantiation of this unit, a table of the stream ones per dtype; the plans are checked against these tables, and the
// launches go through them
using DxStream = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const SpgForm &, long long, const SgPlan &, float *);
using DcStream = void (*)(dim3, size_t, hipStream_t, const void *, const void *, int, long long, const SpgForm &, long long, const SgPlan &, uint32_t *,
                          unsigned long long *);
using DxMfma = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const SpgForm &, long long, const SgPlan &, int, void *);
using DcMfma = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const SpgForm &, long long, const SgPlan &, uint32_t *,
                        unsigned long long *);
struct StreamCase {
    int a, vb, mt;            // a: 0 (uint8 symbols only); vb: 0 (a lane's columns are fixed by mt)
    DxStream dx;
    DcStream dc;
};
struct MfmaCase {
    int dt, a;                // a: 0 (uint8 symbols only)
    DxMfma dx;
    DcMfma dc;
};
#define SGGH_CASE(XT, MT) {0, 0, MT, launch_dx_stream<XT, MT>, launch_dc_stream<XT, MT>}
#define SGGH_CASES(XT) SGGH_CASE(XT, 1), SGGH_CASE(XT, 2), SGGH_CASE(XT, 4), SGGH_CASE(XT, 8), SGGH_CASE(XT, 16)
static const StreamCase kBf16Cases[] = {SGGH_CASES(bf16_t)};
static const StreamCase kF16Cases[] = {SGGH_CASES(f16_t)};
#undef SGGH_CASES
#undef SGGH_CASE
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 0, launch_dx_mfma<bf16_t>, launch_dc_mfma<bf16_t>},
    {NNC_DT_F16, 0, launch_dx_mfma<f16_t>, launch_dc_mfma<f16_t>},
};
static const CbgCaseNames kSgghNames = {true, nullptr, false};

// ------------------------------------------------------------------ C ABI
static int sggh_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    const int rc = h16_check_dtype(fn, x_dtype);
    return rc != NNC_OK ? rc : sgg_check(fn, m, kdim, ncols, k, group_rows);
}

// the group fields behind the record of the ungrouped sparse half plan (its NNC_CBSPDX_H16_PLAN_LEN = NNC_CBSPDC_H16_PLAN_LEN values
// and one reserved 0), at the offsets of the other group-wise half plans
static void sggh_plan_tail(const SgPlan &p, int64_t kdim, int64_t group_rows, int64_t *out)
{
    const bool mfma = p.path == NNC_CBMM_MFMA;
    out[NNC_CBSPDX_H16_PLAN_LEN] = 0;
    cbg_grouped_plan_tail(mfma ? NNC_CBMM_TILED : p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out + NNC_CBGRAD_GROUPED_H16_P_GROUP_ROWS);
    out[NNC_CBGRAD_GROUPED_H16_P_HELD] = mfma ? tile_groups(group_rows) : 0;
}

extern "C" int64_t nnc_cbsp_grouped_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols)
{
    if (sg_check("nnc_cbsp_grouped_dx_h16_workspace_bytes", m, kdim, ncols, 1, 1) != NNC_OK) return 0;
    return sgh_dx_ws_bytes(sgh_dx_plan(m, kdim, ncols, 1, CB_PLAN_CUS), m, kdim);
}

extern "C" int nnc_cbsp_grouped_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbsp_grouped_dx_h16_plan";
    int rc = sggh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    const SgPlan p = sgh_dx_plan(m, kdim, ncols, k, cus);
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgghNames, p.path, 0, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgghNames, p.path, x_dtype, 0, mc)) != NNC_OK) return rc;
    if ((rc = nnc_cbsp_dx_h16_plan(x_dtype, m, kdim, ncols, 1, k, cus, out)) != NNC_OK) return rc;   // the shared fields: the ungrouped record
    out[NNC_CBSPDX_P_WORKSPACE] = sgh_dx_ws_bytes(p, m, kdim);                                       // (the stream path always writes partials)
    sggh_plan_tail(p, kdim, group_rows, out);
    return NNC_OK;
}

extern "C" int nnc_cbsp_grouped_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                                       const void *zero_symbols_dev, int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, void *dx,
                                       int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_dx_h16";
    int rc = sggh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = sgg_check_form(fn, m, kdim, ncols, nnz, packed, packed_bytes, zero_symbols_dev)) != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_h16: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_h16: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_h16: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_h16: g is NULL");
    if (reinterpret_cast<uintptr_t>(g) % 2 || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_h16: g or dx is not aligned to its element size");
    const int64_t need = nnc_cbsp_grouped_dx_h16_workspace_bytes(m, kdim, ncols);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_grouped_dx_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK)
        return rc;
    const SgPlan p = sgh_dx_plan(m, kdim, ncols, k, cu_count());
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgghNames, p.path, 0, 0, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgghNames, p.path, x_dtype, 0, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SpgForm f = spg_form(packed, sp_layout(kdim, ncols, 1, nnz), nnz, zero_symbols_dev, group_rows, centers_dev, k);
    if (p.path != NNC_CBMM_STREAM)   // nothing, dx = 0, or the MFMA tile: W_h holds c_{z_q} at a skipped position, so no row sums and no rank-1 term
        return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
            mc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, f, ncols, p, direct, out);
            LAUNCHCHK("k_cbspgdx_mfma");
            return NNC_OK;
        });
    // The stream path is not cbg_run_dx's sequence: the rank-1 term has to meet the float32 sum before a half dx is rounded, so the row
    // sums of g come first and k_cbspgdx_finish, behind the partials, adds it and rounds once.
    float *part = reinterpret_cast<float *>(workspace);
    float *rs = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sgh_part_bytes(p, m, kdim));
    if ((rc = cbsp_rowsum_dt(g, x_dtype, m, ncols, rs, s)) != NNC_OK) return rc;
    sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, f, ncols, p, part);
    LAUNCHCHK("k_cbspgdx_stream (h16)");
    (x_dtype == NNC_DT_BF16 ? launch_dx_finish<bf16_t> : launch_dx_finish<f16_t>)(s, part, p.splits, m, kdim, rs, f, dx, dx_dtype);
    LAUNCHCHK("k_cbspgdx_finish");
    return NNC_OK;
}

extern "C" int64_t nnc_cbsp_grouped_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (sgg_check("nnc_cbsp_grouped_dc_h16_workspace_bytes", m, kdim, ncols, k, group_rows) != NNC_OK) return 0;
    SgPlan p;
    if (sgh_dc_plan(m, kdim, ncols, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return h16_dc_ws_bytes(p.path, gg_groups(kdim, group_rows) * k);
}

extern "C" int nnc_cbsp_grouped_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbsp_grouped_dc_h16_plan";
    int rc = sggh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    SgPlan p;
    if ((rc = sgh_dc_plan(m, kdim, ncols, k, cus, p)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgghNames, p.path, 0, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgghNames, p.path, x_dtype, 0, mc)) != NNC_OK) return rc;
    if ((rc = nnc_cbsp_dc_h16_plan(x_dtype, m, kdim, ncols, 1, k, cus, out)) != NNC_OK) return rc;   // the shared fields: the ungrouped record
    out[NNC_CBSPDC_P_WORKSPACE] = h16_dc_ws_bytes(p.path, gg_groups(kdim, group_rows) * k);          // (G * k bins)
    sggh_plan_tail(p, kdim, group_rows, out);
    return NNC_OK;
}

extern "C" int nnc_cbsp_grouped_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes,
                                       int64_t ncols, const void *zero_symbols_dev, int64_t nnz, int32_t k, int64_t group_rows, void *dc, int32_t out_f64,
                                       void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_dc_h16";
    int rc = sggh_check(fn, x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = sgg_check_form(fn, m, kdim, ncols, nnz, packed, packed_bytes, zero_symbols_dev)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dc_h16: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dc_h16: x or g is NULL");
    if (reinterpret_cast<uintptr_t>(x) % 2 || reinterpret_cast<uintptr_t>(g) % 2)
        return fail(NNC_EINVAL, "nnc_cbsp_grouped_dc_h16: x or g is not aligned to its element size");
    const int64_t need = nnc_cbsp_grouped_dc_h16_workspace_bytes(m, kdim, ncols, k, group_rows);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_grouped_dc_h16_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK)
        return rc;
    SgPlan p;
    if ((rc = sgh_dc_plan(m, kdim, ncols, k, cu_count(), p)) != NNC_OK) return rc;
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kSgghNames, p.path, 0, 0, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kSgghNames, p.path, x_dtype, 0, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SpgForm f = spg_form(packed, sp_layout(kdim, ncols, 1, nnz), nnz, zero_symbols_dev, group_rows, nullptr, k);
    const int nbins = (int)(gg_groups(kdim, group_rows) * k);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, f, ncols, p, hdr, sums);
            LAUNCHCHK("k_cbspgdc_stream (h16)");
        } else {
            mc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, f, ncols, p, hdr, sums);
            LAUNCHCHK("k_cbspgdc_mfma");
        }
        return NNC_OK;
    });
}
