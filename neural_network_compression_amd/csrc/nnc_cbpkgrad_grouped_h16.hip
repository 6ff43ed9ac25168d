// nnc_cbpkgrad_grouped_h16.hip -- the backward pass of the group-wise codebook matmul on 2- and 4-bit packed indices on bf16 / fp16
// activations (include/nnc_cbgrad_grouped_h16.h, nnc_cbpk_grouped_dx_h16 / nnc_cbpk_grouped_dc_h16).
// W_h[i, o] = the centre centers[i / group_rows][label (i, o)] rounded to the type of g, a label >= K reading 0 and a padding field
// past ncols forming no product; products are exact in float32, every sum is float32, dc is binned into G x K exact integers.
//
// The plans are the ungrouped packed half ones (section 15's stream plans; nnc_cbh16plan.hpp's tiles and splits at m > 16) plus the
// group fields, as section 20 took the float32 ones: the path, the tiles, the splits, the order of every sum and S are those of
// nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16.  The two main loops are the ungrouped kernels' (hm_accumulate, dcm_accumulate), the pick of a
// row's table or set tile_group_of (nnc_cbgrad_grouped.hpp).
//   m <= 16   k_cbpkdx_stream_grouped<XT> / k_cbpkdc_stream_grouped<XT> of nnc_cbpkgrad_grouped.hpp: section 20's kernels with g and
//             x widened as they are loaded and, for dx, the per-wave tables of the rounded centres.
//   k_cbpkdx_mfma_grouped  m > 16.  k_cbpkdx_mfma (nnc_cbpk_h16.hip) with one whole per-bank table (2^BITS entries x PK_COPIES: 2 KiB
//             or 512 B) per group of the tile, up to four; thread t decodes index row n0 + (t mod 128) for the whole kernel and keeps
//             a pointer to its row's table.  A column at or past the end of the split is written as 0, never table[0].
//   k_cbpkdc_mfma_grouped  m > 16.  dcm_accumulate unchanged, then k_cbpkdc_mfma's epilogue with one set of [K][64] bins per group of
//             the tile: the 32 rows of an accumulator lie in one group, so the set is a scalar; one cbdc_flush per set.
// No load leaves the packed buffer; everything past m, kdim, ncols and the end of a split is zero in the images, never memory.
#include "nnc_cbgrad_grouped.hpp"
#include "nnc_cbgrad_h16.hpp"
#include "nnc_cbh16plan.hpp"
#include "nnc_cbpkgrad_grouped.hpp"

// ------------------------------------------------------------------ dx, m > 16
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads; out, direct and cols_per_split as k_cbdx_mfma.  LDS: `tables`
// tables [ENTRIES][PK_COPIES] (table t that of group n0 / group_rows + t), the staging rows of all of them, the two images.
template <typename XT, int BITS, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbpkdx_mfma_grouped(const XT *__restrict__ g, long long m, long long kdim,
                                                                    const unsigned char *__restrict__ packed, long long row_bytes, long long ncols,
                                                                    const float *__restrict__ centers, int k, int tables, long long col_tiles,
                                                                    long long cols_per_split, long long group_rows, int direct, void *__restrict__ out_)
{
    constexpr int ENTRIES = 1 << BITS, PER = 32 / BITS, NW = 16 / PER;   // NW: the dwords of a thread's 16 fields
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const int all = tables * ENTRIES;
    float *cb = hm_smem;                                // [tables][ENTRIES][PK_COPIES]
    float *stage = cb + (all << PK_CSHIFT);             // [tables][ENTRIES]
    XT *gs = reinterpret_cast<XT *>(hm_smem + hm_table_words(all, PK_CSHIFT));   // [HM_BM][HM_LD]: g tile, row-major in o
    XT *ws = gs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: W^T tile, [i][o]

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);   // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const TileGroups G = tile_groups_at(T.n0, kdim, group_rows);
    for (int j = threadIdx.x; j < all; j += HM_THREADS) {          // (a table past the last group repeats it, unread)
        const int t = j / ENTRIES, e = j % ENTRIES;
        stage[j] = e < k ? (float)(XT)centers[std::min(G.q0 + t, G.groups - 1) * k + e] : 0.0f;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < (all << PK_CSHIFT); w += HM_THREADS) cb[w] = stage[w >> PK_CSHIFT];

    const long long gi = T.n0 + T.wc;
    const bool row_ok = gi < kdim;
    const unsigned char *prow = packed + (row_ok ? gi * row_bytes : 0LL);
    const float *tab = cb + tile_group_of(G, gi, group_rows, tables) * (ENTRIES * PK_COPIES) + (T.lane & (PK_COPIES - 1));
    uint32_t lw[NW];

    auto load_w = [&](long long ob) {
        const long long o0 = ob + T.wk0;                // a multiple of 16: the 16 fields are 16 * BITS / 8 aligned bytes
#pragma unroll
        for (int d = 0; d < NW; ++d) lw[d] = 0u;
        if (row_ok && o0 < T.k_hi) {                    // (k_hi <= ncols: the bytes lie inside the padded row)
            const unsigned char *p = prow + o0 * BITS / 8;
            if constexpr (NW == 2) {
                const uint2 v = *reinterpret_cast<const uint2 *>(p);
                lw[0] = v.x, lw[1] = v.y;
            } else {
                lw[0] = *reinterpret_cast<const uint32_t *>(p);
            }
        }
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t l = (lw[j / PER] >> (BITS * (j % PER))) & MASK;
            // a column past the split, so every column past ncols, is 0 and not table[label 0 of the padding]
            w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? tab[l << PK_CSHIFT] : 0.0f;
        }
        hm_store_w(ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(g, m, ncols, T, gs, ws, acc, load_w, store_w);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads.  LDS: the two images, then `sets` sets of bins [k][64] int64 (copy
// `lane` of every bin this lane's own), set t for group m0 / group_rows + t.
template <typename XT, int BITS, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbpkdc_mfma_grouped(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                                    const unsigned char *__restrict__ packed, long long row_bytes, long long ncols, int k,
                                                                    int sets, int terms_log2, long long col_tiles, long long rows_per_split,
                                                                    long long group_rows, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    XT *xs = reinterpret_cast<XT *>(hm_smem);           // [HM_BM][HM_LD]: x^T tile, [i][r]
    XT *gs = xs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: g^T tile, [o][r]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + HM_BN * HM_LD);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, (sets * k) << PKG_RLOG2, scx, scg, Sw)) return;   // (uniform over the launch)
    dcm_scales<XT>(scx, scg, Sw);

    const HmTile T = hm_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i, [k_lo, k_hi): rows r
    typename HFrag<XT>::C acc[2][2];
    dcm_accumulate<XT, XVEC>(x, g, kdim, ncols, T, scx, scg, xs, gs, acc);

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col): its 32 rows lie in one group, whose set is a scalar; the 32 lanes
    // of a row read 32 consecutive fields of packed row i, and a lane's dword lies inside the padded row when its column lies inside
    // the matrix
    const TileGroups G = tile_groups_at(T.m0, kdim, group_rows);
    const long long row0 = tile_wave_row0(T.m0);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int set = (int)tile_group_of(G, row0 + a * 32, group_rows, sets);
        unsigned long long *mybins = bins + (((long long)set * k) << PKG_RLOG2) + T.lane;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const long long o = hm_acc_col(T.n0 + T.wn, b, T.lane);
            if (o >= ncols) continue;
            const long long bitpos = o * BITS;
            const unsigned char *pcol = packed + ((bitpos >> 5) << 2);
            const int sh = (int)(bitpos & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = hm_acc_row(T.m0 + T.wm, a, r, T.lane);
                if (i >= kdim) continue;
                const uint32_t l = (*reinterpret_cast<const uint32_t *>(pcol + i * row_bytes) >> sh) & MASK;
                if (l < (uint32_t)k) atomicAdd(&mybins[l << PKG_RLOG2], cbdc_fix(acc[a][b][r], Sw));
            }
        }
    }
    for (int t = 0; t < sets && G.q0 + t < G.groups; ++t) cbdc_flush(bins + (((long long)t * k) << PKG_RLOG2), k, PKG_RLOG2, sums + (G.q0 + t) * k);
}

// ------------------------------------------------------------------ plans (host)
// m <= 16 and the empty shapes: section 15's plans (pg_dx_plan, pg_dc_plan) with section 20's per-wave tables.  m > 16:
// nnc_cbh16plan.hpp's tiles and splits, so those of nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16, with the LDS of the tables / sets of the
// tile's groups.
static PgPlan pgh_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int64_t group_rows, int cus, int &tables)
{
    if (h16_mfma_shape(m, kdim, ncols)) {
        tables = tile_groups(group_rows);
        PgPlan p = h16_mfma_plan<PgPlan>(h16_dx_tiles(m, kdim, ncols), (long long)hm_table_words(tables << bits, PK_CSHIFT) * 4);
        p.entries = 1 << bits;
        p.copies = PK_COPIES;
        return p;
    }
    PgPlan p = pg_dx_plan(m, kdim, ncols, bits, cus);
    tables = 0;
    if (p.path == NNC_CBMM_STREAM) {
        tables = CB_WAVES;
        p.lds = (long long)CB_WAVES * p.entries * PK_COPIES * 4;
    }
    return p;
}

static int pgh_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int cus, PgPlan &p, int &sets)
{
    if (h16_mfma_shape(m, kdim, ncols)) {
        sets = tile_groups(group_rows);
        p = h16_mfma_plan<PgPlan>(h16_dc_tiles(m, kdim, ncols), (((long long)sets * k) << PKG_RLOG2) * 8);
        p.copies = 1 << PKG_RLOG2;
        return NNC_OK;
    }
    const int rc = pg_dc_plan(m, kdim, ncols, bits, k, cus, p);
    sets = p.path == NNC_CBMM_STREAM ? 1 : 0;
    return rc;
}

// ------------------------------------------------------------------ launches
template <typename XT, int BITS, int VB, int MT>
static void launch_dx_stream(dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const unsigned char *packed, long long row_bytes,
                             long long ncols, const float *centers, int k, long long rpg, long long group_rows, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbpkdx_stream_grouped<XT, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(g), m, kdim, packed, row_bytes,
                       ncols, centers, k, rpg, group_rows, direct, out);
}

template <typename XT, int BITS, int VB, int MT>
static void launch_dc_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const unsigned char *packed,
                             long long row_bytes, long long ncols, int k, int tl, long long rpg, long long group_rows, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbpkdc_stream_grouped<XT, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x),
                       reinterpret_cast<const XT *>(g), m, kdim, packed, row_bytes, ncols, k, tl, rpg, group_rows, hdr, sums);
}

template <typename XT, int BITS>
static void launch_dx_mfma(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const unsigned char *packed, long long row_bytes,
                           long long ncols, const float *centers, int k, int tables, long long col_tiles, long long cps, long long group_rows, int direct,
                           void *out)
{
    hm_launch(g, ncols, k_cbpkdx_mfma_grouped<XT, BITS, true>, k_cbpkdx_mfma_grouped<XT, BITS, false>, grid, lds, s, reinterpret_cast<const XT *>(g), m, kdim,
              packed, row_bytes, ncols, centers, k, tables, col_tiles, cps, group_rows, direct, out);
}

template <typename XT, int BITS>
static void launch_dc_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const unsigned char *packed,
                           long long row_bytes, long long ncols, int k, int sets, int tl, long long col_tiles, long long rps, long long group_rows,
                           uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((dcm_xvec(x, g, kdim, ncols) ? k_cbpkdc_mfma_grouped<XT, BITS, true> : k_cbpkdc_mfma_grouped<XT, BITS, false>), grid, dim3(HM_THREADS),
                       lds, s, reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim, packed, row_bytes, ncols, k, sets, tl, col_tiles, rps,
                       group_rows, hdr, sums);
}

// every kernel instantiation of this unit: per dtype the stream list of nnc_cbpkgrad.hpp (one shared case list), and the MFMA ones
using DxStream = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const unsigned char *, long long, long long, const float *, int, long long,
                          long long, int, void *);
using DcStream = void (*)(dim3, size_t, hipStream_t, const void *, const void *, int, long long, const unsigned char *, long long, long long, int, int,
                          long long, long long, uint32_t *, unsigned long long *);
using DxMfma = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const unsigned char *, long long, long long, const float *, int, int,
                        long long, long long, long long, int, void *);
using DcMfma = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const unsigned char *, long long, long long, int, int, int,
                        long long, long long, long long, uint32_t *, unsigned long long *);
struct StreamCase {
    int a, vb, mt;            // a: bits
    DxStream dx;
    DcStream dc;
};
struct MfmaCase {
    int dt, a;                // a: bits
    DxMfma dx;
    DcMfma dc;
};
#define BF_CASE(B, V, M) {B, V, M, launch_dx_stream<bf16_t, B, V, M>, launch_dc_stream<bf16_t, B, V, M>},
#define HF_CASE(B, V, M) {B, V, M, launch_dx_stream<f16_t, B, V, M>, launch_dc_stream<f16_t, B, V, M>},
static const StreamCase kBf16Cases[] = {PKG_STREAM_CASES(BF_CASE)};
static const StreamCase kF16Cases[] = {PKG_STREAM_CASES(HF_CASE)};
#undef BF_CASE
#undef HF_CASE
static const MfmaCase kMfmaCases[] = {
    {NNC_DT_BF16, 4, launch_dx_mfma<bf16_t, 4>, launch_dc_mfma<bf16_t, 4>}, {NNC_DT_BF16, 2, launch_dx_mfma<bf16_t, 2>, launch_dc_mfma<bf16_t, 2>},
    {NNC_DT_F16, 4, launch_dx_mfma<f16_t, 4>, launch_dc_mfma<f16_t, 4>},   {NNC_DT_F16, 2, launch_dx_mfma<f16_t, 2>, launch_dc_mfma<f16_t, 2>},
};
static const CbgCaseNames kPkNames = {true, "bits", true};

// ------------------------------------------------------------------ C ABI
static int pgh_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows)
{
    const int rc = h16_check_dtype(fn, x_dtype);
    return rc != NNC_OK ? rc : pgg_check(fn, m, kdim, ncols, bits, k, group_rows);
}

static void pgh_plan_tail(const PgPlan &p, int64_t kdim, int64_t group_rows, int held, int64_t *out)
{
    cbg_grouped_plan_tail(p.path == NNC_CBMM_MFMA ? NNC_CBMM_TILED : p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out);
    out[4] = held;
}

extern "C" int64_t nnc_cbpk_grouped_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    return nnc_cbpk_dx_h16_workspace_bytes(m, kdim, ncols, bits);
}

extern "C" int nnc_cbpk_grouped_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus,
                                            int64_t *out)
{
    const char *fn = "nnc_cbpk_grouped_dx_h16_plan";
    int rc = pgh_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, std::string(fn) + ": cus < 1");
    if (!out) return fail(NNC_EINVAL, std::string(fn) + ": out is NULL");
    PgPlan p;
    int tables;
    p = pgh_dx_plan(m, kdim, ncols, bits, group_rows, cus, tables);
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    if ((rc = nnc_cbpk_dx_h16_plan(x_dtype, m, kdim, ncols, bits, k, cus, out)) != NNC_OK) return rc;   // the shared fields: the ungrouped record
    out[NNC_CBPKDX_P_LDS] = p.lds;                                                                     // (the tables of the groups)
    pgh_plan_tail(p, kdim, group_rows, tables, out + NNC_CBPKDX_H16_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbpk_grouped_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                                       int64_t ncols, const float *centers_dev, int32_t k, int64_t group_rows, void *dx, int dx_dtype, void *workspace,
                                       int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbpk_grouped_dx_h16";
    int rc = pgh_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_h16: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_h16: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_h16: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_h16: g is NULL");
    if (reinterpret_cast<uintptr_t>(g) % 2 || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbpk_grouped_dx_h16: g or dx is not aligned to its element size");
    const int64_t need = nnc_cbpk_grouped_dx_h16_workspace_bytes(m, kdim, ncols, bits);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_grouped_dx_h16_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK)
        return rc;
    PgPlan p;
    int tables;
    p = pgh_dx_plan(m, kdim, ncols, bits, group_rows, CB_PLAN_CUS, tables);
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kPkNames, p.path, x_dtype, bits, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM) p = pgh_dx_plan(m, kdim, ncols, bits, group_rows, cu_count(), tables);   // (the row groups of this device)
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, pk, row_bytes, ncols, centers_dev, k, p.rows_per_group,
                   group_rows, direct, out);
            LAUNCHCHK("k_cbpkdx_stream_grouped (h16)");
        } else {
            mc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, pk, row_bytes, ncols,
                                        centers_dev, k, tables, p.col_tiles, p.per_split, group_rows, direct, out);
            LAUNCHCHK("k_cbpkdx_mfma_grouped");
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbpk_grouped_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows)
{
    if (pgg_check("nnc_cbpk_grouped_dc_h16_workspace_bytes", m, kdim, ncols, bits, k, group_rows) != NNC_OK) return 0;
    return h16_dc_ws_bytes(m == 0 || kdim == 0 || ncols == 0 ? NNC_CBMM_ZERO : NNC_CBMM_STREAM, gg_groups(kdim, group_rows) * k);
}

extern "C" int nnc_cbpk_grouped_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus,
                                            int64_t *out)
{
    const char *fn = "nnc_cbpk_grouped_dc_h16_plan";
    int rc = pgh_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, std::string(fn) + ": cus < 1");
    if (!out) return fail(NNC_EINVAL, std::string(fn) + ": out is NULL");
    PgPlan p;
    int sets;
    if ((rc = pgh_dc_plan(m, kdim, ncols, bits, k, group_rows, cus, p, sets)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, cus, out)) != NNC_OK) return rc;
    if ((rc = nnc_cbpk_dc_h16_plan(x_dtype, m, kdim, ncols, bits, k, cus, out)) != NNC_OK) return rc;   // the shared fields: the ungrouped record
    out[NNC_CBPKDC_P_LDS] = p.lds;                                                                     // (a set of bins per group)
    out[NNC_CBPKDC_P_WORKSPACE] = h16_dc_ws_bytes(p.path, gg_groups(kdim, group_rows) * k);            // (G * k bins)
    pgh_plan_tail(p, kdim, group_rows, sets, out + NNC_CBPKDC_H16_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbpk_grouped_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                                       int64_t ncols, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes,
                                       void *stream)
{
    const char *fn = "nnc_cbpk_grouped_dc_h16";
    int rc = pgh_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dc_h16: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbpk_grouped_dc_h16: x or g is NULL");
    if (reinterpret_cast<uintptr_t>(x) % 2 || reinterpret_cast<uintptr_t>(g) % 2)
        return fail(NNC_EINVAL, "nnc_cbpk_grouped_dc_h16: x or g is not aligned to its element size");
    PgPlan p;
    int sets;
    if ((rc = pgh_dc_plan(m, kdim, ncols, bits, k, group_rows, CB_PLAN_CUS, p, sets)) != NNC_OK) return rc;
    const int nbins = (int)(gg_groups(kdim, group_rows) * k);
    const int64_t need = h16_dc_ws_bytes(p.path, nbins);
    if ((rc = cb_check_workspace(fn, "nnc_cbpk_grouped_dc_h16_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK)
        return rc;
    const StreamCase *sc;
    if ((rc = cbg_stream_case(fn, h16_cases(x_dtype, kBf16Cases, kF16Cases), kPkNames, p.path, bits, p.vb, p.mt, sc)) != NNC_OK) return rc;
    const MfmaCase *mc;
    if ((rc = h16_mfma_case(fn, kMfmaCases, kPkNames, p.path, x_dtype, bits, mc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM && (rc = pgh_dc_plan(m, kdim, ncols, bits, k, group_rows, cu_count(), p, sets)) != NNC_OK)
        return rc;                                                                        // (the row groups of this device)
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, pk, row_bytes, ncols, k, p.terms_log2,
                   p.rows_per_group, group_rows, hdr, sums);
            LAUNCHCHK("k_cbpkdc_stream_grouped (h16)");
        } else {
            mc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, pk, row_bytes, ncols, k,
                                        sets, p.terms_log2, p.col_tiles, p.per_split, group_rows, hdr, sums);
            LAUNCHCHK("k_cbpkdc_mfma_grouped");
        }
        return NNC_OK;
    });
}
