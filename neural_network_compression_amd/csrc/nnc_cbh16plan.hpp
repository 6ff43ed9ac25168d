// nnc_cbh16plan.hpp -- the host side the five backward units on bf16 / fp16 activations share (nnc_cbgrad_h16.hip, nnc_cbspgrad_h16.hip,
// nnc_cbpk_h16.hip, nnc_cbgrad_grouped_h16.hip, nnc_cbpkgrad_grouped_h16.hip): the MFMA plan of m > 16, which
// depends on the shape alone, and the pieces of glue beside nnc_cbgrad.hpp's that only the half units need.  A unit adds what its
// index form fixes: the table or the bins in the LDS, the fields of its own record.
#pragma once
#include "nnc_cbgrad.hpp"

// ------------------------------------------------------------------ the MFMA plan, m > 16
// The 128 x 128 tiles of the output, the reduced dimension split by section 16's rule for CB_PLAN_CUS compute units whatever the
// device (cus changes the stream grid only), and the two LDS images of nnc_cbmfma.hpp's tile.
struct H16Tiles {
    long long col_tiles, row_tiles, splits, per_split;
    int terms_log2;           // dc: ceil(log2(kdim * ncols * splits)), S's T; dx: 0
    long long image_bytes;
};

static inline long long h16_splits(long long tiles, long long extent, long long &per_split)
{
    const long long s = std::max(1LL, std::min({cdiv(2LL * CB_PLAN_CUS, tiles), extent / (2 * HM_BK), 16LL}));
    per_split = cdiv(cdiv(extent, s), HM_BK) * HM_BK;   // every split starts on a whole step
    return cdiv(extent, per_split);
}

static inline H16Tiles h16_tiles(long long cols, long long rows, long long extent)
{
    H16Tiles t{};
    t.col_tiles = cdiv(cols, HM_BN);
    t.row_tiles = cdiv(rows, HM_BM);
    t.splits = h16_splits(t.col_tiles * t.row_tiles, extent, t.per_split);
    t.image_bytes = (long long)(HM_BM + HM_BN) * HM_LD * 2;
    return t;
}

// dx [m][kdim]: tiles of kdim x m, ncols split
static inline H16Tiles h16_dx_tiles(long long m, long long kdim, long long ncols) { return h16_tiles(kdim, m, ncols); }

// dW [kdim][ncols]: tiles of ncols x kdim, m split
static inline H16Tiles h16_dc_tiles(long long m, long long kdim, long long ncols)
{
    H16Tiles t = h16_tiles(ncols, kdim, m);
    t.terms_log2 = ceil_log2(kdim * ncols * t.splits);
    return t;
}

// the fields every unit's plan struct (CgPlan, SgPlan, PgPlan) has for them; form_lds: the table (dx) or the bins (dc) of the form
template <typename Plan> static inline Plan h16_mfma_plan(const H16Tiles &t, long long form_lds)
{
    Plan p{};
    p.path = NNC_CBMM_MFMA;
    p.col_tiles = t.col_tiles, p.row_tiles = t.row_tiles, p.splits = t.splits, p.per_split = t.per_split;
    p.terms_log2 = t.terms_log2;
    p.lds = t.image_bytes + form_lds;
    return p;
}

static inline bool h16_mfma_shape(long long m, long long kdim, long long ncols) { return m > CB_SKINNY_M && kdim > 0 && ncols > 0; }

// ------------------------------------------------------------------ the glue of the half entry points
static inline int h16_check_dtype(const char *fn, int x_dtype)
{
    if (x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16) return fail(NNC_EINVAL, std::string(fn) + ": x_dtype must be NNC_DT_BF16 or NNC_DT_F16");
    return NNC_OK;
}

// the dc workspace on either path: the header, then the int64 sums of the nbins bins
static inline int64_t h16_dc_ws_bytes(int path, long long nbins) { return path == NNC_CBMM_ZERO ? 0 : CBG_HDR_BYTES + 8LL * nbins; }

// the table of a unit's stream instantiations for x_dtype: one per dtype, the same cases (N)
template <typename Case, size_t N> static inline const Case (&h16_cases(int dt, const Case (&bf16)[N], const Case (&f16)[N]))[N]
{
    return dt == NNC_DT_BF16 ? bf16 : f16;
}

// The MFMA instantiation a plan asks for, in the wording of cbg_stream_case: c = the entry {dt, a} of `cases` where the path is
// NNC_CBMM_MFMA (NNC_EINVAL if the table has none), NULL on every other path.  a is label_bytes or bits, n.first its name.
template <typename Case, size_t N>
static int h16_mfma_case(const char *fn, const Case (&cases)[N], const CbgCaseNames &n, int path, int dt, int a, const Case *&c)
{
    c = nullptr;
    if (path != NNC_CBMM_MFMA) return NNC_OK;
    for (const Case &e : cases)
        if (e.dt == dt && e.a == a) c = &e;
    if (c) return NNC_OK;
    return fail(NNC_EINVAL, std::string(fn) + ": no MFMA instantiation for dtype " + std::to_string(dt) +
                                (n.first ? ", " + (n.first + (" " + std::to_string(a))) : std::string()));
}
