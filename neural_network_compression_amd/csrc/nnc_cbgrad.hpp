// nnc_cbgrad.hpp -- what the backward pass of the codebook matmul (nnc_cbgrad.hip) shares with those of its bitmap-sparse and
// packed siblings (nnc_cbspgrad.hip, nnc_cbpkgrad.hip): the fixed-order wave reduction of the dx stream kernels, the scaling and fixed-point binning of dc (DESIGN.md
// section 12), the workspace sizes and the launches of the kernels both use (defined in nnc_cbgrad.hip).  The tiled kernels' shared
// text is in nnc_cbtile.hpp.  The host plans of the byte form (CgPlan, dx_plan, dc_plan) and its argument checks (cg_check) are here
// too: the group-wise backward pass (nnc_cbgrad_grouped.hip) follows the same plans.
#pragma once
#include "nnc_cbmm.hpp"

#define CBG_FLAG_OK 0
#define CBG_FLAG_NONFINITE 1   // x or g holds Inf / NaN, or m * max|x| * max|g| >= 2^127: dc is NaN
#define CBG_FLAG_ZERO 2        // max|x| or max|g| is 0: every dW is 0
#define CBG_HDR_BYTES 64       // dc workspace: {max|x| bits, max|g| bits, S, flag} then int64 sums[K] at byte 64

// The m partials of every lane summed over the wave: a reduce-scatter (at lane bit 32 >> t the lanes with the bit set keep the upper
// half of the rows they hold and take their partner's; then the rest of the butterfly on one value).  N + log2(64 / N) shuffles
// instead of 6 N; every pair adds in a fixed order, so the sum depends on the data only.  Returns the total of row `row`, the
// same on every lane of a group of 64 / N lanes.  Both candidates of an exchange are read into values before the select: a select
// between two elements of the array is a select between two addresses to the compiler, which at N = 16 keeps the array in scratch.
template <int N>
__device__ __forceinline__ float wave_reduce_rows(float (&v)[N], int lane, int &row)
{
    row = 0;
#pragma unroll
    for (int t = 0; (N >> t) > 1; ++t) {
        const int half = N >> (t + 1), bit = 32 >> t;
        const bool up = (lane & bit) != 0;
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const float a = v[j], b = v[j + half];
            v[j] = (up ? b : a) + __shfl_xor(up ? a : b, bit);
        }
        row += up ? half : 0;
    }
    float s = v[0];
#pragma unroll
    for (int bit = 64 / N / 2; bit >= 1; bit >>= 1) s += __shfl_xor(s, bit);
    return s;
}

// the workspaces of the backward entry points: dx, the partials [splits][m][kdim] when ncols is split; dc, the header and int64 sums[k]
static inline int64_t cbg_dx_ws_bytes(long long splits, long long m, long long kdim) { return splits > 1 ? (int64_t)splits * m * kdim * 4 : 0; }
static inline int64_t cbg_dc_ws_bytes(int path, int k) { return path == NNC_CBMM_STREAM || path == NNC_CBMM_TILED ? CBG_HDR_BYTES + 8LL * k : 0; }

// S of the dc sums from the maxima k_cbgrad_absmax left (uniform over the launch); flag as CBG_FLAG_*
__device__ __forceinline__ int cbdc_shift(const uint32_t *amax, long long m, int terms_log2, int &flag)
{
    const uint32_t ux = amax[0], ug = amax[1];
    flag = CBG_FLAG_OK;
    if (ux >= 0x7F800000u || ug >= 0x7F800000u) {
        flag = CBG_FLAG_NONFINITE;
        return 0;
    }
    const double bound = (double)m * (double)__uint_as_float(ux) * (double)__uint_as_float(ug);
    if (!(bound > 0.0)) {
        flag = CBG_FLAG_ZERO;
        return 0;
    }
    int P = 0;
    (void)frexp(bound, &P);   // bound = f * 2^P, f in [0.5, 1): 2^P > bound
    if (P > 127) {
        flag = CBG_FLAG_NONFINITE;
        return 0;
    }
    return 62 - terms_log2 - P;
}

// e with |v| = f * 2^e, f in [0.5, 1), of a finite non-zero |v| given as bits (subnormals included)
__device__ __forceinline__ int cbdc_exp(uint32_t bits)
{
    const int E = (int)(bits >> 23);
    return E ? E - 126 : (32 - __clz((int)bits)) - 149;
}

// The exponents scx, scg that bring max |x| and max |g| (k_cbgrad_absmax's bits, finite and non-zero: CBG_FLAG_OK) to [0.5, 1).
// The dc kernels scale every x by 2^scx and every g by 2^scg as they load them (v_ldexp_f32: exact, a float32 multiplier cannot
// hold 2^+-149), so dW' = dW * 2^(scx + scg) is formed in float32's normal range whatever the magnitudes; they bin
// rint(dW' * 2^(S - scx - scg)).
__device__ __forceinline__ void cbdc_scales(const uint32_t *amax, int &scx, int &scg)
{
    scx = -cbdc_exp(amax[0]);
    scg = -cbdc_exp(amax[1]);
}

// The loads of the dc kernels are made whatever the guard says (of v[0], which they always have, finite, where it is false) and
// cbdc_scaled(value, guard, s) is value * 2^s, or +-0 (the value * 2^-512) where the guard is false: a guarded load followed by
// the scaling compiles to a branch that waits for each load in turn.  A batch of loads goes first, then a sched_barrier, then
// the scaling, so that the loads of the batch are in flight together.
__device__ __forceinline__ long long cbdc_idx(long long idx, bool ok) { return ok ? idx : 0; }
__device__ __forceinline__ float cbdc_scaled(float v, bool ok, int s) { return ldexpf(v, ok ? s : -512); }

// the fixed-point image of one dW: exact scaling by 2^S (|v * 2^S| < 2^63), nearest integer, ties to even
__device__ __forceinline__ unsigned long long cbdc_fix(float v, int S) { return (unsigned long long)(long long)rintf(ldexpf(v, S)); }

// the workgroup's bins into the global sums (integer atomics), copies summed in order; zero bins are skipped
__device__ __forceinline__ void cbdc_flush(const unsigned long long *bins, int k, int rlog2, unsigned long long *__restrict__ sums)
{
    __syncthreads();
    const int R = 1 << rlog2;
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        unsigned long long s = 0;
        for (int r = 0; r < R; ++r) s += bins[(j << rlog2) + r];
        if (s) atomicAdd(&sums[j], s);
    }
}

// ------------------------------------------------------------------ plans (host)
struct CgPlan {
    int path;                 // NNC_CBMM_NONE / _STREAM / _TILED / _ZERO
    int vb, mt;               // stream: bytes per lane per row, rows of m per launch (a power of two >= m)
    int entries, cshift;      // dx stream: the LDS codebook (entries x (1 << cshift) copies); tiled: k + 1 entries
    int rlog2;                // dc: 1 << rlog2 copies of every LDS bin
    int aligned;
    long long col_tiles, row_tiles;   // stream: column blocks x row groups; tiled: tiles
    long long splits, per_split;      // dx: splits of ncols (columns per split); dc: splits of m (rows of m per split)
    long long rows_per_group;         // stream: label rows per workgroup
    int terms_log2;                   // dc: ceil(log2(kdim * ncols * splits))
    long long lds;
};

static int ceil_log2(long long v)
{
    int l = 0;
    while (l < 62 && (1LL << l) < v) ++l;
    return l;
}

// the stream geometry both directions share: a column block of 64 lanes x E labels, row groups for two workgroups per CU
static void cg_stream_grid(CgPlan &p, long long m, long long kdim, long long ncols, int lb, int cus, uintptr_t labels)
{
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    p.path = NNC_CBMM_STREAM;
    p.mt = cb_mt(m);
    p.vb = std::min(16, (64 / p.mt) * lb);
    p.col_tiles = cdiv(ncols, 64LL * (p.vb / lb));
    const long long groups = std::max(1LL, std::min(cdiv(2LL * cus, p.col_tiles), cdiv(kdim, (long long)CB_WAVES * CB_UNROLL)));
    p.rows_per_group = cdiv(kdim, groups);
    p.row_tiles = cdiv(kdim, p.rows_per_group);
    p.aligned = labels % p.vb == 0 && (ncols * lb) % p.vb == 0;
}

static CgPlan dx_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus, uintptr_t labels)
{
    CgPlan p{};
    if (m == 0 || kdim == 0) return p;                       // NNC_CBMM_NONE: dx is empty
    if (ncols == 0) {                                        // dx = 0
        p.path = NNC_CBMM_ZERO;
        return p;
    }
    if (m <= CB_SKINNY_M) {
        cg_stream_grid(p, m, kdim, ncols, lb, cus, labels);
        p.splits = p.col_tiles;                              // one split per column block
        p.per_split = 64LL * (p.vb / lb);
        if (lb == 1) {
            p.entries = 256;
            p.cshift = __builtin_ctz(CB_U8_COPIES);
        } else {
            p.entries = k + 1;
            while ((1 << p.cshift) < CB_U8_COPIES && (long long)p.entries << (p.cshift + 1) <= CB_U16_WORDS) ++p.cshift;
        }
        p.lds = ((long long)p.entries << p.cshift) * 4 + (long long)p.entries * 4;
    } else {
        p.path = NNC_CBMM_TILED;
        p.col_tiles = cdiv(kdim, TB_N);
        p.row_tiles = cdiv(m, TB_M);
        long long s = std::min({cdiv(2LL * CB_PLAN_CUS, p.col_tiles * p.row_tiles), ncols / (16 * TB_K), 16LL});
        s = std::max(1LL, s);
        p.per_split = cdiv(ncols, s);
        p.splits = cdiv(ncols, p.per_split);
        p.entries = k + 1;
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + k + 1) * 4;
    }
    return p;
}

static int dc_rlog2(int k) { return k <= 64 ? 5 : (k <= 256 ? 3 : 1); }   // as k_centroid_grad: K x copies x 8 B <= 16.3 KiB

static CgPlan dc_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus, uintptr_t labels)
{
    CgPlan p{};
    if (m == 0 || kdim == 0 || ncols == 0) {                 // no terms: dc = 0
        p.path = NNC_CBMM_ZERO;
        return p;
    }
    p.rlog2 = dc_rlog2(k);
    const long long bins = ((long long)k << p.rlog2) * 8;
    if (m <= CB_SKINNY_M) {
        cg_stream_grid(p, m, kdim, ncols, lb, cus, labels);
        p.splits = 1;
        p.per_split = m;
        p.lds = bins;
    } else {
        p.path = NNC_CBMM_TILED;
        p.col_tiles = cdiv(ncols, TB_N);
        p.row_tiles = cdiv(kdim, TB_M);
        long long s = std::min({cdiv(2LL * CB_PLAN_CUS, p.col_tiles * p.row_tiles), m / (16 * TB_K), 16LL});
        s = std::max(1LL, s);
        p.per_split = cdiv(m, s);
        p.splits = cdiv(m, p.per_split);
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N) * 4 + bins;
    }
    p.terms_log2 = ceil_log2(kdim * ncols * p.splits);
    return p;
}

// the argument checks of the byte form's backward entry points (NNC_EINVAL, or NNC_OK)
static int cg_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    const std::string f(fn);
    if (m < 0 || kdim < 0 || ncols < 0) return fail(NNC_EINVAL, f + ": negative size");
    if (label_bytes != 1 && label_bytes != 2) return fail(NNC_EINVAL, f + ": label_bytes must be 1 or 2");
    if (k < 1 || k > NNC_KMAX) return fail(NNC_EINVAL, f + ": k outside 1..NNC_KMAX");
    if (label_bytes == 1 && k > 256) return fail(NNC_EINVAL, f + ": k > 256 needs 2-byte labels");
    if (m > (1LL << 40) || kdim > (1LL << 40) || ncols > (1LL << 40)) return fail(NNC_EINVAL, f + ": size too large");
    if (m > 0 && kdim > 0 && ncols > 0 && (kdim > (1LL << 62) / ncols || kdim * ncols > (1LL << 62) / (16 * TB_K)))
        return fail(NNC_EINVAL, f + ": kdim * ncols too large");
    return NNC_OK;
}

// ------------------------------------------------------------------ groups (host): the group-wise backward passes (nnc_cbgrad_grouped.hip, nnc_cbpkgrad_grouped.hip)
// the most groups the 128 index rows of a tile lie in: tiles start on multiples of 128, group_rows is a multiple of 32
static inline int tile_groups(long long group_rows) { return group_rows % 128 == 0 ? 1 : (group_rows == 32 ? 4 : 2); }

// G as the layers count it: centers and dc have a row even where kdim = 0
static inline long long gg_groups(long long kdim, long long group_rows) { return std::max(1LL, cdiv(kdim, group_rows)); }

// the shared kernels of nnc_cbgrad.hip, launched on `s` (NNC_OK, or the launch error):
//   cbgrad_absmax  amax[0..1] = bits of max |x[0, nx)|, max |g[0, ng)| (amax zeroed by the caller)   k_cbgrad_absmax
//   cbgrad_reduce  out[idx] = sum over s < splits of part[s * mn + idx], in split order                k_cbgrad_reduce
//   cbdc_finish    dc[j] = ldexp(sums[j], -S), float64 or float32; NaN on CBG_FLAG_NONFINITE          k_cbdc_finish
int cbgrad_absmax(const float *x, long long nx, const float *g, long long ng, uint32_t *amax, hipStream_t s);
int cbgrad_reduce(const float *part, long long splits, long long mn, float *out, hipStream_t s);
int cbdc_finish(const uint32_t *hdr, const long long *sums, int k, int f64, void *out, hipStream_t s);
