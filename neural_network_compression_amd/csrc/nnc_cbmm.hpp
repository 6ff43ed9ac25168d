// nnc_cbmm.hpp -- what the codebook matmul (nnc_cbmm.hip), its bitmap-sparse sibling (nnc_cbsp.hip) and its backward pass
// (nnc_cbgrad.hip) share: the launch constants, the per-bank LDS codebook layout, the label-row loads of the stream kernels and the
// register-blocked FMA step of the tiled kernels.  The 2- and 4-bit packed form (nnc_cbpk.hip) takes cb_fill, tb_tile_fma and
// the split-K combine from here.  The plan (cb_plan) and the stream kernel k_cbmm_stream itself live here too, templated on the
// type of x: nnc_cbmm.hip instantiates them for float32, nnc_cbmm_h16.hip for bf16 / fp16 activations.  The group-wise unit
// (nnc_cbmm_grouped.hip: one codebook per block of rows) follows the same plan and takes cb_fill, cb_refill, the label-row loads,
// tb_tile_fma and HFrag from here.  cb_mt and cb_check_workspace serve every entry point of the nnc_cb*.hip units; cb_check_operands,
// cb_direct and cb_finish the five forward units that take half x (nnc_cbmm_h16, nnc_cbmm_grouped, nnc_cbpk_grouped, nnc_cbsp_h16,
// nnc_cbsp_grouped_h16).  The MFMA tile and the k loop of those five, and of the dx kernels of the half backward units, is
// nnc_cbmfma.hpp.
#pragma once
#include "nnc_common.hpp"
#include <type_traits>

#define CB_WAVES 4
#define CB_THREADS (CB_WAVES * WAVE)
#define CB_UNROLL 8               // label rows in flight per wave
#define CB_SKINNY_M 16
#define CB_U8_COPIES 32           // K <= 256 (uint8): 32 copies of a 256-entry table (zero-padded: no bounds test) = 32 KiB
#define CB_U16_WORDS 8448         // K > 256 (uint16): copies = the largest power of two with (K + 1) * copies <= this (33 KiB)
#define CB_PLAN_CUS 256           // the workspace query plans for this many CUs (the plan's splits never shrink with more)
#define TB_M 128
#define TB_N 128
#define TB_K 8

using bf16_t = __bf16;      // the 2-byte activation types of nnc_cbmm_h16 (NNC_DT_BF16, NNC_DT_F16)
using f16_t = _Float16;

#define HM_BM 128                 // k_cbmm_mfma (nnc_cbmm_h16.hip): the output tile of a workgroup,
#define HM_BN 128
#define HM_BK 32                  // its k step,
#define HM_LD 40                  // the 2-byte elements per row of its LDS images: HM_BK of k and 16 bytes of padding,
#define HM_THREADS 256            // and its threads

// the MFMA of the two 2-byte types: 8 values of A and of B per lane, a 32 x 32 float32 tile of 16 registers
template <typename XT> struct HFrag;
template <> struct HFrag<bf16_t> {
    typedef bf16_t V __attribute__((ext_vector_type(8)));
    typedef float C __attribute__((ext_vector_type(16)));
    __device__ static __forceinline__ C mfma(V a, V b, C c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct HFrag<f16_t> {
    typedef f16_t V __attribute__((ext_vector_type(8)));
    typedef float C __attribute__((ext_vector_type(16)));
    __device__ static __forceinline__ C mfma(V a, V b, C c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

static inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
// the rows of x (of g in the backward pass) a stream kernel is instantiated for: the power of two >= m (m <= CB_SKINNY_M)
static inline int cb_mt(long long m) { return m <= 1 ? 1 : (m <= 2 ? 2 : (m <= 4 ? 4 : (m <= 8 ? 8 : 16))); }
// k_cbmm_mfma's table and its staging row, in float32 words, rounded up so that the images behind them start on 16 bytes
__host__ __device__ static inline int hm_table_words(int entries, int cshift) { return ((entries << cshift) + entries + 3) & ~3; }

// y[idx] = the split-K partials part[s][idx], s < splits, summed in an order that depends on `splits` alone, + bias[idx % ncols],
// ReLU (k_cbmm_reduce, nnc_cbmm.hip; splits = 0: y = bias or 0), launched on `s`: NNC_OK or the launch error
int cbmm_reduce(const float *part, long long splits, long long mn, long long ncols, const float *bias, int relu, float *y, hipStream_t s);
// the same sums written as y_dtype (NNC_DT_*): float32, or bf16 / fp16 with one rounding to nearest even of the float32 value
int cbmm_reduce_dt(const float *part, long long splits, long long mn, long long ncols, const float *bias, int relu, void *y, int y_dtype, hipStream_t s);

// ------------------------------------------------------------------ the plan (host)
// Every decision nnc_cbmm_f32 (and nnc_cbmm_h16, `mfma`: its m > 16 kernel is k_cbmm_mfma, nnc_cbmm_h16.hip) takes before it
// launches: which kernel, its instantiation, the LDS table, the grid and the K splits.  nnc_cbmm_plan / nnc_cbmm_h16_plan report
// it (include/nnc.h), so the tests can see which regime a call hits.
struct CbPlan {
    int path;                // NNC_CBMM_NONE / _STREAM / _TILED / _BIAS / _MFMA
    int vb, mt;              // stream: bytes per lane per row, rows of x per launch (a power of two >= m)
    int entries, cshift;     // the LDS codebook: entries (centres, then zeros) x (1 << cshift) copies
    int aligned;             // stream: every label row starts on a VB-byte boundary (no funnel shift)
    long long col_tiles, row_tiles;
    long long splits, rows_per_split;
    long long lds;           // dynamic LDS bytes of the main kernel
};

// the splits and tiles (m >= 1, kdim >= 1, ncols >= 1)
static inline void cb_grid(CbPlan &p, long long m, long long kdim, long long ncols, int lb, int cus, bool mfma)
{
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    long long s;
    if (m <= CB_SKINNY_M) {
        p.path = NNC_CBMM_STREAM;
        p.mt = cb_mt(m);
        const int e_max = 64 / p.mt;                                 // accumulators per lane <= 64
        p.vb = std::min(16, e_max * lb);
        p.row_tiles = 1;
        p.col_tiles = cdiv(ncols, 64LL * (p.vb / lb));
        // enough workgroups for two per CU; every wave keeps at least one batch of rows; the partials (splits x m x ncols x 4 B)
        // stay within a quarter of the index stream
        s = std::min({cdiv(2LL * cus, p.col_tiles), kdim / (CB_WAVES * CB_UNROLL), kdim * lb / (16 * m)});
    } else if (mfma) {
        p.path = NNC_CBMM_MFMA;
        p.col_tiles = cdiv(ncols, HM_BN);
        p.row_tiles = cdiv(m, HM_BM);
        // two workgroups per CU; every split keeps at least two HM_BK steps
        s = std::min({cdiv(2LL * cus, p.col_tiles * p.row_tiles), kdim / (2 * HM_BK), 16LL});
    } else {
        p.path = NNC_CBMM_TILED;
        p.col_tiles = cdiv(ncols, TB_N);
        p.row_tiles = cdiv(m, TB_M);
        s = std::min({cdiv(2LL * cus, p.col_tiles * p.row_tiles), kdim / (16 * TB_K), 16LL});
    }
    s = std::max(1LL, s);
    p.rows_per_split = cdiv(kdim, s);
    if (p.path == NNC_CBMM_MFMA) p.rows_per_split = cdiv(p.rows_per_split, HM_BK) * HM_BK;   // every split starts on a whole k step
    p.splits = cdiv(kdim, p.rows_per_split);
}

// the per-bank LDS table of a label width: its entries (uint8: 256, zero-padded; uint16: k + 1, entry k the out-of-range value) and
// the log2 of its copies (cshift zero on entry)
static inline void cb_table_shape(int lb, int k, int &entries, int &cshift)
{
    if (lb == 1) {
        entries = 256;
        cshift = __builtin_ctz(CB_U8_COPIES);
    } else {
        entries = k + 1;
        while ((1 << cshift) < CB_U8_COPIES && (long long)entries << (cshift + 1) <= CB_U16_WORDS) ++cshift;
    }
}

static inline CbPlan cb_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus, uintptr_t labels, bool mfma = false)
{
    CbPlan p{};
    if (m == 0 || ncols == 0) return p;                              // NNC_CBMM_NONE: nothing to write
    if (kdim == 0) {                                                 // y = bias (zeros without one), by k_cbmm_reduce
        p.path = NNC_CBMM_BIAS;
        return p;
    }
    cb_grid(p, m, kdim, ncols, lb, cus, mfma);
    if (p.path != NNC_CBMM_TILED) {   // the per-bank table of the stream kernels; k_cbmm_mfma looks its W tile up in the same one
        cb_table_shape(lb, k, p.entries, p.cshift);
        if (p.path == NNC_CBMM_MFMA) {
            p.lds = (long long)hm_table_words(p.entries, p.cshift) * 4 + (long long)(HM_BM + HM_BN) * HM_LD * 2;
        } else {
            p.aligned = labels % p.vb == 0 && (ncols * lb) % p.vb == 0;
            p.lds = ((long long)p.entries << p.cshift) * 4 + (long long)p.mt * (p.vb / lb) * 64 * 4 + (long long)p.entries * 4;
        }
    } else {
        p.entries = k + 1;
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + k + 1) * 4;
    }
    return p;
}

static inline int64_t cb_ws_bytes(const CbPlan &p, long long m, long long ncols) { return p.splits > 1 ? (int64_t)p.splits * m * ncols * 4 : 0; }

// The workspace checks of an entry point `fn` whose query `query` answered `need`, in the order every entry point makes them: a
// negative size (NNC_EINVAL), less than `need` (NNC_ENOSPACE), a NULL or, with `align` > 0, a misaligned pointer where bytes are
// needed (NNC_EINVAL; `misaligned` is the entry point's wording of the last).  NNC_OK otherwise.
static inline int cb_check_workspace(const char *fn, const char *query, const void *workspace, int64_t workspace_bytes, int64_t need, int align = 0,
                                     const char *misaligned = "")
{
    const std::string f(fn);
    if (workspace_bytes < 0) return fail(NNC_EINVAL, f + ": negative workspace size");
    if (workspace_bytes < need) return fail(NNC_ENOSPACE, f + ": workspace smaller than " + query + "()");
    if (need > 0 && !workspace) return fail(NNC_EINVAL, f + ": workspace is NULL");
    if (need > 0 && align > 0 && reinterpret_cast<uintptr_t>(workspace) % align) return fail(NNC_EINVAL, f + ": " + misaligned);
    return NNC_OK;
}

// The operand checks of a forward entry point `fn` (nnc_cbmm_h16, nnc_cbmm_grouped, nnc_cbpk_grouped) behind its size checks, in
// the order each makes them: y_dtype is float32 or x's type, centers, y where there is an output, the inputs where there is a
// product (`inputs_missing`, worded `inputs`: "x or labels", "x"), x and y aligned to their element size.  NNC_EINVAL or NNC_OK.
static inline int cb_check_operands(const char *fn, const void *x, int x_dtype, const void *y, int y_dtype, const void *centers, int64_t m, int64_t kdim,
                                    int64_t ncols, bool inputs_missing, const char *inputs)
{
    const std::string f(fn);
    if (y_dtype != NNC_DT_F32 && y_dtype != x_dtype) return fail(NNC_EINVAL, f + ": y_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers) return fail(NNC_EINVAL, f + ": centers is NULL");
    if (m > 0 && ncols > 0 && !y) return fail(NNC_EINVAL, f + ": y is NULL");
    if (m > 0 && ncols > 0 && kdim > 0 && inputs_missing) return fail(NNC_EINVAL, f + ": " + inputs + " is NULL");
    const int xb = x_dtype == NNC_DT_F32 ? 4 : 2, yb = y_dtype == NNC_DT_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(x) % xb || reinterpret_cast<uintptr_t>(y) % yb) return fail(NNC_EINVAL, f + ": x or y is not aligned to its element size");
    return NNC_OK;
}

// what the main kernel of such an entry point writes: y itself with one split (direct 1: float32, 2: x's type), else (0) the float32
// partials into the workspace, which cb_finish then sums into y (k_cbmm_reduce)
static inline int cb_direct(long long splits, int y_dtype) { return splits == 1 ? (y_dtype == NNC_DT_F32 ? 1 : 2) : 0; }
static inline int cb_finish(int direct, const void *workspace, long long splits, long long mn, long long ncols, const float *bias, int relu, void *y,
                            int y_dtype, hipStream_t s)
{
    return direct ? NNC_OK : cbmm_reduce_dt(reinterpret_cast<const float *>(workspace), splits, mn, ncols, bias, relu, y, y_dtype, s);
}

// G as the group-wise layers count it: centers and dc have a row even where kdim = 0
static inline long long gg_groups(long long kdim, long long group_rows) { return std::max(1LL, cdiv(kdim, group_rows)); }

// The group_rows checks of every group-wise entry point `fn`, forward and backward, in the order each makes them: a multiple of
// 32 and at least 32; at most 2^40; and, where the caller keeps bins (bins_k = its k > 0: the dc sums of the backward units), at
// most 2^30 of them.  NNC_EINVAL or NNC_OK.
static inline int cb_check_group_rows(const char *fn, int64_t kdim, int64_t group_rows, int32_t bins_k = 0)
{
    const std::string f(fn);
    if (group_rows < 32 || group_rows % 32) return fail(NNC_EINVAL, f + ": group_rows must be a positive multiple of 32");
    if (group_rows > (1LL << 40)) return fail(NNC_EINVAL, f + ": size too large");
    if (bins_k > 0 && gg_groups(kdim, group_rows) * bins_k > (1LL << 30)) return fail(NNC_EINVAL, f + ": more than 2^30 bins (groups * k)");
    return NNC_OK;
}

// the most groups of group_rows rows that the rows of one split lie in (the group-wise units report it in their plans)
static inline long long max_groups_per_split(long long splits, long long rows_per_split, long long kdim, long long group_rows)
{
    long long most = 0;
    for (long long s = 0; s < splits; ++s) {
        const long long lo = s * rows_per_split, hi = std::min(kdim, lo + rows_per_split);
        most = std::max(most, (hi - 1) / group_rows - lo / group_rows + 1);
    }
    return most;
}

// the per-bank table: entry j of lane l at word j * copies + (l mod copies), copies = 1 << cshift
template <typename LT> struct CbTable;
template <> struct CbTable<uint8_t> {
    __device__ static __forceinline__ int index(uint32_t l, int, int cshift, int lane) { return (int)((l << cshift) | (lane & ((1 << cshift) - 1))); }
};
template <> struct CbTable<uint16_t> {
    __device__ static __forceinline__ int index(uint32_t l, int k, int cshift, int lane)
    {
        return (int)((std::min(l, (uint32_t)k) << cshift) | (lane & ((1 << cshift) - 1)));   // entry k holds the out-of-range value
    }
};

// one TB_K step of the 128 x 128 tile: thread (tx, ty) adds xs[kk][ty*8 + a] * ws[kk][tx*8 + b] into acc[a][b], kk in order
__device__ __forceinline__ void tb_tile_fma(const float *xs, const float *ws, int tx, int ty, float (&acc)[8][8])
{
#pragma unroll
    for (int kk = 0; kk < TB_K; ++kk) {
        const float4 a0 = *reinterpret_cast<const float4 *>(xs + kk * TB_M + ty * 8);
        const float4 a1 = *reinterpret_cast<const float4 *>(xs + kk * TB_M + ty * 8 + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(ws + kk * TB_N + tx * 8);
        const float4 b1 = *reinterpret_cast<const float4 *>(ws + kk * TB_N + tx * 8 + 4);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = __builtin_fmaf(av[a], bv[b], acc[a][b]);
    }
}

// ------------------------------------------------------------------ device helpers
// the table: `entries` values (centers, then zeros), `1 << cshift` copies of each, copy c of entry j at j * copies + c.  The
// centres come from global memory once per workgroup into `stage`; the copies are made from LDS (a loop of global loads per copy
// was a chain of L2 round trips in front of every workgroup).
// RT = bf16_t / f16_t: every centre rounded to RT (to nearest even, as torch's .to(dtype)) and widened back.
template <typename RT = float>
__device__ __forceinline__ void cb_fill(float *cb, float *stage, const float *__restrict__ centers, int k, int entries, int cshift)
{
    for (int j = threadIdx.x; j < entries; j += blockDim.x) stage[j] = j < k ? (float)(RT)centers[j] : 0.0f;
    __syncthreads();
    const int words = entries << cshift;
#pragma unroll 8
    for (int w = threadIdx.x; w < words; w += blockDim.x) cb[w] = stage[w >> cshift];
}

// the grouped layers (nnc_cbmm_grouped.hip) change tables on the way through a split: the copies of the first k entries
// rewritten from another group's centres (the zeros behind them stay).  The caller's barriers keep readers of the old table out.
template <typename RT = float>
__device__ __forceinline__ void cb_refill(float *cb, const float *__restrict__ centers, int k, int cshift)
{
    const int words = k << cshift;
#pragma unroll 8
    for (int w = threadIdx.x; w < words; w += blockDim.x) cb[w] = (float)(RT)centers[w >> cshift];
}

template <int VB> struct Chunk;
template <> struct Chunk<4> { using T = uint32_t; };
template <> struct Chunk<8> { using T = uint2; };
template <> struct Chunk<16> { using T = uint4; };

template <int VB>
__device__ __forceinline__ void load_chunk(const unsigned char *p, uint32_t *w)
{
    const typename Chunk<VB>::T v = *reinterpret_cast<const typename Chunk<VB>::T *>(p);
    __builtin_memcpy(w, &v, VB);
}

// o[d] = bytes [s + 4d, s + 4d + 4) of the 2N-dword window w (s < 4N, uniform over the wave)
template <int N>
__device__ __forceinline__ void funnel(const uint32_t *w, uint32_t s, uint32_t *o)
{
    const uint32_t q = s >> 2, r = s & 3;
    uint32_t v[N + 1];
#pragma unroll
    for (int d = 0; d <= N; ++d) {
        uint32_t t = w[d];
#pragma unroll
        for (int qq = 1; qq < N; ++qq) t = q == (uint32_t)qq ? w[d + qq] : t;
        v[d] = t;
    }
#pragma unroll
    for (int d = 0; d < N; ++d) o[d] = __builtin_amdgcn_alignbyte(v[d + 1], v[d], r);
}

// The label row loads of the byte-form stream kernels, forward and backward: the lane's VB bytes of label
// row i into w (s = 0) where every row starts on a VB-byte boundary; else the two aligned chunks that hold them into the 2N-dword
// window w, and the byte offset s of the lane's bytes in it (uniform over the wave: funnel() shifts by it).  `base` the labels,
// `lane_off` the byte offset of the lane's window in its row; a lane past the row (`active` false) reads the row's first chunk.
template <int VB, bool ALIGNED>
__device__ __forceinline__ void cb_row_words(uintptr_t base, long long row_bytes, long long lane_off, bool active, long long i, uint32_t *w, uint32_t &s)
{
    constexpr int N = VB / 4;
    const uintptr_t row = base + (uintptr_t)(i * row_bytes);
    if constexpr (ALIGNED) {
        s = 0;
        load_chunk<VB>(reinterpret_cast<const unsigned char *>(active ? row + lane_off : row), w);
    } else {
        const uintptr_t first = row & ~(uintptr_t)(VB - 1);          // the chunk that holds the row's first byte
        s = (uint32_t)(__builtin_amdgcn_readfirstlane((uint32_t)((row + blockIdx.x * (64 * VB)) & (VB - 1))));
        const uintptr_t a = ((row + lane_off) & ~(uintptr_t)(VB - 1));
        const uintptr_t a0 = active ? a : first;
        const uintptr_t a1 = (active && a + VB < row + row_bytes) ? a + VB : a0;
        load_chunk<VB>(reinterpret_cast<const unsigned char *>(a0), w);
        load_chunk<VB>(reinterpret_cast<const unsigned char *>(a1), w + N);
    }
}

// x[r, i + u] of a batch of U rows of a forward stream kernel: lane f holds value f = r * U + u (and f + 64), broadcast later by
// v_readlane.  Vector loads keep the x reads off the LGKM counter that every LDS lookup waits on.  The second value exists only
// where a batch holds more than 64 (MT * CB_UNROLL > 64: MT = 16 at U = CB_UNROLL).  A shorter batch of an MT = 16 kernel (U = 1, or
// the U = 4 of the packed kernels) passes that guard too and still loads nothing: its row r1 = (lane + 64) / U >= 16 >= m, m <= 16
// on every stream path.
template <int MT, typename XT>
__device__ __forceinline__ void cb_load_x(const XT *__restrict__ x, long long kdim, int m, int lane, long long i, int U, float &xa, float &xb)
{
    const int f0 = lane, f1 = lane + 64;
    const int r0 = f0 / U, r1 = f1 / U;
    xa = r0 < m ? (float)x[(long long)r0 * kdim + i + f0 % U] : 0.0f;
    xb = (MT * CB_UNROLL > 64 && r1 < m) ? (float)x[(long long)r1 * kdim + i + f1 % U] : 0.0f;
}

// The step of a group-wise stream kernel that walks its workgroup's rows [.., s_hi) group by group: the rows from g_lo on that
// lie in `group` end at g_hi (the group's end or the workgroup's), and wave `wave` takes [i0, i1) of them, divided among the
// CB_WAVES waves as an ungrouped kernel divides its whole range.
__device__ __forceinline__ void cb_group_step(long long group, long long group_rows, long long g_lo, long long s_hi, int wave, long long &g_hi, long long &i0,
                                              long long &i1)
{
    g_hi = std::min(s_hi, (group + 1) * group_rows);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
}

// ------------------------------------------------------------------ skinny: m <= 16
// grid (col_tiles, splits), CB_THREADS threads.  `out` is y (direct != 0: + bias, ReLU here) or the float32 partials
// [split][m][ncols].  XT = float is nnc_cbmm_f32's kernel (nnc_cbmm.hip).  XT = bf16_t / f16_t is nnc_cbmm_h16's (nnc_cbmm_h16.hip):
// x is read as XT and widened (exact), the table holds the centres rounded to XT and widened, the arithmetic is the same float32
// fmaf chain, and direct = 2 stores y as XT (one rounding) where direct = 1 stores float32.
template <typename XT, typename LT, int VB, int MT, bool ALIGNED>
__global__ __launch_bounds__(CB_THREADS) void k_cbmm_stream(const XT *__restrict__ x, int m, long long kdim, const unsigned char *__restrict__ labels,
                                                            long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                            long long rows_per_split, const float *__restrict__ bias, int relu, int direct,
                                                            void *__restrict__ out_)
{
    constexpr int LB = sizeof(LT), E = VB / LB, N = VB / 4, PER = 32 / (8 * LB) /* labels per dword */;
    extern __shared__ float smem[];
    float *cb = smem;
    float *red = smem + (entries << cshift);
    float *stage = red + MT * E * 64;
    float *out = reinterpret_cast<float *>(out_);
    cb_fill<XT>(cb, stage, centers, k, entries, cshift);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    const long long per_wave = (s_hi - s_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(s_hi, s_lo + wave * per_wave), i1 = std::min(s_hi, i0 + per_wave);
    const uintptr_t base = reinterpret_cast<uintptr_t>(labels);
    const long long row_bytes = ncols * LB;
    const long long lane_off = (long long)blockIdx.x * (64 * VB) + lane * VB;   // byte offset of the lane's window in its row

    float acc[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[r][e] = 0.0f;
    __syncthreads();

    auto row_words = [&](long long i, uint32_t *w, uint32_t &s) { cb_row_words<VB, ALIGNED>(base, row_bytes, lane_off, active, i, w, s); };
    auto load_x = [&](long long i, int U, float &xa, float &xb) { cb_load_x<MT>(x, kdim, m, lane, i, U, xa, xb); };
    auto consume = [&](const uint32_t *w, uint32_t s, float xa, float xb, int u, int U) {
        float xv[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            const int f = r * U + u;
            xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
        }
        uint32_t o[N];
        if constexpr (ALIGNED) {
#pragma unroll
            for (int d = 0; d < N; ++d) o[d] = w[d];
        } else {
            funnel<N>(w, s, o);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t l = (o[e / PER] >> (8 * LB * (e % PER))) & (LB == 1 ? 0xFFu : 0xFFFFu);
            const float wv = cb[CbTable<LT>::index(l, k, cshift, lane)];
#pragma unroll
            for (int r = 0; r < MT; ++r) acc[r][e] = __builtin_fmaf(xv[r], wv, acc[r][e]);
        }
    };

    constexpr int WN = ALIGNED ? N : 2 * N;
    long long i = i0;
    for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
        uint32_t w[CB_UNROLL][WN], s[CB_UNROLL];
        float xa, xb;
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) row_words(i + u, w[u], s[u]);
        load_x(i, CB_UNROLL, xa, xb);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], s[u], xa, xb, u, CB_UNROLL);
    }
    for (; i < i1; ++i) {
        uint32_t w[WN], s;
        float xa, xb;
        row_words(i, w, s);
        load_x(i, 1, xa, xb);
        consume(w, s, xa, xb, 0, 1);
    }

    // the waves' sums, added to wave 0's in wave order
    for (int src = 1; src < CB_WAVES; ++src) {
        __syncthreads();
        if (wave == src) {
#pragma unroll
            for (int r = 0; r < MT; ++r)
#pragma unroll
                for (int e = 0; e < E; ++e) red[(r * E + e) * 64 + lane] = acc[r][e];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < MT; ++r)
#pragma unroll
                for (int e = 0; e < E; ++e) acc[r][e] += red[(r * E + e) * 64 + lane];
        }
    }
    if (wave != 0 || !active) return;
#pragma unroll
    for (int r = 0; r < MT; ++r) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const long long c = c0 + e;
            if (r >= m || c >= ncols) continue;
            float v = acc[r][e];
            if (direct) {
                if (bias) v += bias[c];
                if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
                if (!std::is_same<XT, float>::value && direct == 2)
                    reinterpret_cast<XT *>(out_)[(long long)r * ncols + c] = (XT)v;
                else
                    out[(long long)r * ncols + c] = v;
            } else {
                out[((long long)blockIdx.y * m + r) * ncols + c] = v;
            }
        }
    }
}
