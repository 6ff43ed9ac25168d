// nnc_cbgrad.hpp -- what the five backward units of the codebook matmul share (nnc_cbgrad.hip, nnc_cbgrad_grouped.hip,
// nnc_cbspgrad.hip, nnc_cbpkgrad.hip, nnc_cbpkgrad_grouped.hip).  Device side: the fixed-order wave
// reduction of the dx stream kernels, the scaling and fixed-point binning of dc and the x load of the dc
// stream kernels (cbdc_load_x).  Host side: the plans of the byte form (CgPlan, dx_plan, dc_plan) and its argument checks
// (cg_check), which the group-wise unit follows too; the list of the uint8 and uint16 stream instantiations; and the glue every
// backward entry point runs, written once: the lookup in a unit's table of stream instantiations and its error (cbg_stream_case),
// the checks of a plan call (cbg_plan_out), the tail of a grouped plan record (cbg_grouped_plan_tail) and the two sequences of
// HIP calls (cbg_run_dx, cbg_run_dc), which take the unit's own launch as a callable.  The kernels both directions of every unit
// launch (k_cbgrad_absmax, k_cbgrad_reduce, k_cbdc_finish) are launched by nnc_cbgrad.hip; the first two and the byte form's two
// stream kernels are templates here, on the element type: float32, or the bf16 / fp16 of nnc_cbgrad_h16.hip (DESIGN.md section
// 22).  The tiled kernels' shared text is in nnc_cbtile.hpp, the label row loads and the group step of the stream kernels in
// nnc_cbmm.hpp.
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

// x[r, i + u] of a batch of U rows of a dc stream kernel, scaled by 2^scx: lane f holds value f = r * U + u (and f + 64),
// broadcast later by v_readlane (as k_cbmm_stream's cb_load_x); a bf16 / fp16 x is widened first
template <int MT, typename XT>
__device__ __forceinline__ void cbdc_load_x(const XT *__restrict__ x, long long kdim, int m, int scx, int lane, long long i, int U, float &xa, float &xb)
{
    const int f0 = lane, f1 = lane + 64;
    const int r0 = f0 / U, r1 = f1 / U;
    xa = cbdc_scaled((float)x[cbdc_idx((long long)r0 * kdim + i + f0 % U, r0 < m)], r0 < m, scx);
    xb = MT * CB_UNROLL > 64 ? cbdc_scaled((float)x[cbdc_idx((long long)r1 * kdim + i + f1 % U, r1 < m)], r1 < m, scx) : 0.0f;
}

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

// ------------------------------------------------------------------ the stream kernels of the byte form and the kernels around them
// Templated on the element type of x and g (k_cbgrad_reduce: of its output): nnc_cbgrad.hip instantiates them for float32,
// nnc_cbgrad_h16.hip for bf16 / fp16.
// ------------------------------------------------------------------ max |x|, max |g|
// amax[0] = bits of max |x|, amax[1] = bits of max |g| (zeroed by the caller).  |v| as a bit pattern orders as the value; a NaN
// orders above Inf, so amax >= 0x7F800000 means "not finite".  XT = bf16_t / f16_t (nnc_cbgrad_h16.hip): the bits of the widened value.
template <typename XT>
__global__ __launch_bounds__(256) void k_cbgrad_absmax(const XT *__restrict__ x, long long nx, const XT *__restrict__ g, long long ng,
                                                       uint32_t *__restrict__ amax)
{
    __shared__ uint32_t wmax[2][4];
    uint32_t a = 0, b = 0;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < nx; i += nth) a = std::max(a, __float_as_uint((float)x[i]) & 0x7FFFFFFFu);
    for (long long i = tid; i < ng; i += nth) b = std::max(b, __float_as_uint((float)g[i]) & 0x7FFFFFFFu);
#pragma unroll
    for (int bit = 32; bit >= 1; bit >>= 1) {
        a = std::max(a, (uint32_t)__shfl_xor((int)a, bit));
        b = std::max(b, (uint32_t)__shfl_xor((int)b, bit));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        wmax[0][wave] = a;
        wmax[1][wave] = b;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t v = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) v = std::max(v, wmax[threadIdx.x][w]);
        if (v) atomicMax(&amax[threadIdx.x], v);
    }
}

// ------------------------------------------------------------------ dx, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  out: dx (one column block; direct 1: float32, 2: XT) or the float32 partials
// [block][m][kdim].  XT = float is nnc_cbmm_dx_f32's kernel; XT = bf16_t / f16_t nnc_cbmm_dx_h16's: g is read as XT and widened, the
// table holds the centres rounded to XT and widened, the arithmetic is the same float32 fmaf chain.
template <typename XT, typename LT, int VB, int MT, bool ALIGNED>
__global__ __launch_bounds__(CB_THREADS) void k_cbdx_stream(const XT *__restrict__ g, int m, long long kdim, const unsigned char *__restrict__ labels,
                                                            long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                            long long rows_per_group, int direct, void *__restrict__ out_)
{
    constexpr int LB = sizeof(LT), E = VB / LB, N = VB / 4, PER = 32 / (8 * LB);
    extern __shared__ float smem[];
    float *cb = smem;
    float *stage = smem + (entries << cshift);
    float *out = reinterpret_cast<float *>(out_);
    cb_fill<XT>(cb, stage, centers, k, entries, cshift);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));   // the lane's columns inside the matrix
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (r < m && e < ne) ? (float)g[(long long)r * ncols + c0 + e] : 0.0f;

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const uintptr_t base = reinterpret_cast<uintptr_t>(labels);
    const long long row_bytes = ncols * LB;
    const long long lane_off = (long long)blockIdx.x * (64 * VB) + lane * VB;
    float *dst = direct ? out : out + (long long)blockIdx.x * m * kdim;
    __syncthreads();

    auto row_words = [&](long long i, uint32_t *w, uint32_t &s) { cb_row_words<VB, ALIGNED>(base, row_bytes, lane_off, active, i, w, s); };
    auto consume = [&](const uint32_t *w, uint32_t s, long long i) {
        uint32_t o[N];
        if constexpr (ALIGNED) {
#pragma unroll
            for (int d = 0; d < N; ++d) o[d] = w[d];
        } else {
            funnel<N>(w, s, o);
        }
        float p[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) p[r] = 0.0f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t l = (o[e / PER] >> (8 * LB * (e % PER))) & (LB == 1 ? 0xFFu : 0xFFFFu);
            const float wv = e < ne ? cb[CbTable<LT>::index(l, k, cshift, lane)] : 0.0f;   // (columns past the row: no Inf * 0)
#pragma unroll
            for (int r = 0; r < MT; ++r) p[r] = __builtin_fmaf(gv[r][e], wv, p[r]);
        }
        int row;
        const float v = wave_reduce_rows<MT>(p, lane, row);
        if ((lane & (64 / MT - 1)) == 0 && row < m) {
            if (!std::is_same<XT, float>::value && direct == 2)
                reinterpret_cast<XT *>(out_)[(long long)row * kdim + i] = (XT)v;
            else
                dst[(long long)row * kdim + i] = v;
        }
    };

    constexpr int WN = ALIGNED ? N : 2 * N;
    long long i = i0;
    for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
        uint32_t w[CB_UNROLL][WN], s[CB_UNROLL];
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) row_words(i + u, w[u], s[u]);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], s[u], i + u);
    }
    for (; i < i1; ++i) {
        uint32_t w[WN], s;
        row_words(i, w, s);
        consume(w, s, i);
    }
}

// ------------------------------------------------------------------ the split partials, summed in split order
// (OT = float, or bf16_t / f16_t: the float32 sum rounded once to nearest even)
template <typename OT>
__global__ __launch_bounds__(256) void k_cbgrad_reduce(const float *__restrict__ part, long long splits, long long mn, OT *__restrict__ out)
{
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < mn; idx += (long long)gridDim.x * blockDim.x) {
        float v = part[idx];
        for (long long s = 1; s < splits; ++s) v += part[s * mn + idx];
        out[idx] = (OT)v;
    }
}

// ------------------------------------------------------------------ dc, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  LDS: the bins, [k][1 << rlog2] int64.  XT = bf16_t / f16_t
// (nnc_cbmm_dc_h16): x and g are widened as they are loaded; the rest is the float32 kernel.
template <typename XT, typename LT, int VB, int MT, bool ALIGNED>
__global__ __launch_bounds__(CB_THREADS) void k_cbdc_stream(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
                                                            const unsigned char *__restrict__ labels, long long ncols, int k, int rlog2, int terms_log2,
                                                            long long rows_per_group, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    constexpr int LB = sizeof(LT), E = VB / LB, N = VB / 4, PER = 32 / (8 * LB);
    extern __shared__ unsigned long long bins[];
    int flag;
    const int S = cbdc_shift(hdr, m, terms_log2, flag);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        hdr[2] = (uint32_t)S;
        hdr[3] = (uint32_t)flag;
    }
    if (flag != CBG_FLAG_OK) return;   // (uniform over the launch)
    int scx, scg;
    cbdc_scales(hdr, scx, scg);
    const int Sw = S - scx - scg;      // the shift of dW' = dW * 2^(scx + scg)
    for (int j = threadIdx.x; j < (k << rlog2); j += CB_THREADS) bins[j] = 0ull;

    const int lane = threadIdx.x & 63;
    const int rep = lane & ((1 << rlog2) - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (float)g[cbdc_idx((long long)r * ncols + c0 + e, r < m && e < ne)];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = cbdc_scaled(gv[r][e], r < m && e < ne, scg);

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const uintptr_t base = reinterpret_cast<uintptr_t>(labels);
    const long long row_bytes = ncols * LB;
    const long long lane_off = (long long)blockIdx.x * (64 * VB) + lane * VB;
    __syncthreads();

    auto row_words = [&](long long i, uint32_t *w, uint32_t &s) { cb_row_words<VB, ALIGNED>(base, row_bytes, lane_off, active, i, w, s); };
    auto load_x = [&](long long i, int U, float &xa, float &xb) { cbdc_load_x<MT>(x, kdim, m, scx, lane, i, U, xa, xb); };
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
            float d = 0.0f;
#pragma unroll
            for (int r = 0; r < MT; ++r) d = __builtin_fmaf(xv[r], gv[r][e], d);   // dW'[i, o], r ascending
            if (e < ne && l < (uint32_t)k) atomicAdd(&bins[(l << rlog2) + rep], cbdc_fix(d, Sw));
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
    cbdc_flush(bins, k, rlog2, sums);
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
        cb_table_shape(lb, k, p.entries, p.cshift);
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
// (gg_groups, the count of groups, and the group_rows checks are nnc_cbmm.hpp's)
static inline int tile_groups(long long group_rows) { return group_rows % 128 == 0 ? 1 : (group_rows == 32 ? 4 : 2); }

// the shared kernels, launched on `s` by nnc_cbgrad.hip (NNC_OK, or the launch error); dtype / out_dtype are NNC_DT_*:
//   cbgrad_absmax_dt  amax[0..1] = bits of max |x[0, nx)|, max |g[0, ng)| as float32 (amax zeroed by the caller)   k_cbgrad_absmax
//   cbgrad_reduce_dt  out[idx] = sum over s < splits of part[s * mn + idx], in split order, as out_dtype          k_cbgrad_reduce
//   cbdc_finish       dc[j] = ldexp(sums[j], -S), float64 or float32; NaN on CBG_FLAG_NONFINITE                    k_cbdc_finish
// cbgrad_absmax / cbgrad_reduce: the float32 calls of the five float32 units
int cbgrad_absmax_dt(const void *x, long long nx, const void *g, long long ng, int dtype, uint32_t *amax, hipStream_t s);
int cbgrad_reduce_dt(const float *part, long long splits, long long mn, void *out, int out_dtype, hipStream_t s);
int cbdc_finish(const uint32_t *hdr, const long long *sums, int k, int f64, void *out, hipStream_t s);
static inline int cbgrad_absmax(const float *x, long long nx, const float *g, long long ng, uint32_t *amax, hipStream_t s)
{
    return cbgrad_absmax_dt(x, nx, g, ng, NNC_DT_F32, amax, s);
}
static inline int cbgrad_reduce(const float *part, long long splits, long long mn, float *out, hipStream_t s)
{
    return cbgrad_reduce_dt(part, splits, mn, out, NNC_DT_F32, s);
}

// ------------------------------------------------------------------ the host glue of every backward entry point
// The (vb, mt) of the stream kernels the byte-form plans (cg_stream_grid) can ask for, per label width, written once: the tables
// of nnc_cbgrad.hip (both widths) and of nnc_cbgrad_grouped.hip (uint8) are made from these lists, so the grouped unit cannot miss
// a case the plan produces.  The packed list is PKG_STREAM_CASES (nnc_cbpkgrad.hpp).
#define CBG_U8_STREAM_CASES(X) X(16, 1) X(16, 2) X(16, 4) X(8, 8) X(4, 16)
#define CBG_U16_STREAM_CASES(X) X(16, 1) X(16, 2) X(16, 4) X(16, 8) X(8, 16)

// How a unit words a missing stream instantiation: "<fn>: no [grouped ]stream instantiation for [<first> a, ][vb v, ]mt m".  Its
// table entries begin with the three ints {a, vb, mt}: a = label_bytes or bits (0 where `first` is NULL), vb = 0 without `vb`.
struct CbgCaseNames {
    bool grouped;
    const char *first;
    bool vb;
};

// The stream instantiation a plan asks for: c = the entry {a, vb, mt} of `cases` where the path is NNC_CBMM_STREAM (NNC_EINVAL
// and the unit's message if the table has none), NULL on every other path.
template <typename Case, size_t N>
static int cbg_stream_case(const char *fn, const Case (&cases)[N], const CbgCaseNames &n, int path, int a, int vb, int mt, const Case *&c)
{
    c = nullptr;
    if (path != NNC_CBMM_STREAM) return NNC_OK;
    for (const Case &e : cases)
        if (e.a == a && e.vb == vb && e.mt == mt) c = &e;
    if (c) return NNC_OK;
    return fail(NNC_EINVAL, std::string(fn) + ": no " + (n.grouped ? "grouped " : "") + "stream instantiation for " +
                                (n.first ? n.first + (" " + std::to_string(a)) + ", " : std::string()) + (n.vb ? "vb " + std::to_string(vb) + ", " : std::string()) +
                                "mt " + std::to_string(mt));
}

// the checks of a plan call behind its plan: cus, out, then the stream instantiation
template <typename Case, size_t N>
static int cbg_plan_out(const char *fn, const Case (&cases)[N], const CbgCaseNames &n, int path, int a, int vb, int mt, int32_t cus, const int64_t *out)
{
    if (cus < 1) return fail(NNC_EINVAL, std::string(fn) + ": cus < 1");
    if (!out) return fail(NNC_EINVAL, std::string(fn) + ": out is NULL");
    const Case *c;
    return cbg_stream_case(fn, cases, n, path, a, vb, mt, c);
}

// the four values a grouped plan adds to the ungrouped record (the packed one adds a fifth of its own behind them)
static inline void cbg_grouped_plan_tail(int path, long long row_tiles, long long rows_per_group, long long kdim, long long group_rows, int64_t *out)
{
    const bool stream = path == NNC_CBMM_STREAM, tiled = path == NNC_CBMM_TILED;
    out[0] = group_rows;
    out[1] = kdim > 0 ? cdiv(kdim, group_rows) : 0;
    out[2] = stream ? rows_per_group : 0;
    out[3] = stream ? max_groups_per_split(row_tiles, rows_per_group, kdim, group_rows)
                    : (tiled ? max_groups_per_split(cdiv(kdim, 128), 128, kdim, group_rows) : 0);
}

// What every dx entry point does on the stream behind its checks and its plan: nothing (NNC_CBMM_NONE); dx = 0 (NNC_CBMM_ZERO); else
// the unit's stream or tiled kernel -- launch(direct, out) launches it and returns its status -- into dx itself with one split
// (direct 1: float32, 2: dx_dtype), or (direct 0) into the float32 partials at the head of the workspace, which k_cbgrad_reduce
// then sums into dx in split order.  dx_dtype is NNC_DT_F32 in the float32 units (the second form), or the half type of
// nnc_cbmm_dx_h16.
template <typename Launch>
static int cbg_run_dx(int path, long long splits, long long m, long long kdim, void *dx, int dx_dtype, void *workspace, hipStream_t s, Launch launch)
{
    if (path == NNC_CBMM_NONE) return NNC_OK;
    if (path == NNC_CBMM_ZERO) {
        HIPCHK(hipMemsetAsync(dx, 0, (size_t)(m * kdim) * (dx_dtype == NNC_DT_F32 ? 4 : 2), s));
        return NNC_OK;
    }
    const int direct = splits == 1 ? (dx_dtype == NNC_DT_F32 ? 1 : 2) : 0;
    const int rc = launch(direct, direct ? dx : workspace);
    if (rc != NNC_OK) return rc;
    if (!direct) return cbgrad_reduce_dt(reinterpret_cast<const float *>(workspace), splits, m * kdim, dx, dx_dtype, s);
    return NNC_OK;
}

template <typename Launch>
static int cbg_run_dx(int path, long long splits, long long m, long long kdim, float *dx, void *workspace, hipStream_t s, Launch launch)
{
    return cbg_run_dx(path, splits, m, kdim, dx, NNC_DT_F32, workspace, s, [&](int direct, void *out) { return launch(direct, reinterpret_cast<float *>(out)); });
}

// What every dc entry point does on the stream behind its checks and its plan: dc = 0 over the nbins bins (NNC_CBMM_ZERO); else the
// workspace (`need` bytes: the header, then int64 sums[nbins]) zeroed, k_cbgrad_absmax over x and g of x_dtype into the header, the
// unit's stream or tiled kernel -- launch(hdr, sums) launches it and returns its status -- and k_cbdc_finish from the sums into dc.
template <typename Launch>
static int cbg_run_dc(int path, const void *x, const void *g, int x_dtype, long long m, long long kdim, long long ncols, int nbins, void *dc, int out_f64,
                      void *workspace, int64_t need, hipStream_t s, Launch launch)
{
    if (path == NNC_CBMM_ZERO) {
        HIPCHK(hipMemsetAsync(dc, 0, (size_t)nbins * (out_f64 ? 8 : 4), s));
        return NNC_OK;
    }
    uint32_t *hdr = reinterpret_cast<uint32_t *>(workspace);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(workspace) + CBG_HDR_BYTES);
    HIPCHK(hipMemsetAsync(workspace, 0, (size_t)need, s));
    int rc = cbgrad_absmax_dt(x, m * kdim, g, m * ncols, x_dtype, hdr, s);
    if (rc != NNC_OK) return rc;
    if ((rc = launch(hdr, sums)) != NNC_OK) return rc;
    return cbdc_finish(hdr, reinterpret_cast<const long long *>(sums), nbins, (int)(out_f64 != 0), dc, s);
}

template <typename Launch>
static int cbg_run_dc(int path, const float *x, const float *g, long long m, long long kdim, long long ncols, int nbins, void *dc, int out_f64,
                      void *workspace, int64_t need, hipStream_t s, Launch launch)
{
    return cbg_run_dc(path, x, g, NNC_DT_F32, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, launch);
}
