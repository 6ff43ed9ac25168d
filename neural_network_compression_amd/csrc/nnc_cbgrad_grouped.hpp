// nnc_cbgrad_grouped.hpp -- what the two backward units of the group-wise byte form share (nnc_cbgrad_grouped.hip: float32;
// nnc_cbgrad_grouped_h16.hip: bf16 / fp16 activations): the two stream kernels (m <= 16), templated on the
// element type of g and x as the ungrouped ones of nnc_cbgrad.hpp are, and the argument checks both units make.  XT = float is
// nnc_cbmm_grouped_dx_f32's / nnc_cbmm_grouped_dc_f32's kernel, instruction for instruction what it was in nnc_cbgrad_grouped.hip;
// XT = bf16_t / f16_t reads g and x as XT and widens them, and the dx tables hold the centres rounded to XT and widened.  The fmaf
// chains, the walk through the groups and the barriers do not depend on XT.  Also here: which table or set of bins an index row of an
// MFMA tile uses (tile_group_of), for the MFMA kernels of both group-wise half units (the packed one too, section 27).
#pragma once
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ dx, m <= 16
// k_cbdx_stream<XT, uint8_t> with centers[groups][k]: grid (column blocks, row groups), CB_THREADS threads, the same `out` (direct
// 1: float32, 2: XT, 0: the float32 partials).
template <typename XT, int VB, int MT, bool ALIGNED>
__global__ __launch_bounds__(CB_THREADS) void k_cbdx_stream_grouped(const XT *__restrict__ g, int m, long long kdim, const unsigned char *__restrict__ labels,
                                                                    long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                                    long long rows_per_group, long long group_rows, int direct, void *__restrict__ out_)
{
    using LT = uint8_t;
    constexpr int LB = sizeof(LT), E = VB / LB, N = VB / 4, PER = 32 / (8 * LB);
    extern __shared__ float smem[];
    float *cb = smem;
    float *stage = smem + (entries << cshift);
    float *out = reinterpret_cast<float *>(out_);
    long long group = (long long)blockIdx.y * rows_per_group / group_rows;
    cb_fill<XT>(cb, stage, centers + group * k, k, entries, cshift);

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

    const long long s_lo = (long long)blockIdx.y * rows_per_group, s_hi = std::min(kdim, s_lo + rows_per_group);
    long long g_lo = s_lo, g_hi, i0, i1;   // the rows of the workgroup that lie in `group`, and the wave's share of them
    cb_group_step(group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
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
            const uint32_t l = (o[e / PER] >> (8 * LB * (e % PER))) & 0xFFu;
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
    for (;;) {
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
        if (g_hi >= s_hi) break;
        // on to the next group's rows, divided among the waves as the whole range is
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();   // every wave has left the rows of the group before
        cb_refill<XT>(cb, centers + group * k, k, cshift);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dc, m <= 16
// k_cbdc_stream<XT, uint8_t> with sums[groups][k]: grid (column blocks, row groups), CB_THREADS threads.  LDS: one group's bins,
// [k][1 << rlog2] int64.  The walk is k_cbdx_stream_grouped's; at a boundary the bins go into the group's sums and are cleared by
// the threads that have just read them, ahead of the barrier that opens the next stretch.
template <typename XT, int VB, int MT, bool ALIGNED>
__global__ __launch_bounds__(CB_THREADS) void k_cbdc_stream_grouped(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
                                                                    const unsigned char *__restrict__ labels, long long ncols, int k, int rlog2, int terms_log2,
                                                                    long long rows_per_group, long long group_rows, uint32_t *__restrict__ hdr,
                                                                    unsigned long long *__restrict__ sums)
{
    using LT = uint8_t;
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

    long long group = (long long)blockIdx.y * rows_per_group / group_rows;
    const long long s_lo = (long long)blockIdx.y * rows_per_group, s_hi = std::min(kdim, s_lo + rows_per_group);
    long long g_lo = s_lo, g_hi, i0, i1;   // the rows of the workgroup that lie in `group`, and the wave's share of them
    cb_group_step(group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
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
            const uint32_t l = (o[e / PER] >> (8 * LB * (e % PER))) & 0xFFu;
            float d = 0.0f;
#pragma unroll
            for (int r = 0; r < MT; ++r) d = __builtin_fmaf(xv[r], gv[r][e], d);   // dW'[i, o], r ascending
            if (e < ne && l < (uint32_t)k) atomicAdd(&bins[(l << rlog2) + rep], cbdc_fix(d, Sw));
        }
    };

    constexpr int WN = ALIGNED ? N : 2 * N;
    for (;;) {
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
        cbdc_flush(bins, k, rlog2, sums + group * k);   // (begins with a barrier: every wave has left the group's rows)
        if (g_hi >= s_hi) break;
        for (int j = threadIdx.x; j < k; j += CB_THREADS)   // the copies this thread has just summed
            for (int r = 0; r < (1 << rlog2); ++r) bins[(j << rlog2) + r] = 0ull;
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ the groups of an MFMA tile, m > 16 (both group-wise half units)
// The 128 index rows of a tile that starts at row i0 lie in the groups q0, q0 + 1, ... of the layer's `groups`; a kernel holds `held`
// (tile_groups: 1, 2 or 4) tables (dx) or sets of bins (dc) for them, one past the last group being unread.
struct TileGroups {
    long long q0, groups;
};

__device__ __forceinline__ TileGroups tile_groups_at(long long i0, long long kdim, long long group_rows)
{
    return {i0 / group_rows, (kdim + group_rows - 1) / group_rows};
}

// the table or set of index row i
__device__ __forceinline__ long long tile_group_of(const TileGroups &G, long long i, long long group_rows, int held)
{
    return std::min((long long)held - 1, i / group_rows - G.q0);
}

// dc: the first index row of the wave's quarter of the tile, T.m0 + T.wm, as a scalar.  The 32 rows of accumulator row a start at
// + 32 a and lie in one group (group_rows is a multiple of 32), so their set is a scalar too.
__device__ __forceinline__ long long tile_wave_row0(long long m0) { return m0 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 7) * 64; }

// ------------------------------------------------------------------ the checks of both units (host)
// cg_check's checks at label_bytes 1, then those nnc_cbmm_grouped makes of k and group_rows
static int gg_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (k > 256) return fail(NNC_EINVAL, std::string(fn) + ": k outside 1..256 (group codebooks take uint8 labels only)");
    const int rc = cg_check(fn, m, kdim, ncols, 1, k);
    if (rc != NNC_OK) return rc;
    return cb_check_group_rows(fn, kdim, group_rows, k);
}
