// nnc_cbpkgrad_grouped.hpp -- what the two backward units of the group-wise packed form share (nnc_cbpkgrad_grouped.hip: float32;
// nnc_cbpkgrad_grouped_h16.hip: bf16 / fp16 activations): the two stream kernels (m <= 16), templated on the
// element type of g and x as the ungrouped ones of nnc_cbpkgrad.hpp are, and the argument checks both units make.  XT = float is
// nnc_cbpk_grouped_dx_f32's / nnc_cbpk_grouped_dc_f32's kernel, instruction for instruction what it was in nnc_cbpkgrad_grouped.hip;
// XT = bf16_t / f16_t reads g and x as XT and widens them, and the dx tables hold the centres rounded to XT and widened.  The fmaf
// chains, the walk through the groups and the barriers do not depend on XT.
#pragma once
#include "nnc_cbpkgrad.hpp"

// ------------------------------------------------------------------ dx, m <= 16
// k_cbpkdx_stream<XT> with centers[groups][k]: grid (column blocks, row groups), CB_THREADS threads, the same `out`.  LDS: one table
// per wave, [CB_WAVES][2^BITS][PK_COPIES].  A wave's rows (the share k_cbpkdx_stream gives it) are walked in stretches cut at the
// group's end, each a run of batches of CB_UNROLL rows and then single rows: a row's sum does not depend on the batch it is in.
template <typename XT, int BITS, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbpkdx_stream_grouped(const XT *__restrict__ g, int m, long long kdim, const unsigned char *__restrict__ packed,
                                                                      long long row_bytes, long long ncols, const float *__restrict__ centers, int k,
                                                                      long long rows_per_group, long long group_rows, int direct, void *__restrict__ out_)
{
    constexpr int E = 8 * VB / BITS, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BITS, ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    static_assert(E * MT <= PKG_G, "g values per lane");
    extern __shared__ float smem[];
    float *out = reinterpret_cast<float *>(out_);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *cb = smem + wave * (ENTRIES * PK_COPIES);    // this wave's table: [ENTRIES][PK_COPIES]
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;                     // then the lane's VB bytes lie inside the padded row
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));   // the lane's columns inside the matrix
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (r < m && e < ne) ? (float)g[(long long)r * ncols + c0 + e] : 0.0f;

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const unsigned char *mine = packed + (active ? (long long)blockIdx.x * (64 * VB) + lane * VB : 0LL);
    const char *tab = reinterpret_cast<const char *>(cb) + ((lane & (PK_COPIES - 1)) << 2);
    float *dst = direct ? out : out + (long long)blockIdx.x * m * kdim;

    // lane j holds centre j of group q (rounded to XT and widened); 0 from k on
    auto centre = [&](long long q) {
        const float c = (float)(XT)centers[q * k + std::min(lane, k - 1)];
        return lane < k ? c : 0.0f;
    };
    // the wave's table from the centres its lanes hold: word t * 64 + lane is copy lane & 31 of entry 2 t + (lane >> 5)
    auto fill = [&](float cv) {
#pragma unroll
        for (int t = 0; t < ENTRIES / 2; ++t) {
            const int lo = __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv), 2 * t);
            const int hi = __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv), 2 * t + 1);
            cb[t * 64 + lane] = __builtin_bit_cast(float, lane < 32 ? lo : hi);
        }
        __builtin_amdgcn_wave_barrier();                // the lookups below read what other lanes of this wave wrote
    };
    auto consume = [&](const uint32_t *w, long long i) {
        float p[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) p[r] = 0.0f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            constexpr int SH = 7;                                        // entry l of this lane's copy at byte l << 7
            const int bit = BITS * (e % PER);
            const uint32_t d = w[e / PER];
            const uint32_t a = (bit >= SH ? d >> (bit - SH) : d << (SH - bit)) & (MASK << SH);
            const float wv = e < ne ? *reinterpret_cast<const float *>(tab + a) : 0.0f;   // (columns past the row: no Inf * 0)
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

    if (i0 >= i1) return;                               // uniform over the wave; the kernel has no workgroup barrier
    long long group = i0 / group_rows;
    float cv = centre(group);
    long long i = i0;
    for (;;) {
        const long long e1 = std::min(i1, (group + 1) * group_rows);   // the end of the stretch: the group's or the wave's
        fill(cv);                                       // the lookups of the stretch before were issued ahead of these writes
        if (e1 < i1) cv = centre(group + 1);            // the next group's centres arrive while this stretch runs
        for (; i + CB_UNROLL <= e1; i += CB_UNROLL) {
            uint32_t w[CB_UNROLL][N];
#pragma unroll
            for (int u = 0; u < CB_UNROLL; ++u) pk_load<VB>(mine + (i + u) * row_bytes, w[u]);
#pragma unroll
            for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], i + u);
        }
        for (; i < e1; ++i) {
            uint32_t w[N];
            pk_load<VB>(mine + i * row_bytes, w);
            consume(w, i);
        }
        if (e1 >= i1) break;
        ++group;
        __builtin_amdgcn_wave_barrier();                // the stretch's lookups stay ahead of the next fill
    }
}

// ------------------------------------------------------------------ dc, m <= 16
// k_cbpkdc_stream<XT> with sums[groups][k]: grid (column blocks, row groups), CB_THREADS threads.  LDS: one group's bins, [k][64]
// int64, copy `lane` of every bin this lane's own.  The workgroup's rows are walked group by group as k_cbdc_stream_grouped walks
// them: each stretch is divided among the four waves; at a boundary the bins go into the group's sums and are cleared by the
// threads that have just read them, ahead of the barrier that opens the next stretch.  Every wave reaches every barrier.
template <typename XT, int BITS, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbpkdc_stream_grouped(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
                                                                      const unsigned char *__restrict__ packed, long long row_bytes, long long ncols, int k,
                                                                      int terms_log2, long long rows_per_group, long long group_rows,
                                                                      uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    constexpr int E = 8 * VB / BITS, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    static_assert(E * MT <= PKG_G, "g values per lane");
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
    for (int j = threadIdx.x; j < (k << PKG_RLOG2); j += CB_THREADS) bins[j] = 0ull;

    const int lane = threadIdx.x & 63;
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
    const unsigned char *mine = packed + (active ? (long long)blockIdx.x * (64 * VB) + lane * VB : 0LL);
    unsigned long long *mybins = bins + lane;
    __syncthreads();

    auto load_x = [&](long long i, int U, float &xa, float &xb) { cbdc_load_x<MT>(x, kdim, m, scx, lane, i, U, xa, xb); };
    auto consume = [&](const uint32_t *w, float xa, float xb, int u, int U) {
        float xv[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            const int f = r * U + u;
            xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t l = (w[e / PER] >> (BITS * (e % PER))) & MASK;
            float d = 0.0f;
#pragma unroll
            for (int r = 0; r < MT; ++r) d = __builtin_fmaf(xv[r], gv[r][e], d);   // dW'[i, o], r ascending
            if (e < ne && l < (uint32_t)k) atomicAdd(&mybins[l << PKG_RLOG2], cbdc_fix(d, Sw));
        }
    };

    for (;;) {
        long long i = i0;
        for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
            uint32_t w[CB_UNROLL][N];
            float xa, xb;
#pragma unroll
            for (int u = 0; u < CB_UNROLL; ++u) pk_load<VB>(mine + (i + u) * row_bytes, w[u]);
            load_x(i, CB_UNROLL, xa, xb);
#pragma unroll
            for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], xa, xb, u, CB_UNROLL);
        }
        for (; i < i1; ++i) {
            uint32_t w[N];
            float xa, xb;
            pk_load<VB>(mine + i * row_bytes, w);
            load_x(i, 1, xa, xb);
            consume(w, xa, xb, 0, 1);
        }
        cbdc_flush(bins, k, PKG_RLOG2, sums + group * k);   // (begins with a barrier: every wave has left the group's rows)
        if (g_hi >= s_hi) break;                            // (s_hi and g_hi are the workgroup's: uniform)
        for (int j = threadIdx.x; j < k; j += CB_THREADS)   // the copies this thread has just summed
            for (int r = 0; r < (1 << PKG_RLOG2); ++r) bins[(j << PKG_RLOG2) + r] = 0ull;
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ the checks of both units (host)
// pg_check's checks, then those nnc_cbpk_grouped makes of group_rows and the bound on the G * k bins
static int pgg_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows)
{
    const int rc = pg_check(fn, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    return cb_check_group_rows(fn, kdim, group_rows, k);
}

