// nnc_cbwpgrad_grouped.hip -- the backward pass of the group-wise codebook matmul on 5- and 6-bit split-plane ("wide packed") indices
// (nnc_cbwp_grouped.hip) from the (G, K) codebooks and the buffer nnc_cbwp_pack wrote for the whole index matrix: the indices are never
// unpacked, W and dW never built (include/nnc_cbwpgrad_grouped.h, nnc_cbwp_grouped_dx / nnc_cbwp_grouped_dc).
// W[i, o] = c[i / group_rows][label (i, o)] (a label >= K reads 0), y = x @ W, g = dL/dy:
//
//   dx[r, i]  = sum_o g[r, o] * c[i / group_rows][label (i, o)]   a column past ncols forms no product
//   dc[q, j]  = sum_{(i, o): i / group_rows = q, label (i, o) = j} sum_r x[r, i] * g[r, o]   G x K bins; a padding field falls into none
//
// One fact shapes the six kernels.  Index row i produces column i of dx, so in dx the codebook changes along the output axis: a
// thread or a wave that owns an index row owns one table.  In dc it changes along the rows of dW: a set of bins per group.  (In the
// forward pass it changes along the reduction axis, which is why nnc_cbwp_grouped.hip's walks look different.)
// The plans are the ungrouped ones (wg_dx_plan, wg_dc_plan of nnc_cbwpgrad.hpp), so the path, the grids, the splits, the order of
// every sum and the shift S of the dc sums are those of nnc_cbwp_dx / nnc_cbwp_dc on the same shape; the dc ones are in turn the
// byte form's at label_bytes 1, which the group-wise byte form follows too.  All kernels are templated on <BASE, PLANES> = <4, 1>
// (5 bits) and <4, 2> (6 bits); the decode is section 37's (wp_move, wp_plane_load, wg_label: whole aligned words of the base part
// and of every plane).
//   k_cbwpdx_stream_grouped  m <= 16.  k_cbwpdx_stream's geometry and decode.  Every wave owns a table (2^bits entries x 32 per-bank
//                            copies: 4 or 8 KiB), walks its own index rows in stretches cut at the group's end and rewrites the
//                            table from the centres its lanes hold, loaded while the stretch before ran: no workgroup barrier, no
//                            staging row.  Row i of dx is k_cbwpdx_stream's with the table of i's group.
//   k_cbwpdx_tiled_grouped   m > 16, float32.  k_cbwpdx_tiled with the tables (2^bits entries, zeros from k on) of the up to four
//                            groups the 128 index rows of a tile lie in; a thread decodes one index row throughout and keeps a
//                            pointer to that row's table.
//   k_cbwpdx_mfma_grouped    m > 16, bf16 / fp16.  k_cbwpdx_mfma's loads (8 bytes of the base part and 2 of every plane a step) with
//                            k_cbdx_mfma_grouped's tables: the 32 per-bank copies of the ungrouped table are divided over the 1, 2 or 4
//                            tables of the tile's groups, so the LDS is the ungrouped kernel's.
//   k_cbwpdc_stream_grouped  m <= 16.  k_cbwpdc_stream's loop with the workgroup walk of k_cbdc_stream_grouped: the bins are one
//                            group's, flushed into sums + q * K and cleared at every boundary.
//   k_cbwpdc_tiled_grouped   m > 16, float32.  k_cbwpdc_tiled with the 1 << rlog2 copies of a bin cut into per-group sets: a thread's
//                            8 index rows lie in one group; one binning pass, one flush per set.
//   k_cbwpdc_mfma_grouped    m > 16, bf16 / fp16.  dcm_accumulate, then k_cbwpdc_mfma's epilogue into the set of the accumulator's
//                            32 rows (one group: group_rows is a multiple of 32, so the set is a scalar).
// The integer sums are exact, so neither walk changes a bit of dc; which wave takes a row changes no bit of dx.  Everything that
// steers a walk comes from blockIdx, the kernel arguments and the readfirstlane'd wave number: every wave of a workgroup reaches
// every barrier, and no cross-lane read sits in a lane-dependent branch.
// k_cbgrad_absmax, k_cbgrad_reduce and k_cbdc_finish (over G * K bins) are nnc_cbgrad.hip's; the sequences of HIP calls are
// cbg_run_dx / cbg_run_dc.  No load leaves the packed buffer.  No float atomics; no host read.
#include "nnc_cbwpgrad.hpp"
#include "nnc_cbgrad_grouped.hpp"
#include "nnc_cbgrad_h16.hpp"
#include "nnc_cbwpgrad_grouped.h"

#define WGG_CSHIFT 5              // 32 per-bank copies of a table of 32 or 64 entries (wp_cshift(5) = wp_cshift(6))

// ------------------------------------------------------------------ dx, m <= 16
// k_cbwpdx_stream<XT> with centers[groups][k]: grid (column blocks, row groups), CB_THREADS threads, the same `out`.  LDS: one table
// per wave, [CB_WAVES][2^bits][32].  A wave's rows (the share k_cbwpdx_stream gives it) are walked in stretches cut at the group's
// end, each a run of batches of U rows and then single rows: a row's sum does not depend on the batch it is in.
template <typename XT, int BASE, int PLANES, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbwpdx_stream_grouped(const XT *__restrict__ g, int m, long long kdim, const unsigned char *__restrict__ packed,
                                                                      long long base_bytes, long long plane_bytes, long long ncols,
                                                                      const float *__restrict__ centers, int k, long long rows_per_group,
                                                                      long long group_rows, int direct, void *__restrict__ out_)
{
    constexpr int BITS = BASE + PLANES, E = 8 * VB / BASE, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BASE, ENTRIES = 1 << BITS;
    constexpr int COPIES = 1 << WGG_CSHIFT;
    constexpr int SH = WGG_CSHIFT + 2;                  // entry l of this lane's copy at byte l << SH
    constexpr uint32_t MASK = (1u << BASE) - 1;
    // rows in flight: k_cbwpdx_stream's, halved at 6 bits and 32 columns a lane, where eight rows of three loads on top of the 64
    // values of g and the walk took all 256 VGPRs and copies in AGPRs.  A row's sum does not depend on the batch it is in.
    constexpr int U = (PLANES == 2 && E == 32) ? 4 : CB_UNROLL;
    static_assert(E * MT <= PKG_G && (E == 4 || E == 8 || E == 16 || E == 32), "g values per lane");
    static_assert(ENTRIES <= 64, "a wave's 64 lanes hold a table, one centre each");
    extern __shared__ float smem[];
    float *out = reinterpret_cast<float *>(out_);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *cb = smem + wave * (ENTRIES * COPIES);       // this wave's table: [ENTRIES][COPIES]
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;                     // then the lane's VB base bytes and its plane bits lie inside the padded parts
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));   // the lane's columns inside the matrix
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (r < m && e < ne) ? (float)g[(long long)r * ncols + c0 + e] : 0.0f;

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *mine = packed + (active ? c0 * BASE / 8 : 0LL);
    const unsigned char *myplane = packed + base_bytes + (active ? c0 / 8 : 0LL);
    const char *tab = reinterpret_cast<const char *>(cb) + ((lane & (COPIES - 1)) << 2);
    float *dst = direct ? out : out + (long long)blockIdx.x * m * kdim;

    // lane j holds centre j of group q (rounded to XT and widened); 0 from k on (k <= 64 = the lanes of a wave)
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
            __builtin_amdgcn_sched_barrier(0);          // two broadcast values live at a time (k_cbwp_stream_grouped's fill)
        }
        __builtin_amdgcn_wave_barrier();                // the lookups below read what other lanes of this wave wrote
    };
    auto load_row = [&](long long i, uint32_t *w, uint32_t *pl) {
        pk_load<VB>(mine + i * row_bytes, w);
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = wp_plane_load<E>(myplane + i * row_bytes + p * plane_bytes, lane);
    };
    auto consume = [&](const uint32_t *w, const uint32_t *pl, long long i) {
        float s[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) s[r] = 0.0f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            uint32_t a = wp_move(w[e / PER], BASE * (e % PER), SH, MASK);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) a |= wp_move(pl[p], e, SH + BASE + p, 1u);
            const float wv = e < ne ? *reinterpret_cast<const float *>(tab + a) : 0.0f;   // (columns past the row: no Inf * 0)
#pragma unroll
            for (int r = 0; r < MT; ++r) s[r] = __builtin_fmaf(gv[r][e], wv, s[r]);
        }
        int row;
        const float v = wave_reduce_rows<MT>(s, lane, row);
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
        for (; i + U <= e1; i += U) {
            uint32_t w[U][N], pl[U][PLANES];
#pragma unroll
            for (int u = 0; u < U; ++u) load_row(i + u, w[u], pl[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) consume(w[u], pl[u], i + u);
        }
        for (; i < e1; ++i) {
            uint32_t w[N], pl[PLANES];
            load_row(i, w, pl);
            consume(w, pl, i);
        }
        if (e1 >= i1) break;
        ++group;
        __builtin_amdgcn_wave_barrier();                // the stretch's lookups stay ahead of the next fill
    }
}

// ------------------------------------------------------------------ dc, m <= 16
// k_cbwpdc_stream<XT> with sums[groups][k]: grid (column blocks, row groups), CB_THREADS threads.  LDS: one group's bins,
// [k][1 << rlog2] int64, a lane adding into copy lane mod copies.  The workgroup's rows are walked group by group as
// k_cbdc_stream_grouped walks them: each stretch is divided among the four waves; at a boundary the bins go into the group's sums
// and are cleared by the threads that have just read them, ahead of the barrier that opens the next stretch.
template <typename XT, int BASE, int PLANES, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbwpdc_stream_grouped(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
                                                                      const unsigned char *__restrict__ packed, long long base_bytes,
                                                                      long long plane_bytes, long long ncols, int k, int rlog2, int terms_log2,
                                                                      long long rows_per_group, long long group_rows, uint32_t *__restrict__ hdr,
                                                                      unsigned long long *__restrict__ sums)
{
    constexpr int E = 8 * VB / BASE, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BASE;
    constexpr uint32_t MASK = (1u << BASE) - 1;
    static_assert(E * MT <= PKG_G && (E == 4 || E == 8 || E == 16 || E == 32), "g values per lane");
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
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *mine = packed + (active ? c0 * BASE / 8 : 0LL);
    const unsigned char *myplane = packed + base_bytes + (active ? c0 / 8 : 0LL);
    unsigned long long *mybins = bins + (lane & ((1 << rlog2) - 1));
    __syncthreads();

    auto load_row = [&](long long i, uint32_t *w, uint32_t *pl) {
        pk_load<VB>(mine + i * row_bytes, w);
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = wp_plane_load<E>(myplane + i * row_bytes + p * plane_bytes, lane);
    };
    auto load_x = [&](long long i, int U, float &xa, float &xb) { cbdc_load_x<MT>(x, kdim, m, scx, lane, i, U, xa, xb); };
    auto consume = [&](const uint32_t *w, const uint32_t *pl, float xa, float xb, int u, int U) {
        float xv[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            const int f = r * U + u;
            xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            uint32_t l = (w[e / PER] >> (BASE * (e % PER))) & MASK;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) l |= ((pl[p] >> e) & 1u) << (BASE + p);
            float d = 0.0f;
#pragma unroll
            for (int r = 0; r < MT; ++r) d = __builtin_fmaf(xv[r], gv[r][e], d);   // dW'[i, o], r ascending
            if (e < ne && l < (uint32_t)k) atomicAdd(&mybins[l << rlog2], cbdc_fix(d, Sw));
        }
    };

    for (;;) {
        long long i = i0;
        for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
            uint32_t w[CB_UNROLL][N], pl[CB_UNROLL][PLANES];
            float xa, xb;
#pragma unroll
            for (int u = 0; u < CB_UNROLL; ++u) load_row(i + u, w[u], pl[u]);
            load_x(i, CB_UNROLL, xa, xb);
#pragma unroll
            for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], pl[u], xa, xb, u, CB_UNROLL);
        }
        for (; i < i1; ++i) {
            uint32_t w[N], pl[PLANES];
            float xa, xb;
            load_row(i, w, pl);
            load_x(i, 1, xa, xb);
            consume(w, pl, xa, xb, 0, 1);
        }
        cbdc_flush(bins, k, rlog2, sums + group * k);       // (begins with a barrier: every wave has left the group's rows)
        if (g_hi >= s_hi) break;                            // (s_hi and g_hi are the workgroup's: uniform)
        for (int j = threadIdx.x; j < k; j += CB_THREADS)   // the copies this thread has just summed
            for (int r = 0; r < (1 << rlog2); ++r) bins[(j << rlog2) + r] = 0ull;
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dx, m > 16, float32
// k_cbwpdx_tiled with centers[groups][k]: the same grid, tile, decode and FMA order.  LDS holds `tables` tables of 2^bits entries
// (zeros from k on, so a label >= k reads 0 with no compare), table t that of group n0 / group_rows + t; index row n0 + lr reads the
// one its group has.  c < T.hi <= ncols puts the base dword and the plane dwords inside their padded parts.
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwpdx_tiled_grouped(const float *__restrict__ g, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                              long long base_bytes, long long plane_bytes, long long ncols,
                                                              const float *__restrict__ centers, int k, long long col_tiles, long long cols_per_split,
                                                              long long group_rows, int tables, int direct, float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << (BASE + PLANES);
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: W^T[o, n0 + i] = c[group of n0 + i][label (n0 + i, o)]
    float *cb = ws + TB_K * TB_N;          // [tables][2^bits]

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    const long long q0 = T.n0 / group_rows, groups = (kdim + group_rows - 1) / group_rows;
    for (int j = threadIdx.x; j < tables * ENTRIES; j += 256) {
        const int t = j / ENTRIES, e = j % ENTRIES;
        cb[j] = (e < k && q0 + t < groups) ? centers[(q0 + t) * k + e] : 0.0f;
    }
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lo = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lo..lo+3
    const long long wi = T.n0 + lr, row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *row = packed + (wi < kdim ? wi * row_bytes : 0LL);
    const float *tab = cb + std::min((long long)tables - 1, wi / group_rows - q0) * ENTRIES;
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
        const long long c = ob + lo;
        const bool live = wi < kdim && c < T.hi;
        const uint32_t word = live ? *reinterpret_cast<const uint32_t *>(row + (c * BASE / 32) * 4) : 0u;
        uint32_t pl[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = live ? *reinterpret_cast<const uint32_t *>(row + base_bytes + p * plane_bytes + (c / 32) * 4) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[(lo + j) * TB_N + lr] = (live && c + j < T.hi) ? tab[wg_label<BASE, PLANES>(word, pl, c + j)] : 0.0f;
        __syncthreads();
        tb_tile_fma(gs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_dx(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, kdim, direct, out);
}

// ------------------------------------------------------------------ dc, m > 16, float32
// k_cbwpdc_tiled with sums[groups][k]: the same grid, tiles and FMA order.  The k << rlog2 LDS bins are cut into 1 << sets_log2 sets
// of k << (rlog2 - sets_log2), set t for group m0 / group_rows + t.  Thread (tx, ty) bins index rows m0 + ty * 8 .. + 7, which lie in
// one group, into that group's set; every set then goes into its group's sums.
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwpdc_tiled_grouped(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                              const unsigned char *__restrict__ packed, long long base_bytes, long long plane_bytes,
                                                              long long ncols, int k, int rlog2, int sets_log2, int terms_log2, long long col_tiles,
                                                              long long rows_per_split, long long group_rows, uint32_t *__restrict__ hdr,
                                                              unsigned long long *__restrict__ sums)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]: x[r, i0 + i]
    float *gs = xs + TB_K * TB_M;          // [TB_K][TB_N]: g[r, o0 + o]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + TB_K * TB_N);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, k << rlog2, scx, scg, Sw)) return;

    const TbTile T = tb_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i
    float acc[8][8];
    tb_clear(acc);
    for (long long rb = T.lo; rb < T.hi; rb += TB_K) {
        __syncthreads();
        cbdc_load_tiles(xs, gs, x, g, kdim, ncols, T.m0, T.n0, rb, T.hi, scx, scg);
        __syncthreads();
        tb_tile_fma(xs, gs, T.tx, T.ty, acc);
    }
    const int rl = rlog2 - sets_log2, sets = 1 << sets_log2;
    const long long q0 = T.m0 / group_rows, groups = (kdim + group_rows - 1) / group_rows;
    const int set = (int)std::min((long long)sets - 1, (T.m0 + T.ty * 8) / group_rows - q0);
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    // a column inside the matrix puts its base dword and its plane dwords inside the padded parts of row i < kdim
    cbdc_bin_tile(acc, T, kdim, ncols, k, Sw, bins + ((long long)set * k << rl), rl, threadIdx.x & ((1 << rl) - 1), [&](long long i, long long o) {
        const unsigned char *row = packed + i * row_bytes;
        const uint32_t word = *reinterpret_cast<const uint32_t *>(row + (o * BASE / 32) * 4);
        uint32_t pl[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = *reinterpret_cast<const uint32_t *>(row + base_bytes + p * plane_bytes + (o / 32) * 4);
        return wg_label<BASE, PLANES>(word, pl, o);
    });
    for (int t = 0; t < sets && q0 + t < groups; ++t) cbdc_flush(bins + ((long long)t * k << rl), k, rl, sums + (q0 + t) * k);
}

// ------------------------------------------------------------------ dx, m > 16, bf16 / fp16
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads; out, direct and cols_per_split as k_cbdx_mfma.  LDS: 1 << tlog2
// tables of ENTRIES << (WGG_CSHIFT - tlog2) words (table t that of group n0 / group_rows + t, the centres rounded to XT, zeros from k
// on), the staging row, the two images: k_cbwpdx_mfma's bytes.  Thread t owns index row n0 + (t mod 128), hence one table, and 16
// consecutive o of the step starting at o0 = ob + wk0, a multiple of 16: 8 aligned bytes of the base part and 2 aligned bytes of
// every plane; o0 < k_hi <= ncols puts them inside the padded parts.
template <typename XT, int BASE, int PLANES, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbwpdx_mfma_grouped(const XT *__restrict__ g, long long m, long long kdim,
                                                                    const unsigned char *__restrict__ packed, long long base_bytes, long long plane_bytes,
                                                                    long long ncols, const float *__restrict__ centers, int k, int tlog2,
                                                                    long long col_tiles, long long cols_per_split, long long group_rows, int direct,
                                                                    void *__restrict__ out_)
{
    constexpr int ENTRIES = 1 << (BASE + PLANES), PER = 32 / BASE, NW = 16 / PER;
    constexpr uint32_t MASK = (1u << BASE) - 1;
    static_assert(BASE == 4, "8 bytes of the base part hold a thread's 16 fields");
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, ENTRIES, WGG_CSHIFT);   // xs: the g tile, row-major in o; ws: the W^T tile, [i][o]

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);    // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const int tcs = WGG_CSHIFT - tlog2, tables = 1 << tlog2;       // the copies of one table (log2)
    const TileGroups G = tile_groups_at(T.n0, kdim, group_rows);
    for (int t = 0; t < tables; ++t) {                  // (uniform over the workgroup; a table past the last group repeats it, unread)
        if (t) __syncthreads();                         // the staging row of the table before has been copied
        cb_fill<XT>(L.cb + (long long)t * (ENTRIES << tcs), L.stage, centers + std::min(G.q0 + t, G.groups - 1) * k, k, ENTRIES, tcs);
    }

    const long long gi = T.n0 + T.wc, row_bytes = base_bytes + PLANES * plane_bytes;
    const bool row_ok = gi < kdim;
    const unsigned char *prow = packed + (row_ok ? gi * row_bytes : 0LL);
    const float *tab = L.cb + tile_group_of(G, gi, group_rows, tables) * (ENTRIES << tcs) + (T.lane & ((1 << tcs) - 1));
    uint32_t lw[NW], pl[PLANES];

    auto load_w = [&](long long ob) {
        const long long o0 = ob + T.wk0;
#pragma unroll
        for (int d = 0; d < NW; ++d) lw[d] = 0u;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = 0u;
        if (row_ok && o0 < T.k_hi) {
            load_chunk<4 * NW>(prow + o0 * BASE / 8, lw);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) pl[p] = *reinterpret_cast<const uint16_t *>(prow + base_bytes + p * plane_bytes + o0 / 8);
        }
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint32_t l = (lw[j / PER] >> (BASE * (j % PER))) & MASK;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) l |= ((pl[p] >> j) & 1u) << (BASE + p);
            // a column past the split, so every column past ncols, is 0 and not table[label 0 of the padding]
            w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? tab[l << tcs] : 0.0f;
        }
        hm_store_w(L.ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(g, m, ncols, T, L.xs, L.ws, acc, load_w, store_w);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16, bf16 / fp16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads.  LDS: the two images, then the k << rlog2 int64 bins, cut into
// 1 << sets_log2 sets of k << (rlog2 - sets_log2), set t for group m0 / group_rows + t.  rows_per_split and XVEC as k_cbdc_mfma.
template <typename XT, int BASE, int PLANES, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbwpdc_mfma_grouped(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                                    const unsigned char *__restrict__ packed, long long base_bytes, long long plane_bytes,
                                                                    long long ncols, int k, int rlog2, int sets_log2, int terms_log2, long long col_tiles,
                                                                    long long rows_per_split, long long group_rows, uint32_t *__restrict__ hdr,
                                                                    unsigned long long *__restrict__ sums)
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

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col): its 32 rows lie in one group, whose set is a scalar.  The 32 lanes
    // of a row read 32 consecutive fields of packed row i, which start on a multiple of 32 columns: the lane's base dword and the
    // plane dwords all 32 share lie inside the padded parts when the lane's column lies inside the matrix
    const int rl = rlog2 - sets_log2, sets = 1 << sets_log2;
    const TileGroups G = tile_groups_at(T.m0, kdim, group_rows);
    const long long row0 = tile_wave_row0(T.m0), row_bytes = base_bytes + PLANES * plane_bytes;
    const int rep = T.lane & ((1 << rl) - 1);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int set = (int)tile_group_of(G, row0 + a * 32, group_rows, sets);
        unsigned long long *mybins = bins + ((long long)set * k << rl) + rep;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const long long o = hm_acc_col(T.n0 + T.wn, b, T.lane);
            if (o >= ncols) continue;
            const unsigned char *bcol = packed + (o * BASE / 32) * 4, *pcol = packed + base_bytes + (o / 32) * 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = hm_acc_row(T.m0 + T.wm, a, r, T.lane);
                if (i >= kdim) continue;
                uint32_t pl[PLANES];
#pragma unroll
                for (int p = 0; p < PLANES; ++p) pl[p] = *reinterpret_cast<const uint32_t *>(pcol + i * row_bytes + p * plane_bytes);
                const uint32_t l = wg_label<BASE, PLANES>(*reinterpret_cast<const uint32_t *>(bcol + i * row_bytes), pl, o);
                if (l < (uint32_t)k) atomicAdd(&mybins[l << rl], cbdc_fix(acc[a][b][r], Sw));
            }
        }
    }
    for (int t = 0; t < sets && G.q0 + t < G.groups; ++t) cbdc_flush(bins + ((long long)t * k << rl), k, rl, sums + (G.q0 + t) * k);
}

// ------------------------------------------------------------------ launches
// one signature per direction and path for the three dtypes: g, x and out travel as void *; `held_log2` is the tables of a dx tile
// (log2; the float32 tile takes the count) or the sets of a dc tile
template <typename XT, int BASE, int PLANES, int VB, int MT>
static void launch_dx_stream(dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const WgArgs &w, const float *centers, int k,
                             long long rpg, long long group_rows, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbwpdx_stream_grouped<XT, BASE, PLANES, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(g), m, kdim, w.packed,
                       w.base_bytes, w.plane_bytes, w.ncols, centers, k, rpg, group_rows, direct, out);
}

template <typename XT, int BASE, int PLANES, int VB, int MT>
static void launch_dc_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const WgArgs &w, int k, int rlog2,
                             int tl, long long rpg, long long group_rows, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbwpdc_stream_grouped<XT, BASE, PLANES, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x),
                       reinterpret_cast<const XT *>(g), m, kdim, w.packed, w.base_bytes, w.plane_bytes, w.ncols, k, rlog2, tl, rpg, group_rows, hdr, sums);
}

template <typename XT, int BASE, int PLANES>
static void launch_dx_tile(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const WgArgs &w, const float *centers, int k,
                           int held_log2, long long col_tiles, long long cps, long long group_rows, int direct, void *out)
{
    if constexpr (std::is_same<XT, float>::value)
        hipLaunchKernelGGL((k_cbwpdx_tiled_grouped<BASE, PLANES>), grid, dim3(256), lds, s, reinterpret_cast<const float *>(g), m, kdim, w.packed,
                           w.base_bytes, w.plane_bytes, w.ncols, centers, k, col_tiles, cps, group_rows, 1 << held_log2, direct,
                           reinterpret_cast<float *>(out));
    else
        hm_launch(g, w.ncols, k_cbwpdx_mfma_grouped<XT, BASE, PLANES, true>, k_cbwpdx_mfma_grouped<XT, BASE, PLANES, false>, grid, lds, s,
                  reinterpret_cast<const XT *>(g), m, kdim, w.packed, w.base_bytes, w.plane_bytes, w.ncols, centers, k, held_log2, col_tiles, cps, group_rows,
                  direct, out);
}

template <typename XT, int BASE, int PLANES>
static void launch_dc_tile(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const WgArgs &w, int k,
                           int rlog2, int held_log2, int tl, long long col_tiles, long long rps, long long group_rows, uint32_t *hdr,
                           unsigned long long *sums)
{
    if constexpr (std::is_same<XT, float>::value)
        hipLaunchKernelGGL((k_cbwpdc_tiled_grouped<BASE, PLANES>), grid, dim3(256), lds, s, reinterpret_cast<const float *>(x),
                           reinterpret_cast<const float *>(g), m, kdim, w.packed, w.base_bytes, w.plane_bytes, w.ncols, k, rlog2, held_log2, tl, col_tiles, rps,
                           group_rows, hdr, sums);
    else
        hipLaunchKernelGGL((dcm_xvec(x, g, kdim, w.ncols) ? k_cbwpdc_mfma_grouped<XT, BASE, PLANES, true> : k_cbwpdc_mfma_grouped<XT, BASE, PLANES, false>),
                           grid, dim3(HM_THREADS), lds, s, reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim, w.packed, w.base_bytes,
                           w.plane_bytes, w.ncols, k, rlog2, held_log2, tl, col_tiles, rps, group_rows, hdr, sums);
}

// every kernel instantiation of this unit: per dtype the base-4 stream list of nnc_cbwpgrad.hpp at one and two planes, and the tiles
// (the float32 tile or the MFMA tile, by dtype); the plans are checked against these tables, and the launches go through them
using WggDxStream = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const WgArgs &, const float *, int, long long, long long, int, void *);
using WggDcStream = void (*)(dim3, size_t, hipStream_t, const void *, const void *, int, long long, const WgArgs &, int, int, int, long long, long long,
                             uint32_t *, unsigned long long *);
using WggDxTile = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const WgArgs &, const float *, int, int, long long, long long,
                           long long, int, void *);
using WggDcTile = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const WgArgs &, int, int, int, int, long long,
                           long long, long long, uint32_t *, unsigned long long *);
struct WggStreamCase {
    int a, vb, mt;            // a: bits
    WggDxStream dx;
    WggDcStream dc;
};
struct WggTileCase {
    int dt, a;                // a: bits
    WggDxTile dx;
    WggDcTile dc;
};
#define WGG_F32(B, P, V, M) {B + P, V, M, launch_dx_stream<float, B, P, V, M>, launch_dc_stream<float, B, P, V, M>},
#define WGG_BF16(B, P, V, M) {B + P, V, M, launch_dx_stream<bf16_t, B, P, V, M>, launch_dc_stream<bf16_t, B, P, V, M>},
#define WGG_F16(B, P, V, M) {B + P, V, M, launch_dx_stream<f16_t, B, P, V, M>, launch_dc_stream<f16_t, B, P, V, M>},
static const WggStreamCase kWggF32Cases[] = {WPG_BASE4_CASES(WGG_F32, 1) WPG_BASE4_CASES(WGG_F32, 2)};
static const WggStreamCase kWggBf16Cases[] = {WPG_BASE4_CASES(WGG_BF16, 1) WPG_BASE4_CASES(WGG_BF16, 2)};
static const WggStreamCase kWggF16Cases[] = {WPG_BASE4_CASES(WGG_F16, 1) WPG_BASE4_CASES(WGG_F16, 2)};
#undef WGG_F32
#undef WGG_BF16
#undef WGG_F16
#define WGG_TILES(DT, XT) {DT, 5, launch_dx_tile<XT, 4, 1>, launch_dc_tile<XT, 4, 1>}, {DT, 6, launch_dx_tile<XT, 4, 2>, launch_dc_tile<XT, 4, 2>}
static const WggTileCase kWggTileCases[] = {WGG_TILES(NNC_DT_F32, float), WGG_TILES(NNC_DT_BF16, bf16_t), WGG_TILES(NNC_DT_F16, f16_t)};
#undef WGG_TILES
static const CbgCaseNames kWggNames = {true, "bits", true};

// The instantiations plan p asks for: sc on the stream path, tc on a tile path (NNC_EINVAL and a message if a table has none), both
// NULL on the paths that launch nothing of this unit.
static int wgg_find(const char *fn, const PgPlan &p, int dt, int bits, const WggStreamCase *&sc, const WggTileCase *&tc)
{
    tc = nullptr;
    const int rc = cbg_stream_case(fn, wg_cases(dt, kWggF32Cases, kWggBf16Cases, kWggF16Cases), kWggNames, p.path, bits, p.vb, p.mt, sc);
    if (rc != NNC_OK || (p.path != NNC_CBMM_TILED && p.path != NNC_CBMM_MFMA)) return rc;
    for (const WggTileCase &c : kWggTileCases)
        if (c.dt == dt && c.a == bits) tc = &c;
    if (tc) return NNC_OK;
    return fail(NNC_EINVAL, std::string(fn) + ": no grouped tile instantiation for dtype " + std::to_string(dt) + ", bits " + std::to_string(bits));
}

// ------------------------------------------------------------------ plans (host)
// wg_dx_plan / wg_dc_plan for the shape, then what the groups change.  dx: the LDS (stream: one table per wave and no staging row;
// float32 tile: a table per group of the tile; MFMA tile: the ungrouped table's copies divided over the tables) and `held`, the
// tables in LDS.  dc: `held`, the per-group sets the copies of a bin are cut into (LDS unchanged).  copies: those of one table / set.
static bool wgg_tile_path(int path) { return path == NNC_CBMM_TILED || path == NNC_CBMM_MFMA; }

static PgPlan wgg_dx_plan(int x_dtype, long long m, long long kdim, long long ncols, int bits, long long group_rows, int cus, int &held)
{
    PgPlan p = wg_dx_plan(x_dtype, m, kdim, ncols, bits, cus);
    held = 0;
    if (p.path == NNC_CBMM_STREAM) {
        held = CB_WAVES;
        p.lds = ((long long)CB_WAVES * p.entries << WGG_CSHIFT) * 4;
    } else if (wgg_tile_path(p.path)) {
        held = tile_groups(group_rows);
        if (p.path == NNC_CBMM_TILED) p.lds += (long long)(held - 1) * p.entries * 4;
        else p.copies /= held;
    }
    return p;
}

static int wgg_dc_plan(int x_dtype, long long m, long long kdim, long long ncols, int bits, int k, long long group_rows, int cus, PgPlan &p, int &held)
{
    const int rc = wg_dc_plan(x_dtype, m, kdim, ncols, bits, k, cus, p);
    held = rc != NNC_OK ? 0 : (p.path == NNC_CBMM_STREAM ? 1 : (wgg_tile_path(p.path) ? tile_groups(group_rows) : 0));
    if (held > 1) p.copies /= held;
    return rc;
}

static void wgg_plan_tail(const PgPlan &p, int64_t kdim, int64_t group_rows, int held, int64_t *out)
{
    cbg_grouped_plan_tail(p.path == NNC_CBMM_MFMA ? NNC_CBMM_TILED : p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out);
    out[4] = held;
}

// ------------------------------------------------------------------ C ABI
// wpg_check's checks (nnc_cbwp.hpp: bits, k, wp_check's, group_rows and the bound on the G * k bins), then wg_check's bound on m * kdim
static int wgg_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows)
{
    const int rc = wpg_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows, k);
    if (rc != NNC_OK) return rc;
    if (m > 0 && kdim > (1LL << 44) / m) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

extern "C" int64_t nnc_cbwp_grouped_dx_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (wgg_check("nnc_cbwp_grouped_dx_workspace_bytes", x_dtype, m, kdim, ncols, bits, 17, 32) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(wg_dx_plan(x_dtype, m, kdim, ncols, bits, CB_PLAN_CUS).splits, m, kdim);
}

extern "C" int nnc_cbwp_grouped_dx_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus,
                                        int64_t *out)
{
    const char *fn = "nnc_cbwp_grouped_dx_plan";
    int rc = wgg_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dx_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dx_plan: out is NULL");
    int held;
    const PgPlan p = wgg_dx_plan(x_dtype, m, kdim, ncols, bits, group_rows, cus, held);
    const WggStreamCase *sc;
    const WggTileCase *tc;
    if ((rc = wgg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    const bool none = p.path == NNC_CBMM_NONE || p.path == NNC_CBMM_ZERO;
    const int64_t v[NNC_CBWPDX_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, none ? 0 : wp_base(bits), none ? 0 : bits - wp_base(bits), p.copies, p.entries,
                                            p.splits, p.per_split, p.lds, p.col_tiles, p.row_tiles, cbg_dx_ws_bytes(p.splits, m, kdim), x_dtype};
    for (int i = 0; i < NNC_CBWPDX_PLAN_LEN; ++i) out[i] = v[i];
    wgg_plan_tail(p, kdim, group_rows, held, out + NNC_CBWPDX_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbwp_grouped_dx(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                                   const float *centers_dev, int32_t k, int64_t group_rows, void *dx, int dx_dtype, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbwp_grouped_dx";
    int rc = wgg_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dx: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dx: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dx: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dx: g is NULL");
    if (reinterpret_cast<uintptr_t>(g) % (x_dtype == NNC_DT_F32 ? 4 : 2) || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbwp_grouped_dx: g or dx is not aligned to its element size");
    const int64_t need = nnc_cbwp_grouped_dx_workspace_bytes(x_dtype, m, kdim, ncols, bits);
    if ((rc = cb_check_workspace(fn, "nnc_cbwp_grouped_dx_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK)
        return rc;
    int held;
    PgPlan p = wgg_dx_plan(x_dtype, m, kdim, ncols, bits, group_rows, CB_PLAN_CUS, held);
    const WggStreamCase *sc;
    const WggTileCase *tc;
    if ((rc = wgg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM) p = wgg_dx_plan(x_dtype, m, kdim, ncols, bits, group_rows, cu_count(), held);   // (the row groups of this device)
    const WgArgs w = {reinterpret_cast<const unsigned char *>(packed), wp_base_bytes(ncols, bits), wp_plane_bytes(ncols), ncols};
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, w, centers_dev, k, p.rows_per_group, group_rows, direct,
                   out);
            LAUNCHCHK("k_cbwpdx_stream_grouped");
        } else {
            tc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, w, centers_dev, k, __builtin_ctz(held),
                   p.col_tiles, p.per_split, group_rows, direct, out);
            LAUNCHCHK((p.path == NNC_CBMM_MFMA ? "k_cbwpdx_mfma_grouped" : "k_cbwpdx_tiled_grouped"));
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbwp_grouped_dc_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows)
{
    if (wgg_check("nnc_cbwp_grouped_dc_workspace_bytes", x_dtype, m, kdim, ncols, bits, k, group_rows) != NNC_OK) return 0;
    PgPlan p;
    if (wg_dc_plan(x_dtype, m, kdim, ncols, bits, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return h16_dc_ws_bytes(p.path, gg_groups(kdim, group_rows) * k);
}

extern "C" int nnc_cbwp_grouped_dc_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus,
                                        int64_t *out)
{
    const char *fn = "nnc_cbwp_grouped_dc_plan";
    int rc = wgg_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dc_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dc_plan: out is NULL");
    PgPlan p;
    int held;
    if ((rc = wgg_dc_plan(x_dtype, m, kdim, ncols, bits, k, group_rows, cus, p, held)) != NNC_OK) return rc;
    const WggStreamCase *sc;
    const WggTileCase *tc;
    if ((rc = wgg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    const bool zero = p.path == NNC_CBMM_ZERO;
    const int64_t v[NNC_CBWPDC_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, zero ? 0 : wp_base(bits), zero ? 0 : bits - wp_base(bits), p.copies, p.splits,
                                            p.per_split, p.lds, p.col_tiles, p.row_tiles, p.terms_log2,
                                            h16_dc_ws_bytes(p.path, gg_groups(kdim, group_rows) * k), x_dtype};
    for (int i = 0; i < NNC_CBWPDC_PLAN_LEN; ++i) out[i] = v[i];
    wgg_plan_tail(p, kdim, group_rows, held, out + NNC_CBWPDC_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbwp_grouped_dc(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                                   int64_t ncols, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes,
                                   void *stream)
{
    const char *fn = "nnc_cbwp_grouped_dc";
    int rc = wgg_check(fn, x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dc: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbwp_grouped_dc: x or g is NULL");
    const int eb = x_dtype == NNC_DT_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(x) % eb || reinterpret_cast<uintptr_t>(g) % eb)
        return fail(NNC_EINVAL, "nnc_cbwp_grouped_dc: x or g is not aligned to its element size");
    PgPlan p;
    int held;
    if ((rc = wgg_dc_plan(x_dtype, m, kdim, ncols, bits, k, group_rows, CB_PLAN_CUS, p, held)) != NNC_OK) return rc;
    const int nbins = (int)(gg_groups(kdim, group_rows) * k);
    const int64_t need = h16_dc_ws_bytes(p.path, nbins);
    if ((rc = cb_check_workspace(fn, "nnc_cbwp_grouped_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK)
        return rc;
    const WggStreamCase *sc;
    const WggTileCase *tc;
    if ((rc = wgg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM && (rc = wgg_dc_plan(x_dtype, m, kdim, ncols, bits, k, group_rows, cu_count(), p, held)) != NNC_OK)
        return rc;                                                                        // (the row groups of this device)
    const WgArgs w = {reinterpret_cast<const unsigned char *>(packed), wp_base_bytes(ncols, bits), wp_plane_bytes(ncols), ncols};
    const int rlog2 = dc_rlog2(k);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, w, k, rlog2, p.terms_log2, p.rows_per_group,
                   group_rows, hdr, sums);
            LAUNCHCHK("k_cbwpdc_stream_grouped");
        } else {
            tc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, w, k, rlog2, __builtin_ctz(held),
                   p.terms_log2, p.col_tiles, p.per_split, group_rows, hdr, sums);
            LAUNCHCHK((p.path == NNC_CBMM_MFMA ? "k_cbwpdc_mfma_grouped" : "k_cbwpdc_tiled_grouped"));
        }
        return NNC_OK;
    });
}
