// nnc_cbspgrad_grouped.hip -- the backward pass of the pruned group-wise codebook layer (nnc_cbsp_grouped.hip) from the bitmap-sparse
// form of its indices: nothing is unpacked, neither W nor dW is written (include/nnc_cbspgrad_grouped.h, nnc_cbsp_grouped_dx_f32 /
// nnc_cbsp_grouped_dc_f32).  Group q = i / group_rows has the table c_q and the skipped symbol z_q;
// c_{z_q} = c_q[z_q] (0 if z_q >= k), d_q[s] = float32(c_q[s] - c_{z_q}) (-c_{z_q} for s >= k), g = dL/dy:
//
//   dx[r, i] = c_{z_q} * sum_o g[r, o] + sum over the stored (i, o) of g[r, o] * d_q[L[i, o]]   the Jacobian of nnc_cbsp_grouped_f32;
//                                                                                              with c_{z_q} == 0 no rank-1 term
//   dc[q, k] = nnc_cbmm_grouped_dc_f32 on the unpacked labels, bit for bit; a skipped (i, o) falls into bin (q, z_q), none if z_q >= k
//
// The plans are the ungrouped sparse ones (sg_dx_plan, sg_dc_plan of nnc_cbspgrad.hpp at label_bytes 1), so the path, the grids, the
// splits, the order in which every sum is formed and the shift S of the dc sums are those of nnc_cbsp_dx_f32 / nnc_cbsp_dc_f32 on the
// same shape.  The kernels are the ungrouped ones (nnc_cbspgrad.hpp, nnc_cbspgrad.hip) with the additions the group-wise byte form
// makes (nnc_cbgrad_grouped.hpp, nnc_cbgrad_grouped.hip); kernels of their own for the reason nnc_cbmm_grouped.hip gives.
//   k_cbspgdx_stream  m <= 16.  k_cbspdx_stream<float, uint8_t, MT>; the workgroup's index rows go group by group (cb_group_step), each
//                     stretch divided among the four waves, the d table refilled between two barriers (the min(k + 1, 256) entries a
//                     symbol can reach; the lookup clamps, as k_cbspg_stream).  A batch of 64 / E rows ends with its stretch.
//   k_cbspgdx_tiled   m > 16.  k_cbspdx_tiled<uint8_t> with k_cbdx_tiled_grouped's tables: the d tables of the up to four groups of
//                     the tile's 128 index rows are loaded once; a thread decodes one row and keeps a pointer to that row's table.
//   k_cbspgdx_rank1   dx[r, i] = c_{z_q} * rs[r] + dx[r, i] where c_{z_q} != 0, nothing elsewhere.
//   k_cbspgdc_stream  m <= 16.  k_cbspdc_stream<float, uint8_t, MT> with the same walk; the LDS bins are one group's.  At the end of a
//                     stretch a lane's skip register goes into bin z_q and is cleared, the bins go into sums + q * k and are
//                     cleared by the threads that summed them (k_cbdc_stream_grouped with the skip register).
//   k_cbspgdc_tiled   m > 16.  k_cbspdc_tiled<uint8_t> with k_cbdc_tiled_grouped's sets of bins; a thread's 8 index rows lie in one
//                     group, so its one skip register goes into bin z_q of its set.
// Everything that steers a walk comes from blockIdx, the kernel arguments and the wave number (a scalar): every wave of a workgroup
// reaches every barrier, also one whose share of a stretch is empty, and no v_readlane stands under a lane-dependent branch.
// The row sums (cbsp_rowsum), k_cbgrad_absmax, k_cbgrad_reduce, k_cbdc_finish (over G * k bins) and the host sequences (cbg_run_dx,
// cbg_run_dc) are shared with the other backward units.  No float atomics; no host read.
#include "nnc_cbspgrad.hpp"
#include "nnc_cbsp_grouped.hpp"
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ dx, m <= 16
// grid (column blocks, row groups), CB_THREADS threads; LDS as k_cbspdx_stream: the d table (entries << cshift), the staging row.
// out: dx (one column block) or the float32 partials [block][m][kdim] (direct 0).  rows_per_group is the workgroup's index rows (the
// plan's name), not group_rows.
template <int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbspgdx_stream(const float *__restrict__ g, int m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                               const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                               const uint8_t *__restrict__ sym, long long nnz, long long ncols, long long segs,
                                                               const float *__restrict__ centers, int k, const uint8_t *__restrict__ zsym,
                                                               long long group_rows, int entries, int cshift, long long rows_per_group, int direct,
                                                               float *__restrict__ out)
{
    constexpr int E = sg_segs(MT), RB = 64 / E, UR = E >= 8 ? 1 : 8 / E;   // segments per block, rows per batch, rows per step
    extern __shared__ float smem[];
    float *tab = smem;
    float *stage = smem + (entries << cshift);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long blk = blockIdx.x;
    const long long s_lo = (long long)blockIdx.y * rows_per_group, s_hi = std::min(kdim, s_lo + rows_per_group);
    long long group = s_lo / group_rows;
    long long g_lo = s_lo, g_hi, i0, i1;   // the rows of the workgroup that lie in `group`, and the wave's share of them
    cb_group_step(group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
    const int top = std::min(k, entries - 1);   // entry min(symbol, top): d of the symbol, or -c_{z_q} (k < 256: a symbol can pass k)
    sp_fill<float>(tab, stage, centers + group * k, k, spg_cz(centers, k, zsym, group), top + 1, cshift);

    float gv[MT][E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const long long col = (blk * E + e) * 64 + lane;
#pragma unroll
        for (int r = 0; r < MT; ++r) gv[r][e] = (r < m && col < ncols) ? g[(long long)r * ncols + col] : 0.0f;
    }
    float *dst = direct ? out : out + blk * m * kdim;
    __syncthreads();

    for (;;) {
        uint64_t wn;
        long long cn;
        sg_batch<E>(bitmap, lo, hi, segs, blk, i0, i1, lane, wn, cn);
        for (long long ib = i0; ib < i1; ib += RB) {
            const uint64_t wl = wn;
            const long long cl = cn;
            if (ib + RB < i1) sg_batch<E>(bitmap, lo, hi, segs, blk, ib + RB, i1, lane, wn, cn);   // the next batch of the stretch in flight
            const int nb = (int)std::min((long long)RB, i1 - ib);
            for (int u0 = 0; u0 < nb; u0 += UR) {
                uint32_t bits[UR][E], sv[UR][E];
                sg_symbols<uint8_t, E, UR>(wl, cl, u0, lane, sym, nnz, bits, sv);
#pragma unroll
                for (int u = 0; u < UR; ++u) {
                    float p[MT];
#pragma unroll
                    for (int r = 0; r < MT; ++r) p[r] = 0.0f;
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const float dv = tab[CbTable<uint8_t>::index(std::min(sv[u][e], (uint32_t)top), k, cshift, lane)];
#pragma unroll
                        for (int r = 0; r < MT; ++r) p[r] = bits[u][e] ? __builtin_fmaf(gv[r][e], dv, p[r]) : p[r];   // skipped: no product
                    }
                    int row;
                    const float v = wave_reduce_rows<MT>(p, lane, row);
                    if (u0 + u < nb && (lane & (64 / MT - 1)) == 0 && row < m) dst[(long long)row * kdim + ib + u0 + u] = v;
                }
            }
        }
        if (g_hi >= s_hi) break;   // (the same test for the four waves)
        // on to the next group's rows, divided among the waves as the whole range is
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();   // every wave has left the rows of the group before
        sp_fill<float>(tab, stage, centers + group * k, k, spg_cz(centers, k, zsym, group), top + 1, cshift);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dx, m > 16
// k_cbspdx_tiled<uint8_t> with centers[groups][k] and zsym[groups]: the same grid, tile and FMA order.  LDS holds `tables` d tables of
// k + 1 entries (entry k = -c_{z_q}) ahead of the kept mask, table t that of group n0 / group_rows + t.
__global__ __launch_bounds__(256) void k_cbspgdx_tiled(const float *__restrict__ g, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                       const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym,
                                                       long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                       const uint8_t *__restrict__ zsym, long long group_rows, int tables, long long col_tiles,
                                                       long long cols_per_split, int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: d of the stored W[n0 + i, o], 0 where skipped
    float *cb = ws + TB_K * TB_N;          // [tables][k + 1]: d, then -c_z, of the tile's groups
    unsigned char *kept = reinterpret_cast<unsigned char *>(cb + tables * (k + 1));   // [TB_K][TB_N]: 1 where the weight is stored

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    const long long q0 = T.n0 / group_rows, groups = (kdim + group_rows - 1) / group_rows;
    for (int j = threadIdx.x; j < tables * (k + 1); j += 256) {
        const int t = j / (k + 1), e = j - t * (k + 1);
        float v = 0.0f;
        if (q0 + t < groups) v = (e < k ? centers[(q0 + t) * k + e] : 0.0f) - spg_cz(centers, k, zsym, q0 + t);
        cb[j] = v;
    }
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lq = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lq..lq+3 (one segment), as the g tile
    const long long wi = T.n0 + lr;
    const float *tab = cb + std::min((long long)tables - 1, wi / group_rows - q0) * (k + 1);   // the table of the thread's row
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        const int nonfinite = tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
        const long long go = ob + lq;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t keep = 0;
        if (wi < kdim && go < T.hi) {   // (bits past ncols are 0; a split ends on a segment boundary)
            const long long gi = wi * segs, sg = go >> 6;
            const int b0 = (int)(go & 63);
            const uint64_t word = bitmap[gi + sg];
            long long pos = sp_count(lo[gi + sg], lo[gi], hi[wi]) + __popcll(word & ((1ULL << b0) - 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((word >> (b0 + j)) & 1) {
                    if (pos < nnz) {
                        v[j] = tab[std::min((uint32_t)sym[pos], (uint32_t)k)];
                        keep |= 1u << j;
                    }
                    ++pos;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[(lq + j) * TB_N + lr] = v[j];
            kept[(lq + j) * TB_N + lr] = (unsigned char)((keep >> j) & 1);
        }
        // a skipped weight is absent: where the g tile holds an Inf or NaN the FMA must not form g * 0 at a skipped position
        if (__syncthreads_or(nonfinite)) tb_tile_fma_masked(gs, ws, kept, T.tx, T.ty, acc);
        else tb_tile_fma(gs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_dx(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, kdim, direct, out);
}

// ------------------------------------------------------------------ dx += c_{z_q} * row sums of g (k_cbspdx_rank1 with the centre per column)
__global__ __launch_bounds__(256) void k_cbspgdx_rank1(float *__restrict__ dx, long long m, long long kdim, const float *__restrict__ rs,
                                                       const float *__restrict__ centers, int k, const uint8_t *__restrict__ zsym, long long group_rows)
{
    // grid (column blocks, row strides): a thread owns column i, looks its group's centre up once and walks the rows; a column whose
    // group has c_z == 0 costs that one lookup (the common case after prune -> quantize: the pruned cluster's centre)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < kdim; i += (long long)gridDim.x * blockDim.x) {
        const float cz = spg_cz(centers, k, zsym, i / group_rows);
        if (!(cz != 0.0f)) continue;   // (a NaN centre counts; c_z == 0: the rank-1 term is dropped)
        for (long long r = blockIdx.y; r < m; r += gridDim.y) dx[r * kdim + i] = cz * rs[r] + dx[r * kdim + i];
    }
}

// ------------------------------------------------------------------ dc, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  LDS: one group's bins, [k][1 << rlog2] int64; sums[groups][k].
template <int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbspgdc_stream(const float *__restrict__ x, const float *__restrict__ g, int m, long long kdim,
                                                               const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo,
                                                               const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym, long long nnz,
                                                               long long ncols, long long segs, int k, const uint8_t *__restrict__ zsym,
                                                               long long group_rows, int rlog2, int terms_log2, long long rows_per_group,
                                                               uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    constexpr int E = sg_segs(MT), RB = 64 / E, UR = E >= 8 ? 1 : 8 / E;
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
    const long long blk = blockIdx.x;
    float gv[MT][E];
    bool incol[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const long long col = (blk * E + e) * 64 + lane;
        incol[e] = col < ncols;
#pragma unroll
        for (int r = 0; r < MT; ++r) gv[r][e] = g[cbdc_idx((long long)r * ncols + col, r < m && incol[e])];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int r = 0; r < MT; ++r) gv[r][e] = cbdc_scaled(gv[r][e], r < m && incol[e], scg);

    const long long s_lo = (long long)blockIdx.y * rows_per_group, s_hi = std::min(kdim, s_lo + rows_per_group);
    long long group = s_lo / group_rows;
    long long g_lo = s_lo, g_hi, i0, i1;   // the rows of the workgroup that lie in `group`, and the wave's share of them
    cb_group_step(group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
    unsigned long long skip = 0;   // the images of the lane's skipped weights in this group: bin z_q
    __syncthreads();

    for (;;) {
        uint64_t wn;
        long long cn;
        sg_batch<E>(bitmap, lo, hi, segs, blk, i0, i1, lane, wn, cn);
        for (long long ib = i0; ib < i1; ib += RB) {
            const uint64_t wl = wn;
            const long long cl = cn;
            if (ib + RB < i1) sg_batch<E>(bitmap, lo, hi, segs, blk, ib + RB, i1, lane, wn, cn);   // the next batch of the stretch in flight
            const int nb = (int)std::min((long long)RB, i1 - ib);
            for (int u0 = 0; u0 < nb; u0 += UR) {
                // x[r, i] of the UR rows: lane f holds x[f / UR, ib + u0 + f % UR] (f < MT * UR <= 64), broadcast by v_readlane
                float xa;
                {
                    const int r0 = lane / UR;
                    const long long i = ib + u0 + lane % UR;
                    xa = cbdc_scaled(x[cbdc_idx((long long)r0 * kdim + i, r0 < m && i < i1)], r0 < m && i < i1, scx);
                }
                uint32_t bits[UR][E], sv[UR][E];
                sg_symbols<uint8_t, E, UR>(wl, cl, u0, lane, sym, nnz, bits, sv);
#pragma unroll
                for (int u = 0; u < UR; ++u) {
                    if (u0 + u >= nb) break;   // (uniform)
                    float xv[MT];
#pragma unroll
                    for (int r = 0; r < MT; ++r) xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xa), r * UR + u));
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        float d = 0.0f;
#pragma unroll
                        for (int r = 0; r < MT; ++r) d = __builtin_fmaf(xv[r], gv[r][e], d);   // dW'[i, o], r ascending (k_cbdc_stream)
                        const unsigned long long img = cbdc_fix(d, Sw);
                        if (bits[u][e]) {
                            if (sv[u][e] < (uint32_t)k) atomicAdd(&bins[(sv[u][e] << rlog2) + rep], img);
                        } else if (incol[e]) {
                            skip += img;
                        }
                    }
                }
            }
        }
        const uint32_t z = zsym[group];   // (uniform)
        if (z < (uint32_t)k && skip) atomicAdd(&bins[(z << rlog2) + rep], skip);
        skip = 0;
        cbdc_flush(bins, k, rlog2, sums + group * k);   // (begins with a barrier: every wave has left the group's rows)
        if (g_hi >= s_hi) break;                        // (the same test for the four waves)
        for (int j = threadIdx.x; j < k; j += CB_THREADS)   // the copies this thread has just summed
            for (int r = 0; r < (1 << rlog2); ++r) bins[(j << rlog2) + r] = 0ull;
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dc, m > 16
// k_cbspdc_tiled<uint8_t> with sums[groups][k]: the same grid, tiles and FMA order.  The k << rlog2 LDS bins are cut into
// 1 << sets_log2 sets of k << (rlog2 - sets_log2), set t for group m0 / group_rows + t (k_cbdc_tiled_grouped).  Thread (tx, ty) bins
// index rows m0 + ty * 8 .. + 7, which lie in one group, into that group's set; every set then goes into its group's sums.
__global__ __launch_bounds__(256) void k_cbspgdc_tiled(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                       const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo,
                                                       const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym, long long nnz, long long ncols,
                                                       long long segs, int k, const uint8_t *__restrict__ zsym, long long group_rows, int rlog2,
                                                       int sets_log2, int terms_log2, long long col_tiles, long long rows_per_split,
                                                       uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
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
    unsigned long long *mine = bins + ((long long)set * k << rl);
    const uint32_t z = q0 + set < groups ? (uint32_t)zsym[q0 + set] : (uint32_t)k;   // (rows past kdim: nothing is binned)
    const int rep = threadIdx.x & ((1 << rl) - 1);
    const long long ob = T.n0 + T.tx * 8, sg = ob >> 6;
    const int b0 = (int)(ob & 63);
    unsigned long long skip = 0;   // the images of the thread's skipped weights: bin z of its set
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const long long i = T.m0 + T.ty * 8 + a;
        if (i >= kdim || ob >= ncols) continue;
        const long long gi = i * segs;
        const uint64_t word = bitmap[gi + sg];
        long long pos = sp_count(lo[gi + sg], lo[gi], hi[i]) + __popcll(word & ((1ULL << b0) - 1));
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (ob + b >= ncols) continue;
            const unsigned long long img = cbdc_fix(acc[a][b], Sw);
            if ((word >> (b0 + b)) & 1) {
                const uint32_t l = pos < nnz ? (uint32_t)sym[pos] : z;   // (past nnz: skipped, as nnc_cbsp_grouped_unpack reads it)
                ++pos;
                if (l < (uint32_t)k) atomicAdd(&mine[(l << rl) + rep], img);
            } else {
                skip += img;
            }
        }
    }
    if (z < (uint32_t)k && skip) atomicAdd(&mine[(z << rl) + rep], skip);
    for (int t = 0; t < sets && q0 + t < groups; ++t) cbdc_flush(bins + ((long long)t * k << rl), k, rl, sums + (q0 + t) * k);   // (count: blockIdx alone)
}

// ------------------------------------------------------------------ launches
// (SpgForm, nnc_cbsp_grouped.hpp: the parts of the packed buffer and the group-wise operands every kernel takes)
template <int MT>
static void launch_sgg_dx(dim3 grid, size_t lds, hipStream_t s, const float *g, int m, long long kdim, const SpgForm &f, long long ncols, const float *centers,
                          int k, const SgPlan &p, int direct, float *out)
{
    hipLaunchKernelGGL((k_cbspgdx_stream<MT>), grid, dim3(CB_THREADS), lds, s, g, m, kdim, f.bitmap, f.lo, f.hi, f.sym, f.nnz, ncols, f.segs, centers, k, f.zsym,
                       f.group_rows, p.entries, p.cshift, p.rows_per_group, direct, out);
}

template <int MT>
static void launch_sgg_dc(dim3 grid, size_t lds, hipStream_t s, const float *x, const float *g, int m, long long kdim, const SpgForm &f, long long ncols, int k,
                          const SgPlan &p, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbspgdc_stream<MT>), grid, dim3(CB_THREADS), lds, s, x, g, m, kdim, f.bitmap, f.lo, f.hi, f.sym, f.nnz, ncols, f.segs, k, f.zsym,
                       f.group_rows, p.rlog2, p.terms_log2, p.rows_per_group, hdr, sums);
}

// every stream instantiation of this unit; the plans are checked against this table, and the launches go through it
using SggDxLaunch = void (*)(dim3, size_t, hipStream_t, const float *, int, long long, const SpgForm &, long long, const float *, int, const SgPlan &, int,
                             float *);
using SggDcLaunch = void (*)(dim3, size_t, hipStream_t, const float *, const float *, int, long long, const SpgForm &, long long, int, const SgPlan &,
                             uint32_t *, unsigned long long *);
struct SggCase {
    int a, vb, mt;            // a: 0 (uint8 symbols only); vb: 0 (a lane's columns are fixed by mt)
    SggDxLaunch dx;
    SggDcLaunch dc;
};
#define SGG_CASE(MT) {0, 0, MT, launch_sgg_dx<MT>, launch_sgg_dc<MT>}
static const SggCase kSggCases[] = {SGG_CASE(1), SGG_CASE(2), SGG_CASE(4), SGG_CASE(8), SGG_CASE(16)};
#undef SGG_CASE
static const CbgCaseNames kSggNames = {true, nullptr, false};

// ------------------------------------------------------------------ checks (host)
// sg_check's checks at label_bytes 1, then those the group-wise layers make of k and group_rows (the bins of dc included)
static int sgg_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (k > 256) return fail(NNC_EINVAL, std::string(fn) + ": k outside 1..256 (group codebooks take uint8 labels only)");
    const int rc = sg_check(fn, m, kdim, ncols, 1, k);
    if (rc != NNC_OK) return rc;
    return cb_check_group_rows(fn, kdim, group_rows, k);
}

// the form: nnz, the size and the alignment of the buffer, the skipped symbols
static int sgg_check_form(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int64_t nnz, const void *packed, int64_t packed_bytes,
                          const void *zero_symbols)
{
    const std::string f(fn);
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, f + ": nnz outside 0..kdim * ncols");
    if (packed_bytes < sp_layout(kdim, ncols, 1, nnz).bytes)
        return fail(NNC_EINVAL, f + ": packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz)");
    const bool product = m > 0 && kdim > 0 && ncols > 0;
    if (product && (!packed || !zero_symbols)) return fail(NNC_EINVAL, f + ": packed or zero_symbols is NULL");
    if (product && reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, f + ": packed must be 256-byte aligned");
    return NNC_OK;
}

// ------------------------------------------------------------------ C ABI
extern "C" int64_t nnc_cbsp_grouped_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols)
{
    if (sg_check("nnc_cbsp_grouped_dx_workspace_bytes", m, kdim, ncols, 1, 1) != NNC_OK) return 0;
    return sg_dx_ws_bytes(sg_dx_plan(m, kdim, ncols, 1, 1, CB_PLAN_CUS), m, kdim);
}

extern "C" int nnc_cbsp_grouped_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbsp_grouped_dx_plan";
    int rc = sgg_check(fn, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    const SgPlan p = sg_dx_plan(m, kdim, ncols, 1, k, cus);
    if ((rc = cbg_plan_out(fn, kSggCases, kSggNames, p.path, 0, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const bool tiled = p.path == NNC_CBMM_TILED;
    const int tables = tiled ? tile_groups(group_rows) : 0;
    const int64_t v[NNC_CBSPDX_PLAN_LEN] = {p.path, p.mt, p.segs, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries,
                                                    p.splits, p.per_split, p.lds + (tiled ? (long long)(tables - 1) * (k + 1) * 4 : 0), p.col_tiles,
                                                    p.row_tiles, sg_dx_ws_bytes(p, m, kdim)};
    for (int i = 0; i < NNC_CBSPDX_PLAN_LEN; ++i) out[i] = v[i];
    cbg_grouped_plan_tail(p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out + NNC_CBSPDX_PLAN_LEN);
    out[NNC_CBSPDX_GROUPED_P_TABLES] = tables;
    return NNC_OK;
}

extern "C" int nnc_cbsp_grouped_dx_f32(const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                                       const void *zero_symbols_dev, int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, float *dx,
                                       void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_dx_f32";
    int rc = sgg_check(fn, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = sgg_check_form(fn, m, kdim, ncols, nnz, packed, packed_bytes, zero_symbols_dev)) != NNC_OK) return rc;
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_f32: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_f32: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dx_f32: g is NULL");
    const int64_t need = nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_grouped_dx_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK)
        return rc;
    const SgPlan p = sg_dx_plan(m, kdim, ncols, 1, k, cu_count());
    const SggCase *sc;
    if ((rc = cbg_stream_case(fn, kSggCases, kSggNames, p.path, 0, 0, p.mt, sc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SpgForm f = spg_form(packed, sp_layout(kdim, ncols, 1, nnz), nnz, zero_symbols_dev, group_rows, centers_dev, k);
    float *rs = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sg_part_bytes(p, m, kdim));   // behind the partials
    // the row sums of g ahead of the kernel (one pass for every group), the rank-1 term behind the reduce, as nnc_cbsp_dx_f32
    rc = cbg_run_dx(p.path, p.splits, m, kdim, dx, workspace, s, [&](int direct, float *out) {
        const int rr = cbsp_rowsum(g, m, ncols, rs, s);
        if (rr != NNC_OK) return rr;
        if (p.path == NNC_CBMM_STREAM) {
            sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, f, ncols, centers_dev, k, p, direct, out);
            LAUNCHCHK("k_cbspgdx_stream");
        } else {
            const int tables = tile_groups(group_rows);
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            hipLaunchKernelGGL(k_cbspgdx_tiled, grid, dim3(256), (size_t)(p.lds + (long long)(tables - 1) * (k + 1) * 4), s, g, (long long)m, (long long)kdim,
                               f.bitmap, f.lo, f.hi, f.sym, (long long)nnz, (long long)ncols, f.segs, centers_dev, (int)k, f.zsym, (long long)group_rows, tables,
                               p.col_tiles, p.per_split, direct, out);
            LAUNCHCHK("k_cbspgdx_tiled");
        }
        return NNC_OK;
    });
    if (rc != NNC_OK || (p.path != NNC_CBMM_STREAM && p.path != NNC_CBMM_TILED)) return rc;   // (the rank-1 term only where the path wrote dx)
    const long long gx = std::min(cdiv(kdim, 256), 8192LL), gy = std::max(1LL, std::min((long long)m, 8192LL / gx));
    hipLaunchKernelGGL(k_cbspgdx_rank1, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, dx, (long long)m, (long long)kdim, rs, centers_dev, (int)k, f.zsym, (long long)group_rows);
    LAUNCHCHK("k_cbspgdx_rank1");
    return NNC_OK;
}

extern "C" int64_t nnc_cbsp_grouped_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (sgg_check("nnc_cbsp_grouped_dc_workspace_bytes", m, kdim, ncols, k, group_rows) != NNC_OK) return 0;
    SgPlan p;
    if (sg_dc_plan(m, kdim, ncols, 1, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return cbg_dc_ws_bytes(p.path, (int)(gg_groups(kdim, group_rows) * k));
}

extern "C" int nnc_cbsp_grouped_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbsp_grouped_dc_plan";
    int rc = sgg_check(fn, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    SgPlan p;
    if ((rc = sg_dc_plan(m, kdim, ncols, 1, k, cus, p)) != NNC_OK) return rc;
    if ((rc = cbg_plan_out(fn, kSggCases, kSggNames, p.path, 0, 0, p.mt, cus, out)) != NNC_OK) return rc;
    const int64_t v[NNC_CBSPDC_PLAN_LEN] = {p.path, p.mt, p.segs, p.path == NNC_CBMM_ZERO ? 0 : 1LL << p.rlog2, p.splits, p.per_split, p.lds,
                                                    p.col_tiles, p.row_tiles, p.terms_log2, cbg_dc_ws_bytes(p.path, (int)(gg_groups(kdim, group_rows) * k))};
    for (int i = 0; i < NNC_CBSPDC_PLAN_LEN; ++i) out[i] = v[i];
    cbg_grouped_plan_tail(p.path, p.row_tiles, p.rows_per_group, kdim, group_rows, out + NNC_CBSPDC_PLAN_LEN);
    return NNC_OK;
}

extern "C" int nnc_cbsp_grouped_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                                       const void *zero_symbols_dev, int64_t nnz, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace,
                                       int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_dc_f32";
    int rc = sgg_check(fn, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = sgg_check_form(fn, m, kdim, ncols, nnz, packed, packed_bytes, zero_symbols_dev)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dc_f32: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbsp_grouped_dc_f32: x or g is NULL");
    const int64_t need = nnc_cbsp_grouped_dc_workspace_bytes(m, kdim, ncols, k, group_rows);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_grouped_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK)
        return rc;
    SgPlan p;
    if ((rc = sg_dc_plan(m, kdim, ncols, 1, k, cu_count(), p)) != NNC_OK) return rc;
    const SggCase *sc;
    if ((rc = cbg_stream_case(fn, kSggCases, kSggNames, p.path, 0, 0, p.mt, sc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    const SpgForm f = spg_form(packed, sp_layout(kdim, ncols, 1, nnz), nnz, zero_symbols_dev, group_rows, nullptr, k);
    const int nbins = (int)(gg_groups(kdim, group_rows) * k);
    return cbg_run_dc(p.path, x, g, m, kdim, ncols, nbins, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, f, ncols, k, p, hdr, sums);
            LAUNCHCHK("k_cbspgdc_stream");
        } else {
            const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
            hipLaunchKernelGGL(k_cbspgdc_tiled, grid, dim3(256), (size_t)p.lds, s, x, g, (long long)m, (long long)kdim, f.bitmap, f.lo, f.hi, f.sym,
                               (long long)nnz, (long long)ncols, f.segs, (int)k, f.zsym, (long long)group_rows, p.rlog2,
                               __builtin_ctz(tile_groups(group_rows)), p.terms_log2, p.col_tiles, p.per_split, hdr, sums);
            LAUNCHCHK("k_cbspgdc_tiled");
        }
        return NNC_OK;
    });
}
