// nnc_cbspgrad_grouped.hpp -- what the two backward units of the group-wise bitmap-sparse form share (nnc_cbspgrad_grouped.hip:
// float32; nnc_cbspgrad_grouped_h16.hip: bf16 / fp16 activations, section 35): the two stream kernels (m <= 16),
// templated on the element type of g and x as the ungrouped ones of nnc_cbspgrad.hpp are.  XT = float is nnc_cbsp_grouped_dx_f32's /
// nnc_cbsp_grouped_dc_f32's kernel, instruction for instruction what it was in nnc_cbspgrad_grouped.hip; XT = bf16_t / f16_t reads g and
// x as XT and widens them (exact), and the d tables of dx hold rn(c_q[s]) - rn(c_{z_q}), every centre rounded to XT (sp_fill<XT>).  The
// fmaf chains, the walk through the groups and the barriers do not depend on XT.  Both kernels write float32 (dx or its partials, the
// int64 sums); the rank-1 term and the one rounding of a half dx are k_cbspgdx_finish's (nnc_cbspgrad_grouped_h16.hip).
#pragma once
#include "nnc_cbspgrad.hpp"
#include "nnc_cbsp_grouped.hpp"

// ------------------------------------------------------------------ dx, m <= 16
// grid (column blocks, row groups), CB_THREADS threads; LDS as k_cbspdx_stream: the d table (entries << cshift), the staging row.
// out: dx (one column block) or the float32 partials [block][m][kdim] (direct 0).  rows_per_group is the workgroup's index rows (the
// plan's name), not group_rows.
template <typename XT, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbspgdx_stream(const XT *__restrict__ g, int m, long long kdim, const uint64_t *__restrict__ bitmap,
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
    sp_fill<XT>(tab, stage, centers + group * k, k, spg_cz<XT>(centers, k, zsym, group), top + 1, cshift);

    float gv[MT][E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const long long col = (blk * E + e) * 64 + lane;
#pragma unroll
        for (int r = 0; r < MT; ++r) gv[r][e] = (r < m && col < ncols) ? (float)g[(long long)r * ncols + col] : 0.0f;
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
        sp_fill<XT>(tab, stage, centers + group * k, k, spg_cz<XT>(centers, k, zsym, group), top + 1, cshift);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dc, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  LDS: one group's bins, [k][1 << rlog2] int64; sums[groups][k].
template <typename XT, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbspgdc_stream(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
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
        for (int r = 0; r < MT; ++r) gv[r][e] = (float)g[cbdc_idx((long long)r * ncols + col, r < m && incol[e])];
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
                    xa = cbdc_scaled((float)x[cbdc_idx((long long)r0 * kdim + i, r0 < m && i < i1)], r0 < m && i < i1, scx);
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
