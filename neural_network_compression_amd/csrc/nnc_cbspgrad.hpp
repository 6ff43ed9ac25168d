// nnc_cbspgrad.hpp -- what the backward pass of the bitmap-sparse codebook matmul shares between its float32 unit (nnc_cbspgrad.hip,
// DESIGN.md section 13) and its bf16 / fp16 unit (nnc_cbspgrad_h16.hip, section 24): the plans of the float32 entry points (SgPlan,
// sg_dx_plan, sg_dc_plan), which the half unit follows field for field at m <= 16, the argument checks, the batch and symbol loads of
// the stream kernels, and the stream kernels themselves with the element type of g and x as a template parameter: XT = float is the
// float32 unit's kernel, XT = bf16_t / f16_t reads the operands as XT, widens them (exact) and runs the same float32 fmaf chain; the dx
// table is then built from the centres rounded to XT (sp_fill<XT>).
#pragma once
#include "nnc_cbgrad.hpp"
#include "nnc_cbsp.hpp"

// ------------------------------------------------------------------ plans (host)
struct SgPlan {
    int path;                 // NNC_CBMM_NONE / _STREAM / _TILED / _ZERO
    int mt, segs;             // stream: rows of m per launch (a power of two >= m), segments per column block
    int entries, cshift;      // dx: the LDS d table (entries x (1 << cshift) copies); tiled: k + 1 entries
    int rlog2;                // dc: 1 << rlog2 copies of every LDS bin
    long long col_tiles, row_tiles;   // stream: column blocks x row groups; tiled: tiles
    long long splits, per_split;      // dx: splits of ncols (columns per split); dc: splits of m (rows of m per split)
    long long rows_per_group;         // stream: index rows per workgroup
    int terms_log2;                   // dc: T of nnc_cbmm_dc_plan
    long long lds;
};

// segments per column block: at most 32 g values per lane
__host__ __device__ constexpr int sg_segs(int mt) { return mt <= 4 ? 8 : 32 / mt; }

static void sg_stream_grid(SgPlan &p, long long m, long long kdim, long long ncols, int cus)
{
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    p.path = NNC_CBMM_STREAM;
    p.mt = cb_mt(m);
    p.segs = sg_segs(p.mt);
    p.col_tiles = cdiv(cdiv(ncols, 64), p.segs);
    const long long batch = 64 / p.segs;   // index rows per batch of a wave
    const long long groups = std::max(1LL, std::min(cdiv(2LL * cus, p.col_tiles), cdiv(kdim, (long long)CB_WAVES * batch)));
    p.rows_per_group = cdiv(kdim, groups);
    p.row_tiles = cdiv(kdim, p.rows_per_group);
}

static SgPlan sg_dx_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus)
{
    SgPlan p{};
    if (m == 0 || kdim == 0) return p;                       // NNC_CBMM_NONE: dx is empty
    if (ncols == 0) {                                        // dx = 0
        p.path = NNC_CBMM_ZERO;
        return p;
    }
    if (m <= CB_SKINNY_M) {
        sg_stream_grid(p, m, kdim, ncols, cus);
        p.splits = p.col_tiles;                              // one split per column block
        p.per_split = 64LL * p.segs;
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
        p.per_split = cdiv(cdiv(ncols, s), 64) * 64;         // whole segments: a thread's 4 columns never straddle two words
        p.splits = cdiv(ncols, p.per_split);
        p.entries = k + 1;
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + k + 1) * 4 + TB_K * TB_N;
    }
    return p;
}

// the dx workspace: [partials: splits x m x kdim floats, when split, 256-byte aligned][row sums of g: m floats]
static long long sg_part_bytes(const SgPlan &p, long long m, long long kdim) { return p.splits > 1 ? (p.splits * m * kdim * 4 + 255) / 256 * 256 : 0; }
static int64_t sg_dx_ws_bytes(const SgPlan &p, long long m, long long kdim)
{
    return p.path == NNC_CBMM_STREAM || p.path == NNC_CBMM_TILED ? sg_part_bytes(p, m, kdim) + m * 4 : 0;
}

// The splits of m, the bin copies and T are nnc_cbmm_dc_plan's for the same shape (so S, every image and every sum are the dense
// call's).  NNC_OK, or that plan's error.
static int sg_dc_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus, SgPlan &p)
{
    p = SgPlan{};
    if (m == 0 || kdim == 0 || ncols == 0) {                 // no terms: dc = 0
        p.path = NNC_CBMM_ZERO;
        return NNC_OK;
    }
    int64_t d[NNC_CBDC_PLAN_LEN];
    const int rc = nnc_cbmm_dc_plan(m, kdim, ncols, lb, k, CB_PLAN_CUS, 0, d);
    if (rc != NNC_OK) return rc;
    p.splits = d[NNC_CBDC_P_SPLITS];
    p.per_split = d[NNC_CBDC_P_RPS];
    p.terms_log2 = (int)d[NNC_CBDC_P_TERMS_LOG2];
    p.rlog2 = __builtin_ctzll((unsigned long long)d[NNC_CBDC_P_COPIES]);
    const long long bins = ((long long)k << p.rlog2) * 8;
    if (m <= CB_SKINNY_M) {
        sg_stream_grid(p, m, kdim, ncols, cus);
        p.lds = bins;
    } else {
        p.path = NNC_CBMM_TILED;
        p.col_tiles = cdiv(ncols, TB_N);
        p.row_tiles = cdiv(kdim, TB_M);
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N) * 4 + bins;
    }
    return NNC_OK;
}

// ------------------------------------------------------------------ device helpers
// The words and counts of a batch of 64 / E rows x E segments: lane l holds those of row ib + l / E, segment blk * E + l % E
// (0 past the wave's rows or the matrix), broadcast later by v_readlane.
template <int E>
__device__ __forceinline__ void sg_batch(const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                         long long segs, long long blk, long long ib, long long i1, int lane, uint64_t &word, long long &cnt)
{
    const long long i = ib + lane / E, sg = blk * E + lane % E;
    word = 0;
    cnt = 0;
    if (i < i1 && sg < segs) {
        const long long gi = i * segs;
        word = bitmap[gi + sg];
        cnt = sp_count(lo[gi + sg], lo[gi], hi[i]);
    }
}

// lane `src`'s 64-bit value, on every lane
__device__ __forceinline__ uint64_t sg_bcast(uint64_t v, int src)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
}

// The UR rows u0 .. u0 + UR - 1 of a batch: per row and segment the lane's bit and its symbol (0 where the bit is clear).  A
// symbol past the nnz stored ones (a malformed form) counts as skipped, as nnc_cbsp_unpack reads it.  The symbol loads of the
// UR x E (row, segment) pairs are in flight together.
template <typename LT, int E, int UR>
__device__ __forceinline__ void sg_symbols(uint64_t wl, long long cl, int u0, int lane, const LT *__restrict__ sym, long long nnz, uint32_t (&bits)[UR][E],
                                           uint32_t (&sv)[UR][E])
{
#pragma unroll
    for (int u = 0; u < UR; ++u)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int src = (u0 + u) * E + e;
            const uint64_t word = sg_bcast(wl, src);
            const long long pos = (long long)sg_bcast((uint64_t)cl, src) + sp_rank(word);
            bits[u][e] = (uint32_t)(word >> lane) & 1u;
            sv[u][e] = 0;
            if (bits[u][e] && pos < nnz) sv[u][e] = sym[pos];
            else bits[u][e] = 0;
        }
}

// ------------------------------------------------------------------ dx, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  out: dx (one column block) or the float32 partials [block][m][kdim] (direct
// 0).  XT = float (nnc_cbsp_dx_f32, no RS): direct 1 stores the sums, the rank-1 term is k_cbspdx_rank1's afterwards.  XT = bf16_t /
// f16_t (nnc_cbsp_dx_h16) takes one more argument, RS = const float *, the row sums of g: a direct store adds c_z * rs[row] itself,
// exactly as k_cbspdx_rank1 adds it, before the one rounding of direct 2 (dx of XT; direct 1: float32).  The pack keeps the float32
// kernel's argument list, and so its instructions, what they were before the half type was added.
__device__ __forceinline__ const float *sg_rs() { return nullptr; }
__device__ __forceinline__ const float *sg_rs(const float *rs) { return rs; }

template <typename XT, typename LT, int MT, typename... RS>
__global__ __launch_bounds__(CB_THREADS) void k_cbspdx_stream(const XT *__restrict__ g, int m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                              const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const LT *__restrict__ sym,
                                                              long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                              int z, int entries, int cshift, long long rows_per_group, int direct,
                                                              void *__restrict__ out_, RS... rs_)
{
    constexpr bool HALF = !std::is_same<XT, float>::value;
    float *out = reinterpret_cast<float *>(out_);
    const float *rs = sg_rs(rs_...);
    constexpr int E = sg_segs(MT), RB = 64 / E, UR = E >= 8 ? 1 : 8 / E;   // segments per block, rows per batch, rows per step
    extern __shared__ float smem[];
    float *tab = smem;
    float *stage = smem + (entries << cshift);
    const float cz = sp_cz<XT>(centers, k, z);
    sp_fill<XT>(tab, stage, centers, k, cz, entries, cshift);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long blk = blockIdx.x;
    float gv[MT][E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const long long col = (blk * E + e) * 64 + lane;
#pragma unroll
        for (int r = 0; r < MT; ++r) gv[r][e] = (r < m && col < ncols) ? (float)g[(long long)r * ncols + col] : 0.0f;
    }

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    float *dst = direct ? out : out + blk * m * kdim;
    __syncthreads();

    uint64_t wn;
    long long cn;
    sg_batch<E>(bitmap, lo, hi, segs, blk, i0, i1, lane, wn, cn);
    for (long long ib = i0; ib < i1; ib += RB) {
        const uint64_t wl = wn;
        const long long cl = cn;
        if (ib + RB < i1) sg_batch<E>(bitmap, lo, hi, segs, blk, ib + RB, i1, lane, wn, cn);   // the next batch in flight
        const int nb = (int)std::min((long long)RB, i1 - ib);
        for (int u0 = 0; u0 < nb; u0 += UR) {
            uint32_t bits[UR][E], sv[UR][E];
            sg_symbols<LT, E, UR>(wl, cl, u0, lane, sym, nnz, bits, sv);
#pragma unroll
            for (int u = 0; u < UR; ++u) {
                float p[MT];
#pragma unroll
                for (int r = 0; r < MT; ++r) p[r] = 0.0f;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float dv = tab[CbTable<LT>::index(sv[u][e], k, cshift, lane)];
#pragma unroll
                    for (int r = 0; r < MT; ++r) p[r] = bits[u][e] ? __builtin_fmaf(gv[r][e], dv, p[r]) : p[r];   // skipped: no product
                }
                int row;
                const float v = wave_reduce_rows<MT>(p, lane, row);
                if (u0 + u < nb && (lane & (64 / MT - 1)) == 0 && row < m) {
                    const long long at = (long long)row * kdim + ib + u0 + u;
                    if (HALF && direct) {
                        const float t = cz != 0.0f ? cz * rs[row] + v : v;
                        if (direct == 2) reinterpret_cast<XT *>(out_)[at] = (XT)t;
                        else out[at] = t;
                    } else {
                        dst[at] = v;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------ dx += c_z * row sums of g (as sp_epilogue adds its rank-1 term)
// RT: the type c_z is rounded to (sp_cz)
template <typename RT = float>
__global__ __launch_bounds__(256) void k_cbspdx_rank1(float *__restrict__ dx, long long m, long long kdim, const float *__restrict__ rs,
                                                      const float *__restrict__ centers, int k, int z)
{
    const float cz = sp_cz<RT>(centers, k, z);
    if (cz == 0.0f) return;   // the rank-1 term is dropped (uniform over the launch)
    const long long mn = m * kdim;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < mn; idx += (long long)gridDim.x * blockDim.x)
        dx[idx] = cz * rs[idx / kdim] + dx[idx];
}

// ------------------------------------------------------------------ dc, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  LDS: the bins, [k][1 << rlog2] int64.  XT = bf16_t / f16_t
// (nnc_cbsp_dc_h16): x and g are widened as they are loaded and scaled in float32; the rest is the float32 kernel.
template <typename XT, typename LT, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbspdc_stream(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
                                                              const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo,
                                                              const uint32_t *__restrict__ hi, const LT *__restrict__ sym, long long nnz, long long ncols,
                                                              long long segs, int k, int z, int rlog2, int terms_log2, long long rows_per_group,
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

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    unsigned long long skip = 0;   // the images of the lane's skipped weights: bin z
    __syncthreads();

    uint64_t wn;
    long long cn;
    sg_batch<E>(bitmap, lo, hi, segs, blk, i0, i1, lane, wn, cn);
    for (long long ib = i0; ib < i1; ib += RB) {
        const uint64_t wl = wn;
        const long long cl = cn;
        if (ib + RB < i1) sg_batch<E>(bitmap, lo, hi, segs, blk, ib + RB, i1, lane, wn, cn);   // the next batch in flight
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
            sg_symbols<LT, E, UR>(wl, cl, u0, lane, sym, nnz, bits, sv);
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
    if (z < k && skip) atomicAdd(&bins[((uint32_t)z << rlog2) + rep], skip);
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ argument checks (host)
static int sg_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    const std::string f(fn);
    if (m < 0 || kdim < 0 || ncols < 0) return fail(NNC_EINVAL, f + ": negative size");
    if (label_bytes != 1 && label_bytes != 2) return fail(NNC_EINVAL, f + ": label_bytes must be 1 or 2");
    if (k < 1 || k > NNC_KMAX) return fail(NNC_EINVAL, f + ": k outside 1..NNC_KMAX");
    if (label_bytes == 1 && k > 256) return fail(NNC_EINVAL, f + ": k > 256 needs 2-byte labels");
    if (m > (1LL << 40) || !sp_size_ok(kdim, ncols))
        return fail(NNC_EINVAL, f + ": size too large (m <= 2^40, ncols < 2^32, kdim * ceil(ncols / 64) <= 2^40)");
    return NNC_OK;
}

// the arguments both calls share: the form (nnz, size, alignment), the skipped symbol
static int sg_check_form(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t z, int64_t nnz, const void *packed,
                         int64_t packed_bytes)
{
    int rc = sp_check_z(fn, z, label_bytes);
    if (rc != NNC_OK) return rc;
    const std::string f(fn);
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, f + ": nnz outside 0..kdim * ncols");
    if (packed_bytes < sp_layout(kdim, ncols, label_bytes, nnz).bytes)
        return fail(NNC_EINVAL, f + ": packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, label_bytes, nnz)");
    if (m > 0 && kdim > 0 && ncols > 0 && !packed) return fail(NNC_EINVAL, f + ": packed is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, f + ": packed must be 256-byte aligned");
    return NNC_OK;
}
