// nnc_cbsp_grouped.hip -- the pruned group-wise codebook layer run from the bitmap-sparse form of its indices
// (include/nnc_cbsp_grouped.h): one codebook per block of group_rows input rows (nnc_cbmm_grouped.hip, section
// 17) on the form of nnc_cbsp.hip (section 11), float32 x, uint8 labels.
//
// The buffer is section 11's at label_bytes 1.  The skipped symbol is one per group, z_g = zero_symbols[i / group_rows] for row i:
// bit (i, o) is set iff labels[i, o] != z_g.  The counts run through the whole matrix, so the groups are no separate buffers and the
// splits of the plan (sp_plan, nnc_cbsp.hpp: the ungrouped one for the same shape) do not follow them; the kernels walk from one
// group's rows into the next as the group-wise byte kernels do and change their d table on the way, d_g[s] = c_g[s] - c_{z_g}.
//
//     y[r, o] = t[r] + sum over stored (i, o) of x[r, i] * d_g(i)[label] (+ bias, ReLU),   t[r] = sum_g c_{z_g} * rs_g[r]
//
// Kernels of their own, not instantiations of a body shared with nnc_cbsp.hip: called through a device function the stream kernel
// compiles to another instruction stream (section 17).
//   k_cbspg_bits / k_cbspg_emit / k_cbspg_unpack   section 11's pack and unpack with z read per row (a wave's segment lies in one
//                    row: one uniform load per segment).  The two scans between bits and emit look at no label and are
//                    nnc_cbsp.hip's (cbsp_pack_scans).  No per-weight temporary.
//   k_cbspg_rowterm  t[r]: one workgroup per row walks the groups in order; rs_g as k_cbsp_rowsum sums a row, t from the first
//                    group with c_{z_g} != 0 on.  Also the word that says whether any group has one (`applies`).
//   k_cbspg_stream   m <= 16: k_cbsp_stream<float, uint8_t, MT> without the fused row sums, with k_cbmm_stream_grouped's walk: the
//                    split's rows go group by group, each stretch divided among the four waves, the d table refilled between two
//                    barriers at every boundary (the entries a label can reach, min(k + 1, 256) of them; the lookup clamps the
//                    label to the last).  A batch of SP_ROWS rows ends with its stretch.
//   k_cbspg_tiled    m > 16: k_cbsp_tiled<uint8_t> with two d tables in LDS, group g in slot g & 1; a TB_K step may lie across a
//                    boundary.  The tables hold k entries each; a stored label >= k (or a position past nnz) takes -c_{z_g} from
//                    global memory.  The kept mask of the masked step is read from the bitmap itself, so that the two tables
//                    fit into the LDS sp_plan reports for one table and a byte mask.
//   k_cbspg_combine  the split-K partials in k_cbsp_reduce's order, + t[r] where it applies, + bias, ReLU.
// No float atomics anywhere.
#include "nnc_cbsp.hpp"
#include "nnc_cbtile.hpp"

#define SPG_PLAN_LEN NNC_CBSP_GROUPED_PLAN_LEN

// c_{z_g}: 0 where z_g names no centre
__device__ __forceinline__ float spg_cz(const float *__restrict__ centers, int k, const uint8_t *__restrict__ zsym, long long g)
{
    return sp_cz(centers + g * k, k, (int)zsym[g]);
}

// t[r] + acc where t applies, + bias, ReLU (sp_epilogue with the rank-1 term already formed)
__device__ __forceinline__ float spg_epilogue(float acc, bool applies, float tr, const float *__restrict__ bias, long long c, int relu)
{
    float v = applies ? tr + acc : acc;
    if (bias) v += bias[c];
    if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
    return v;
}

// ------------------------------------------------------------------ pack / unpack
// one wave per segment (grid-stride): bitmap word by ballot, its popcount into lo
__global__ __launch_bounds__(256) void k_cbspg_bits(const uint8_t *__restrict__ labels, long long ncols, long long segs, long long g,
                                                    const uint8_t *__restrict__ zsym, long long group_rows, uint64_t *__restrict__ bitmap,
                                                    uint32_t *__restrict__ lo)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * 4;
    for (long long seg = (long long)blockIdx.x * 4 + wave; seg < g; seg += waves) {
        const long long i = seg / segs, c = (seg - i * segs) * 64 + lane;
        const uint32_t z = zsym[i / group_rows];
        const bool keep = c < ncols && (uint32_t)labels[i * ncols + c] != z;
        const uint64_t word = __ballot(keep);
        if (lane == 0) {
            bitmap[seg] = word;
            lo[seg] = (uint32_t)__popcll(word);
        }
    }
}

// one wave per segment: lo[g] becomes the low word of the global count; the symbols go to count + rank (only below `cap`)
__global__ __launch_bounds__(256) void k_cbspg_emit(const uint8_t *__restrict__ labels, long long ncols, long long segs, long long g,
                                                    const uint64_t *__restrict__ bitmap, uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                    uint8_t *__restrict__ sym, long long cap)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * 4;
    for (long long seg = (long long)blockIdx.x * 4 + wave; seg < g; seg += waves) {
        const long long i = seg / segs, s = seg - i * segs, c = s * 64 + lane;
        const uint64_t word = bitmap[seg];
        const uint32_t lo0 = lo[i * segs];
        const long long base = (long long)(((uint64_t)hi[i] << 32) | lo0) + (s > 0 ? (long long)lo[seg] : 0LL);
        if (s > 0 && lane == 0) lo[seg] = (uint32_t)base;   // segment 0 already holds it (read above by every wave of the row)
        if ((word >> lane) & 1) {
            const long long pos = base + sp_rank(word);
            if (pos < cap) sym[pos] = labels[i * ncols + c];
        }
    }
}

__global__ __launch_bounds__(256) void k_cbspg_unpack(const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                      const uint8_t *__restrict__ sym, long long nnz, long long ncols, long long segs, long long g,
                                                      const uint8_t *__restrict__ zsym, long long group_rows, uint8_t *__restrict__ labels)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * 4;
    for (long long seg = (long long)blockIdx.x * 4 + wave; seg < g; seg += waves) {
        const long long i = seg / segs, c = (seg - i * segs) * 64 + lane;
        if (c >= ncols) continue;
        const uint8_t z = zsym[i / group_rows];
        const uint64_t word = bitmap[seg];
        uint8_t v = z;
        if ((word >> lane) & 1) {
            const long long pos = sp_count(lo[seg], lo[i * segs], hi[i]) + sp_rank(word);
            v = pos < nnz ? sym[pos] : z;
        }
        labels[i * ncols + c] = v;
    }
}

// ------------------------------------------------------------------ the rank-1 term
// t[r] = sum over the groups with c_{z_g} != 0, in group order, of c_{z_g} * rs_g[r]; one workgroup per row (grid-stride).  rs_g
// is what k_cbsp_rowsum makes of a whole row: thread-strided sums by 256 from the group's first row, then the halving tree over the
// 256 threads (levels 128 .. 1).  t starts from the first term, not from 0.  *applies = 1 if a group has c_{z_g} != 0 (a NaN centre
// counts), else 0 (t is then 0 and unused).
// The same sums in fewer steps: the groups go in chunks of RT_CHUNK; the c_{z_g} of a chunk come in one parallel load; levels 32 .. 1
// of the tree run inside one wave by lane shifts (a lane below h adds the lane h above it: the value the tree adds there); thread 0
// then adds the chunk's terms in group order.  With four groups or more (or groups of at most 64 rows) a wave takes a group on its
// own, four groups in flight and no barrier: lane l keeps the sums of threads l, l + 64, l + 128 and l + 192 (v0 .. v3), level 128 is
// v0 + v2 and v1 + v3, level 64 their sum (threads past the group hold 0, and the additions of those zeros are written out: -0 + 0
// is +0).  With fewer and longer groups the 256 threads share a group as k_cbsp_rowsum shares a row.
#define RT_CHUNK 256
__device__ __forceinline__ float spg_wave_tree(float v, int lane)
{
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {
        const float o = __shfl_down(v, h);
        if (lane < h) v += o;
    }
    return v;   // lane 0: the sum
}

__global__ __launch_bounds__(256) void k_cbspg_rowterm(const float *__restrict__ x, long long m, long long kdim, const float *__restrict__ centers, int k,
                                                       const uint8_t *__restrict__ zsym, long long group_rows, long long groups, float *__restrict__ t,
                                                       uint32_t *__restrict__ applies)
{
    __shared__ float part[256], czs[RT_CHUNK], rss[RT_CHUNK];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long long r = blockIdx.x; r < m; r += gridDim.x) {
        const float *xr = x + r * kdim;
        float tv = 0.0f;
        bool any = false;
        for (long long c0 = 0; c0 < groups; c0 += RT_CHUNK) {
            const int nc = (int)std::min<long long>(RT_CHUNK, groups - c0);
            czs[threadIdx.x] = (int)threadIdx.x < nc ? spg_cz(centers, k, zsym, c0 + threadIdx.x) : 0.0f;
            __syncthreads();
            if (groups >= CB_WAVES || group_rows <= 64) {
                for (int j0 = wave; j0 < nc; j0 += 4 * CB_WAVES) {
                    float v[4][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {   // the loads of four groups in flight
                        const int j = j0 + q * CB_WAVES;
#pragma unroll
                        for (int w = 0; w < 4; ++w) v[q][w] = 0.0f;
                        if (j < nc && czs[j] != 0.0f) {
                            const long long g0 = (c0 + j) * group_rows, g1 = std::min(kdim, g0 + group_rows);
                            for (long long i = g0 + lane; i < g1; i += 256) {
#pragma unroll
                                for (int w = 0; w < 4; ++w)
                                    if (i + 64 * w < g1) v[q][w] += xr[i + 64 * w];
                            }
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = j0 + q * CB_WAVES;
                        const float s = spg_wave_tree((v[q][0] + v[q][2]) + (v[q][1] + v[q][3]), lane);
                        if (lane == 0 && j < nc) rss[j] = s;
                    }
                }
            } else {
                for (int j = 0; j < nc; ++j) {
                    if (!(czs[j] != 0.0f)) continue;   // uniform over the workgroup: the group adds nothing
                    const long long g0 = (c0 + j) * group_rows, g1 = std::min(kdim, g0 + group_rows);
                    float v = 0.0f;
                    for (long long i = g0 + threadIdx.x; i < g1; i += 256) v += xr[i];
                    part[threadIdx.x] = v;
                    __syncthreads();
                    if (threadIdx.x < 128) part[threadIdx.x] += part[threadIdx.x + 128];
                    __syncthreads();
                    if (wave == 0) {
                        const float s = spg_wave_tree(part[lane] + part[lane + 64], lane);
                        if (lane == 0) rss[j] = s;
                    }
                    __syncthreads();   // part is written again
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int j = 0; j < nc; ++j) {
                    const float cz = czs[j];
                    if (!(cz != 0.0f)) continue;
                    const float term = cz * rss[j];
                    tv = any ? tv + term : term;
                    any = true;
                }
            }
            __syncthreads();   // czs and rss are written again
        }
        if (threadIdx.x == 0) {
            t[r] = tv;
            if (r == 0) *applies = any ? 1u : 0u;
        }
    }
}

// ------------------------------------------------------------------ skinny: m <= 16
// grid (segments, splits), CB_THREADS threads; the LDS of k_cbsp_stream<float, uint8_t, MT>: the d table (entries << cshift), the
// waves' accumulators, the staging row.  out: y (direct != 0) or the float32 partials [split][m][ncols].
template <int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbspg_stream(const float *__restrict__ x, int m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                             const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym,
                                                             long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                             const uint8_t *__restrict__ zsym, long long group_rows, int entries, int cshift,
                                                             long long rows_per_split, const float *__restrict__ t, const uint32_t *__restrict__ applies,
                                                             const float *__restrict__ bias, int relu, int direct, float *__restrict__ out)
{
    constexpr int U = CB_UNROLL;
    extern __shared__ float smem[];
    float *tab = smem;
    float *red = smem + (entries << cshift);          // [MT][64] accumulators
    float *stage = red + MT * 65;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long seg = blockIdx.x;
    const long long col = seg * 64 + lane;
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    long long group = s_lo / group_rows;
    long long g_lo = s_lo, g_hi, i0, i1;   // the rows of the split that lie in `group`, and the wave's share of them
    cb_group_step(group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
    const int top = std::min(k, entries - 1);   // entry min(label, top): d of the label, or -c_{z_g} (k < 256: a label can pass k)
    sp_fill(tab, stage, centers + group * k, k, spg_cz(centers, k, zsym, group), top + 1, cshift);

    float acc[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) acc[r] = 0.0f;
    __syncthreads();

    for (;;) {
        for (long long ib = i0; ib < i1; ib += SP_ROWS) {
            // the words and counts of rows ib .. ib + 63, one row per lane (rows past i1: an empty word)
            const long long ir = ib + lane;
            uint64_t wl = 0;
            long long cl = 0;
            if (ir < i1) {
                const long long gi = ir * segs;
                wl = bitmap[gi + seg];
                cl = sp_count(lo[gi + seg], lo[gi], hi[ir]);
            }
            const uint32_t wlo = (uint32_t)wl, whi = (uint32_t)(wl >> 32), clo = (uint32_t)cl, chi = (uint32_t)((uint64_t)cl >> 32);
            const int nb = (int)std::min((long long)SP_ROWS, i1 - ib);
            for (int u0 = 0; u0 < nb; u0 += U) {
                const long long i = ib + u0;
                float xa, xb;
                {
                    const int f0 = lane, f1 = lane + 64, r0 = f0 / U, r1 = f1 / U;
                    xa = (r0 < m && i + f0 % U < i1) ? x[(long long)r0 * kdim + i + f0 % U] : 0.0f;
                    xb = (MT * U > 64 && r1 < m && i + f1 % U < i1) ? x[(long long)r1 * kdim + i + f1 % U] : 0.0f;
                }
                uint32_t bits[U], sv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {   // the symbol loads of U rows in flight together
                    const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)whi, u0 + u) << 32) |
                                          (uint32_t)__builtin_amdgcn_readlane((int)wlo, u0 + u);
                    const long long cnt = (long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)chi, u0 + u) << 32) |
                                                      (uint32_t)__builtin_amdgcn_readlane((int)clo, u0 + u));
                    bits[u] = (uint32_t)(word >> lane) & 1u;
                    const long long pos = cnt + sp_rank(word);
                    sv[u] = 0;
                    if (bits[u] && pos < nnz) sv[u] = sym[pos];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float wv = tab[CbTable<uint8_t>::index(std::min(sv[u], (uint32_t)top), k, cshift, lane)];
#pragma unroll
                    for (int r = 0; r < MT; ++r) {
                        const int f = r * U + u;
                        const float xv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
                        if (bits[u]) acc[r] = __builtin_fmaf(xv, wv, acc[r]);
                    }
                }
            }
        }
        if (g_hi >= s_hi) break;
        // on to the next group's rows, divided among the waves as a whole split is
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();   // every wave has left the rows of the group before
        sp_fill(tab, stage, centers + group * k, k, spg_cz(centers, k, zsym, group), top + 1, cshift);
        __syncthreads();
    }

    // the waves' sums, added to wave 0's in wave order
    for (int src = 1; src < CB_WAVES; ++src) {
        __syncthreads();
        if (wave == src) {
#pragma unroll
            for (int r = 0; r < MT; ++r) red[r * 64 + lane] = acc[r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < MT; ++r) acc[r] += red[r * 64 + lane];
        }
    }
    if (wave != 0 || col >= ncols) return;
    const bool app = direct && *applies != 0u;
#pragma unroll
    for (int r = 0; r < MT; ++r) {
        if (r >= m) continue;
        if (direct) out[(long long)r * ncols + col] = spg_epilogue(acc[r], app, app ? t[r] : 0.0f, bias, col, relu);
        else out[((long long)blockIdx.y * m + r) * ncols + col] = acc[r];
    }
}

// ------------------------------------------------------------------ tiled: m > 16
// grid (col_tiles * row_tiles, splits), 256 threads, as k_cbsp_tiled<uint8_t>: thread t decodes row t / 32 of the W tile, columns
// (t % 32) * 4 .. + 3.  A split can start off a multiple of TB_K, so a TB_K step can lie across a group boundary, in at most two
// groups (group_rows >= 32): LDS holds two d tables of k entries, group g in slot g & 1, handled as k_cbmm_tiled_grouped handles
// its two: the table of a step's last row is written ahead of the step's first barrier when it is not there yet; the slot it
// replaces was last read two groups earlier, before a barrier every thread has passed.
__global__ __launch_bounds__(256) void k_cbspg_tiled(const float *__restrict__ x, long long m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                     const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym,
                                                     long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                     const uint8_t *__restrict__ zsym, long long group_rows, long long col_tiles, long long rows_per_split,
                                                     const float *__restrict__ t, const uint32_t *__restrict__ applies, const float *__restrict__ bias,
                                                     int relu, int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // two tables of k entries: d of group g in slot g & 1
    auto table = [&](long long g) {
        float *slot = cb + (g & 1) * k;
        const float cz = spg_cz(centers, k, zsym, g);
        for (int j = threadIdx.x; j < k; j += 256) slot[j] = centers[g * k + j] - cz;
    };
    long long g_top = (long long)blockIdx.y * rows_per_split / group_rows;   // the last group whose table is in LDS
    table(g_top);

    const TbTile T = tb_tile(col_tiles, rows_per_split, kdim);
    float acc[8][8];
    tb_clear(acc);

    const int wk = threadIdx.x >> 5, wc = (threadIdx.x & 31) * 4;
    const long long gc = T.n0 + wc, gs = gc >> 6;
    const int b0 = (int)(gc & 63);
    const long long mc = T.n0 + T.tx * 8;   // the thread's 8 output columns: one byte of one bitmap word per row
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        if (std::min(kb + TB_K, T.hi) > (g_top + 1) * group_rows) table(++g_top);   // the step's last row opens a group
        __syncthreads();
        const int nonfinite = tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (gk < T.hi && gc < ncols) {
            const long long grp = gk >= g_top * group_rows ? g_top : g_top - 1;   // a step's rows lie in g_top - 1 and g_top
            const float *tab = cb + (grp & 1) * k;
            const long long gi = gk * segs;
            const uint64_t word = bitmap[gi + gs];
            long long pos = sp_count(lo[gi + gs], lo[gi], hi[gk]) + __popcll(word & ((1ULL << b0) - 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((word >> (b0 + j)) & 1) {
                    const uint32_t l = pos < nnz ? (uint32_t)sym[pos] : (uint32_t)k;
                    v[j] = l < (uint32_t)k ? tab[l] : 0.0f - spg_cz(centers, k, zsym, grp);
                    ++pos;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[wk * TB_N + wc + j] = v[j];
        // a skipped weight is absent: where the x tile holds an Inf or NaN the FMA must not form x * 0 at a skipped position
        // (rare, so the whole workgroup takes the masked step for that tile only; the mask is the bitmap's)
        if (__syncthreads_or(nonfinite)) {
            for (int kk = 0; kk < TB_K; ++kk) {
                const long long row = kb + kk;
                const uint32_t kept = (row < T.hi && mc < ncols) ? (uint32_t)(bitmap[row * segs + (mc >> 6)] >> (mc & 63)) & 0xFFu : 0u;
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    const float av = xs[kk * TB_M + T.ty * 8 + a];
#pragma unroll
                    for (int b = 0; b < 8; ++b)
                        if ((kept >> b) & 1u) acc[a][b] = __builtin_fmaf(av, ws[kk * TB_N + T.tx * 8 + b], acc[a][b]);
                }
            }
        } else {
            tb_tile_fma(xs, ws, T.tx, T.ty, acc);
        }
    }
    const bool app = direct && *applies != 0u;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const long long r = T.m0 + T.ty * 8 + a;
        if (r >= m) continue;
        const float tr = app ? t[r] : 0.0f;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const long long c = T.n0 + T.tx * 8 + b;
            if (c >= ncols) continue;
            if (direct) out[r * ncols + c] = spg_epilogue(acc[a][b], app, tr, bias, c, relu);
            else out[((long long)blockIdx.y * m + r) * ncols + c] = acc[a][b];
        }
    }
}

// ------------------------------------------------------------------ split-K combine
// the partials as k_cbsp_reduce sums them (four quarters of the splits in order, then the quarters in order), + t[r] where it
// applies, + bias, ReLU.  part == NULL (kdim = 0): y = bias; then t and applies are NULL too.
__global__ __launch_bounds__(256) void k_cbspg_combine(const float *__restrict__ part, long long splits, long long m, long long ncols,
                                                       const float *__restrict__ t, const uint32_t *__restrict__ applies, const float *__restrict__ bias,
                                                       int relu, float *__restrict__ y)
{
    __shared__ float qs[SP_RED_Q - 1][64];
    const long long mn = m * ncols;
    const bool app = applies && *applies != 0u;
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long per_q = (splits + SP_RED_Q - 1) / SP_RED_Q;
    const long long s0 = std::min(splits, q * per_q), s1 = std::min(splits, s0 + per_q);
    for (long long base = (long long)blockIdx.x * 64; base < mn; base += (long long)gridDim.x * 64) {
        const long long idx = base + o;
        float v = 0.0f;
        if (idx < mn) {
#pragma unroll 8
            for (long long s = s0; s < s1; ++s) v += part[s * mn + idx];
        }
        __syncthreads();
        if (q > 0) qs[q - 1][o] = v;
        __syncthreads();
        if (q == 0 && idx < mn) {
#pragma unroll
            for (int j = 0; j < SP_RED_Q - 1; ++j) v += qs[j][o];
            const long long r = idx / ncols;
            y[idx] = spg_epilogue(v, app, app ? t[r] : 0.0f, bias, idx - r * ncols, relu);
        }
    }
}

// ------------------------------------------------------------------ C ABI
static int spg_grid(long long g) { return (int)std::max(1LL, std::min(cdiv(g, 4), 65536LL)); }

static int spg_check_shape(const char *fn, int64_t kdim, int64_t ncols, int64_t group_rows)
{
    if (kdim < 0 || ncols < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (!sp_size_ok(kdim, ncols)) return fail(NNC_EINVAL, std::string(fn) + ": size too large (ncols < 2^32, kdim * ceil(ncols / 64) <= 2^40)");
    return cb_check_group_rows(fn, kdim, group_rows);
}

extern "C" int nnc_cbsp_grouped_pack(const void *labels, int64_t kdim, int64_t ncols, int64_t group_rows, const void *zero_symbols_dev, void *packed,
                                     int64_t packed_bytes, int64_t *nnz_dev, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_pack";
    int rc = spg_check_shape(fn, kdim, ncols, group_rows);
    if (rc != NNC_OK) return rc;
    const SpLayout L = sp_layout(kdim, ncols, 1, 0);
    if (packed_bytes < L.bytes) return fail(NNC_ENOSPACE, std::string(fn) + ": packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, 1, 0)");
    if (!packed && L.bytes > 0) return fail(NNC_EINVAL, std::string(fn) + ": packed is NULL");
    if (kdim > 0 && ncols > 0 && (!labels || !zero_symbols_dev)) return fail(NNC_EINVAL, std::string(fn) + ": labels or zero_symbols is NULL");
    if (reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, std::string(fn) + ": packed must be 256-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned char *base = reinterpret_cast<unsigned char *>(packed);
    uint64_t *bitmap = reinterpret_cast<uint64_t *>(base);
    uint32_t *lo = reinterpret_cast<uint32_t *>(base + L.off_lo), *hi = reinterpret_cast<uint32_t *>(base + L.off_hi);
    const long long cap = packed_bytes - L.off_sym;
    const uint8_t *lab = reinterpret_cast<const uint8_t *>(labels), *zs = reinterpret_cast<const uint8_t *>(zero_symbols_dev);
    if (L.g > 0) {
        hipLaunchKernelGGL(k_cbspg_bits, dim3(spg_grid(L.g)), dim3(256), 0, s, lab, (long long)ncols, L.segs, L.g, zs, (long long)group_rows, bitmap, lo);
        LAUNCHCHK("k_cbspg_bits");
    } else if (kdim > 0) {
        HIPCHK(hipMemsetAsync(hi, 0, (size_t)kdim * 4, s));   // ncols = 0: every row is empty
    }
    if ((rc = cbsp_pack_scans(kdim, L.segs, lo, hi, reinterpret_cast<long long *>(nnz_dev), s)) != NNC_OK) return rc;
    if (L.g > 0) {
        hipLaunchKernelGGL(k_cbspg_emit, dim3(spg_grid(L.g)), dim3(256), 0, s, lab, (long long)ncols, L.segs, L.g, bitmap, lo, hi, base + L.off_sym, cap);
        LAUNCHCHK("k_cbspg_emit");
    }
    return NNC_OK;
}

extern "C" int nnc_cbsp_grouped_unpack(const void *packed, int64_t packed_bytes, int64_t kdim, int64_t ncols, int64_t group_rows,
                                       const void *zero_symbols_dev, int64_t nnz, void *labels_out, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_unpack";
    int rc = spg_check_shape(fn, kdim, ncols, group_rows);
    if (rc != NNC_OK) return rc;
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, std::string(fn) + ": nnz outside 0..kdim * ncols");
    const SpLayout L = sp_layout(kdim, ncols, 1, nnz);
    if (packed_bytes < L.bytes) return fail(NNC_EINVAL, std::string(fn) + ": packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz)");
    if (kdim == 0 || ncols == 0) return NNC_OK;
    if (!packed || !labels_out || !zero_symbols_dev) return fail(NNC_EINVAL, std::string(fn) + ": packed, labels_out or zero_symbols is NULL");
    if (reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, std::string(fn) + ": packed must be 256-byte aligned");
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    hipLaunchKernelGGL(k_cbspg_unpack, dim3(spg_grid(L.g)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint64_t *>(base),
                       reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi), base + L.off_sym,
                       (long long)nnz, (long long)ncols, L.segs, L.g, reinterpret_cast<const uint8_t *>(zero_symbols_dev), (long long)group_rows,
                       reinterpret_cast<uint8_t *>(labels_out));
    LAUNCHCHK("k_cbspg_unpack");
    return NNC_OK;
}

static int spg_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (m < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (kdim < 0 || ncols < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (k < 1 || k > 256) return fail(NNC_EINVAL, std::string(fn) + ": k outside 1..256 (group codebooks take uint8 labels only)");
    const int rc = spg_check_shape(fn, kdim, ncols, group_rows);
    if (rc != NNC_OK) return rc;
    if (m > (1LL << 40)) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

// the workspace: [partials: splits x m x ncols floats, when split][t: m floats][applies: one 32-bit word], 256-byte aligned parts
static int64_t spg_ws_bytes(const SpPlan &p, long long m, long long ncols) { return sp_part_bytes(p, m, ncols) + m * 4 + 4; }

extern "C" int64_t nnc_cbsp_grouped_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || m > (1LL << 40) || !sp_size_ok(kdim, ncols)) return 0;
    return spg_ws_bytes(sp_plan(m, kdim, ncols, 1, 1, CB_PLAN_CUS), m, ncols);
}

template <int MT>
static void launch_spg_stream(dim3 grid, size_t lds, hipStream_t s, const float *x, int m, long long kdim, const unsigned char *base, const SpLayout &L,
                              long long nnz, long long ncols, const float *centers, int k, const uint8_t *zsym, long long group_rows, const SpPlan &p,
                              const float *t, const uint32_t *applies, const float *bias, int relu, int direct, float *out)
{
    hipLaunchKernelGGL((k_cbspg_stream<MT>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, reinterpret_cast<const uint64_t *>(base),
                       reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi),
                       reinterpret_cast<const uint8_t *>(base + L.off_sym), nnz, ncols, L.segs, centers, k, zsym, group_rows, p.entries, p.cshift,
                       p.rows_per_split, t, applies, bias, relu, direct, out);
}

// every k_cbspg_stream instantiation there is; the plan is checked against this table, and the launch goes through it
using SpgStreamLaunch = void (*)(dim3, size_t, hipStream_t, const float *, int, long long, const unsigned char *, const SpLayout &, long long, long long,
                                 const float *, int, const uint8_t *, long long, const SpPlan &, const float *, const uint32_t *, const float *, int, int,
                                 float *);
struct SpgStreamCase {
    int mt;
    SpgStreamLaunch fn;
};
static const SpgStreamCase kSpgStreamCases[] = {
    {1, launch_spg_stream<1>}, {2, launch_spg_stream<2>}, {4, launch_spg_stream<4>}, {8, launch_spg_stream<8>}, {16, launch_spg_stream<16>},
};

static SpgStreamLaunch find_spg_stream(int mt)
{
    for (const SpgStreamCase &c : kSpgStreamCases)
        if (c.mt == mt) return c.fn;
    return nullptr;
}

static int no_spg_stream_case(int mt) { return fail(NNC_EINVAL, "nnc_cbsp_grouped: no k_cbspg_stream instantiation for mt " + std::to_string(mt)); }

extern "C" int nnc_cbsp_grouped_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const int rc = spg_check("nnc_cbsp_grouped_plan", m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbsp_grouped_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbsp_grouped_plan: out is NULL");
    const SpPlan p = sp_plan(m, kdim, ncols, 1, k, cus);
    if (p.path == NNC_CBMM_STREAM && !find_spg_stream(p.mt)) return no_spg_stream_case(p.mt);
    const bool product = p.path == NNC_CBMM_STREAM || p.path == NNC_CBMM_TILED;
    const int64_t v[SPG_PLAN_LEN] = {p.path, p.mt, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries, p.splits, p.rows_per_split,
                                     product ? NNC_CBSP_ROWSUM_PASS : NNC_CBSP_ROWSUM_NONE, p.lds, p.col_tiles, p.row_tiles,
                                     product ? spg_ws_bytes(p, m, ncols) : 0, group_rows, kdim > 0 ? cdiv(kdim, group_rows) : 0,
                                     p.splits > 0 ? max_groups_per_split(p.splits, p.rows_per_split, kdim, group_rows) : 0};
    for (int i = 0; i < SPG_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbsp_grouped_f32(const float *x, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                                    const void *zero_symbols_dev, int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, const float *bias_dev,
                                    int32_t relu, float *y, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbsp_grouped_f32";
    int rc = spg_check(fn, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (nnz < 0 || nnz > kdim * ncols) return fail(NNC_EINVAL, std::string(fn) + ": nnz outside 0..kdim * ncols");
    const SpLayout L = sp_layout(kdim, ncols, 1, nnz);
    if (packed_bytes < L.bytes) return fail(NNC_EINVAL, std::string(fn) + ": packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz)");
    if (!centers_dev) return fail(NNC_EINVAL, std::string(fn) + ": centers is NULL");
    if (m > 0 && ncols > 0 && !y) return fail(NNC_EINVAL, std::string(fn) + ": y is NULL");
    const bool product = m > 0 && ncols > 0 && kdim > 0;
    if (product && (!x || !packed || !zero_symbols_dev)) return fail(NNC_EINVAL, std::string(fn) + ": x, packed or zero_symbols is NULL");
    if (product && reinterpret_cast<uintptr_t>(packed) % 256) return fail(NNC_EINVAL, std::string(fn) + ": packed must be 256-byte aligned");
    const int64_t need = nnc_cbsp_grouped_workspace_bytes(m, kdim, ncols);
    if ((rc = cb_check_workspace(fn, "nnc_cbsp_grouped_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK)
        return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const int rgrid = (int)std::max(1LL, std::min(cdiv(mn, 64), 8192LL));
    const SpPlan p = sp_plan(m, kdim, ncols, 1, k, cu_count());
    if (p.path == NNC_CBMM_BIAS) {   // kdim = 0: y = bias (zeros without one)
        hipLaunchKernelGGL(k_cbspg_combine, dim3(rgrid), dim3(256), 0, s, (const float *)nullptr, 0LL, (long long)m, (long long)ncols, (const float *)nullptr,
                           (const uint32_t *)nullptr, bias_dev, (int)relu, y);
        LAUNCHCHK("k_cbspg_combine");
        return NNC_OK;
    }
    const SpgStreamLaunch fn_stream = p.path == NNC_CBMM_STREAM ? find_spg_stream(p.mt) : nullptr;
    if (p.path == NNC_CBMM_STREAM && !fn_stream) return no_spg_stream_case(p.mt);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    const uint8_t *zs = reinterpret_cast<const uint8_t *>(zero_symbols_dev);
    const int direct = p.splits == 1;
    float *part = reinterpret_cast<float *>(workspace);
    float *t = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sp_part_bytes(p, m, ncols));
    uint32_t *applies = reinterpret_cast<uint32_t *>(t + m);
    float *out = direct ? y : part;
    hipLaunchKernelGGL(k_cbspg_rowterm, dim3((unsigned)std::min<long long>(m, 65536)), dim3(256), 0, s, x, (long long)m, (long long)kdim, centers_dev, (int)k, zs,
                       (long long)group_rows, cdiv(kdim, group_rows), t, applies);
    LAUNCHCHK("k_cbspg_rowterm");
    if (p.path == NNC_CBMM_STREAM) {
        fn_stream(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, base, L, nnz, ncols, centers_dev, k, zs, group_rows, p, t,
                  applies, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbspg_stream");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        hipLaunchKernelGGL(k_cbspg_tiled, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, reinterpret_cast<const uint64_t *>(base),
                           reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi),
                           reinterpret_cast<const uint8_t *>(base + L.off_sym), (long long)nnz, (long long)ncols, L.segs, centers_dev, (int)k, zs,
                           (long long)group_rows, p.col_tiles, p.rows_per_split, t, applies, bias_dev, (int)relu, direct, out);
        LAUNCHCHK("k_cbspg_tiled");
    }
    if (!direct) {
        hipLaunchKernelGGL(k_cbspg_combine, dim3(rgrid), dim3(256), 0, s, part, (long long)p.splits, (long long)m, (long long)ncols, t, applies, bias_dev,
                           (int)relu, y);
        LAUNCHCHK("k_cbspg_combine");
    }
    return NNC_OK;
}
