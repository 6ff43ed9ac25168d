// nnc_cbsp_grouped.hpp -- what the bitmap-sparse form of the group-wise codebook layer on float32 activations
// (nnc_cbsp_grouped.hip) shares with the same layer on bf16 / fp16 activations (nnc_cbsp_grouped_h16.hip,
// section 30): the m <= 16 path, templated on the type of x (and, where a kernel stores y, on the type of y), its launches, the
// argument checks and the workspace of that path.
//   k_cbspg_rowterm<XT>         t[r] = sum_g c_{z_g} * rs_g[r], and the word that says whether any group has c_{z_g} != 0
//   k_cbspg_stream<XT, YT, MT>  the stored weights' products, the d table refilled at every group boundary
//   k_cbspg_combine<YT>         the split-K partials, + t[r] where it applies, + bias, ReLU
// XT = float is nnc_cbsp_grouped_f32's kernel.  XT = bf16_t / f16_t: x is read as XT and widened (exact), every centre (c_{z_g} too)
// is rounded to XT (to nearest even) and widened before the difference that fills the d table and before the product with rs_g,
// and the arithmetic is the same float32 chain; YT = XT stores y with one rounding of the float32 value.
#pragma once
#include "nnc_cbsp.hpp"

// c_{z_g} (rounded to RT): 0 where z_g names no centre
template <typename RT = float>
__device__ __forceinline__ float spg_cz(const float *__restrict__ centers, int k, const uint8_t *__restrict__ zsym, long long g)
{
    return sp_cz<RT>(centers + g * k, k, (int)zsym[g]);
}

// t[r] + acc where t applies, + bias, ReLU (sp_epilogue with the rank-1 term already formed)
__device__ __forceinline__ float spg_epilogue(float acc, bool applies, float tr, const float *__restrict__ bias, long long c, int relu)
{
    float v = applies ? tr + acc : acc;
    if (bias) v += bias[c];
    if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
    return v;
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

template <typename XT>
__global__ __launch_bounds__(256) void k_cbspg_rowterm(const XT *__restrict__ x, long long m, long long kdim, const float *__restrict__ centers, int k,
                                                       const uint8_t *__restrict__ zsym, long long group_rows, long long groups, float *__restrict__ t,
                                                       uint32_t *__restrict__ applies)
{
    __shared__ float part[256], czs[RT_CHUNK], rss[RT_CHUNK];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long long r = blockIdx.x; r < m; r += gridDim.x) {
        const XT *xr = x + r * kdim;
        float tv = 0.0f;
        bool any = false;
        for (long long c0 = 0; c0 < groups; c0 += RT_CHUNK) {
            const int nc = (int)std::min<long long>(RT_CHUNK, groups - c0);
            czs[threadIdx.x] = (int)threadIdx.x < nc ? spg_cz<XT>(centers, k, zsym, c0 + threadIdx.x) : 0.0f;
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
                                    if (i + 64 * w < g1) v[q][w] += (float)xr[i + 64 * w];
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
                    for (long long i = g0 + threadIdx.x; i < g1; i += 256) v += (float)xr[i];
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
// grid (segments, splits), CB_THREADS threads; the LDS of k_cbsp_stream<XT, uint8_t, MT>: the d table (entries << cshift), the
// waves' accumulators, the staging row.  out: y as YT (direct != 0) or the float32 partials [split][m][ncols].
template <typename XT, typename YT, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbspg_stream(const XT *__restrict__ x, int m, long long kdim, const uint64_t *__restrict__ bitmap,
                                                             const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, const uint8_t *__restrict__ sym,
                                                             long long nnz, long long ncols, long long segs, const float *__restrict__ centers, int k,
                                                             const uint8_t *__restrict__ zsym, long long group_rows, int entries, int cshift,
                                                             long long rows_per_split, const float *__restrict__ t, const uint32_t *__restrict__ applies,
                                                             const float *__restrict__ bias, int relu, int direct, void *__restrict__ out_)
{
    constexpr int U = CB_UNROLL;
    extern __shared__ float smem[];
    float *tab = smem;
    float *red = smem + (entries << cshift);          // [MT][64] accumulators
    float *stage = red + MT * 65;
    float *out = reinterpret_cast<float *>(out_);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long seg = blockIdx.x;
    const long long col = seg * 64 + lane;
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    long long group = s_lo / group_rows;
    long long g_lo = s_lo, g_hi, i0, i1;   // the rows of the split that lie in `group`, and the wave's share of them
    cb_group_step(group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
    const int top = std::min(k, entries - 1);   // entry min(label, top): d of the label, or -c_{z_g} (k < 256: a label can pass k)
    sp_fill<XT>(tab, stage, centers + group * k, k, spg_cz<XT>(centers, k, zsym, group), top + 1, cshift);

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
                    xa = (r0 < m && i + f0 % U < i1) ? (float)x[(long long)r0 * kdim + i + f0 % U] : 0.0f;
                    xb = (MT * U > 64 && r1 < m && i + f1 % U < i1) ? (float)x[(long long)r1 * kdim + i + f1 % U] : 0.0f;
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
        sp_fill<XT>(tab, stage, centers + group * k, k, spg_cz<XT>(centers, k, zsym, group), top + 1, cshift);
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
        if (direct) {
            const float v = spg_epilogue(acc[r], app, app ? t[r] : 0.0f, bias, col, relu);
            if constexpr (std::is_same<YT, float>::value)
                out[(long long)r * ncols + col] = v;
            else
                reinterpret_cast<YT *>(out_)[(long long)r * ncols + col] = (YT)v;
        } else {
            out[((long long)blockIdx.y * m + r) * ncols + col] = acc[r];
        }
    }
}

// ------------------------------------------------------------------ split-K combine
// the partials as k_cbsp_reduce sums them (four quarters of the splits in order, then the quarters in order), + t[r] where it
// applies, + bias, ReLU, stored as YT.  part == NULL (kdim = 0): y = bias; then t and applies are NULL too.
template <typename YT>
__global__ __launch_bounds__(256) void k_cbspg_combine(const float *__restrict__ part, long long splits, long long m, long long ncols,
                                                       const float *__restrict__ t, const uint32_t *__restrict__ applies, const float *__restrict__ bias,
                                                       int relu, YT *__restrict__ y)
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
            y[idx] = (YT)spg_epilogue(v, app, app ? t[r] : 0.0f, bias, idx - r * ncols, relu);
        }
    }
}

// ------------------------------------------------------------------ host: checks, workspace, launches
static int spg_check_shape(const char *fn, int64_t kdim, int64_t ncols, int64_t group_rows)
{
    if (kdim < 0 || ncols < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (!sp_size_ok(kdim, ncols)) return fail(NNC_EINVAL, std::string(fn) + ": size too large (ncols < 2^32, kdim * ceil(ncols / 64) <= 2^40)");
    return cb_check_group_rows(fn, kdim, group_rows);
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

// the parts of the packed buffer and the group-wise operands every kernel of the m <= 16 path takes
struct SpgForm {
    const uint64_t *bitmap;
    const uint32_t *lo, *hi;
    const uint8_t *sym, *zsym;
    long long nnz, segs, group_rows;
    const float *centers;
    int k;
};

static inline SpgForm spg_form(const void *packed, const SpLayout &L, long long nnz, const void *zero_symbols, long long group_rows, const float *centers,
                               int k)
{
    const unsigned char *base = reinterpret_cast<const unsigned char *>(packed);
    return {reinterpret_cast<const uint64_t *>(base), reinterpret_cast<const uint32_t *>(base + L.off_lo), reinterpret_cast<const uint32_t *>(base + L.off_hi),
            reinterpret_cast<const uint8_t *>(base + L.off_sym), reinterpret_cast<const uint8_t *>(zero_symbols), nnz, L.segs, group_rows, centers, k};
}

template <typename XT>
static void launch_spg_rowterm(hipStream_t s, const void *x, long long m, long long kdim, const SpgForm &f, float *t, uint32_t *applies)
{
    hipLaunchKernelGGL((k_cbspg_rowterm<XT>), dim3((unsigned)std::min<long long>(m, 65536)), dim3(256), 0, s, reinterpret_cast<const XT *>(x), m, kdim,
                       f.centers, f.k, f.zsym, f.group_rows, cdiv(kdim, f.group_rows), t, applies);
}

// `direct` as cb_direct gives it: 0 the float32 partials, 1 y as float32, 2 y as XT
template <typename XT, int MT>
static void launch_spg_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, int m, long long kdim, const SpgForm &f, long long ncols, const SpPlan &p,
                              const float *t, const uint32_t *applies, const float *bias, int relu, int direct, void *out)
{
    auto kern = k_cbspg_stream<XT, float, MT>;
    if (!std::is_same<XT, float>::value && direct == 2) kern = k_cbspg_stream<XT, XT, MT>;
    hipLaunchKernelGGL(kern, grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), m, kdim, f.bitmap, f.lo, f.hi, f.sym, f.nnz, ncols, f.segs,
                       f.centers, f.k, f.zsym, f.group_rows, p.entries, p.cshift, p.rows_per_split, t, applies, bias, relu, direct, out);
}

// y as float32 (YT = float) or as YT
template <typename YT>
static void launch_spg_combine(hipStream_t s, const float *part, long long splits, long long m, long long ncols, const float *t, const uint32_t *applies,
                               const float *bias, int relu, void *y)
{
    const int rgrid = (int)std::max(1LL, std::min(cdiv(m * ncols, 64), 8192LL));
    hipLaunchKernelGGL((k_cbspg_combine<YT>), dim3(rgrid), dim3(256), 0, s, part, splits, m, ncols, t, applies, bias, relu, reinterpret_cast<YT *>(y));
}

// the instantiations of k_cbspg_stream for one type of x; a unit's plan is checked against its table, and its launch goes through it
using SpgStreamLaunch = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const SpgForm &, long long, const SpPlan &, const float *,
                                 const uint32_t *, const float *, int, int, void *);
struct SpgStreamCase {
    int dt, mt;
    SpgStreamLaunch fn;
};
#define SPG_STREAM_CASES(DT, XT)                                                                                                            \
    {DT, 1, launch_spg_stream<XT, 1>}, {DT, 2, launch_spg_stream<XT, 2>}, {DT, 4, launch_spg_stream<XT, 4>}, {DT, 8, launch_spg_stream<XT, 8>}, \
    {DT, 16, launch_spg_stream<XT, 16>}

// The m <= 16 call behind the argument checks (p: sp_plan's stream plan; workspace: spg_ws_bytes): the row term, the stream kernel
// `fn`, and the combine where the call is split.  NNC_OK or the launch error.
template <typename XT>
static int spg_run_stream(SpgStreamLaunch fn, const SpPlan &p, hipStream_t s, const void *x, long long m, long long kdim, const SpgForm &f, long long ncols,
                          const float *bias, int relu, void *y, int y_dtype, void *workspace)
{
    const int direct = cb_direct(p.splits, y_dtype);
    float *part = reinterpret_cast<float *>(workspace);
    float *t = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sp_part_bytes(p, m, ncols));
    uint32_t *applies = reinterpret_cast<uint32_t *>(t + m);
    launch_spg_rowterm<XT>(s, x, m, kdim, f, t, applies);
    LAUNCHCHK("k_cbspg_rowterm");
    fn(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, f, ncols, p, t, applies, bias, relu, direct,
       direct ? y : (void *)part);
    LAUNCHCHK("k_cbspg_stream");
    if (!direct) {
        (y_dtype == NNC_DT_F32 ? launch_spg_combine<float> : launch_spg_combine<XT>)(s, part, p.splits, m, ncols, t, applies, bias, relu, y);
        LAUNCHCHK("k_cbspg_combine");
    }
    return NNC_OK;
}
