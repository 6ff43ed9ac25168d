// nnc_cbwp_grouped.hip -- the group-wise codebook matmul on 5- and 6-bit split-plane ("wide packed") indices
// (include/nnc_cbwp_grouped.h): y = x @ W + bias, W[i, o] = centers[i / group_rows][label (i, o)], the labels in
// the split-plane form of nnc_cbwp.hip (the ordinary buffer of the whole row-major (kdim, ncols) index matrix), x float32, bf16 or
// fp16.  Inference only.
//
// The plan is the ungrouped one (wp_plan, nnc_cbwp.hpp) for the stream and the tiled kernel, and the MFMA grid of cb_grid
// (nnc_cbmm.hpp) for half x at m > 16, so the splits, the workspace and the summation order are those of nnc_cbwp (of
// nnc_cbmm_grouped for the MFMA tile).  As in sections 17 and 18 these are kernels of their own with the walk added, all templated on
// <BASE, PLANES> = <4, 1> (5 bits) and <4, 2> (6 bits):
//   k_cbwp_stream_grouped  m <= 16: k_cbwp_stream's geometry and decode with section 18's walk.  Every wave owns a table (2^bits
//                          entries x 32 per-bank copies: 4 or 8 KiB), walks its own rows group by group and rewrites its table at a
//                          boundary from the K centres it loaded, one per lane, while the stretch before ran: no workgroup barrier,
//                          no exposed load.
//   k_cbwp_tiled_grouped   m > 16, float32 x: k_cbwp_tiled with two tables in LDS, group g in slot g & 1 (a TB_K step may lie across
//                          a boundary).
//   k_cbwp_mfma_grouped    m > 16, bf16 / fp16 x: the tile and k loop of nnc_cbmfma.hpp, k_cbmm_mfma_grouped's walk.  The labels of
//                          a k step (32 index rows x 128 columns) are fetched with whole aligned words, 16 columns of one row per
//                          thread (8 bytes of the base part and 2 bytes of every plane: 2 or 3 loads a step where k_cbwp_mfma issues
//                          32 or 48), assembled to a byte each and handed through a 4 KiB label stage in LDS to the threads that own
//                          the columns of the W image.  On the same x and centres, the bits of nnc_cbmm_grouped on the unpacked labels.
// With one group the three kernels compute what k_cbwp_stream / k_cbwp_tiled / k_cbwp_mfma compute, bit for bit.
#include "nnc_cbwp.hpp"
#include "nnc_cbwp_grouped.h"
#include "nnc_cbmfma.hpp"
#include "nnc_cbtile.hpp"

#define WPG_CSHIFT 5              // 32 per-bank copies of a table of 32 or 64 entries (wp_cshift(5) = wp_cshift(6))
#define WPG_STAGE_BYTES (HM_BK * HM_BN)   // the label stage of the MFMA kernel: a byte per (row, column) of a k step

// ------------------------------------------------------------------ skinny: m <= 16
// grid (col_tiles, splits), CB_THREADS threads; `out` and `direct` as k_cbwp_stream (0: float32 partials, 1: float32 y, 2: y as XT).
// A split is divided among the four waves as k_cbwp_stream divides it.  A wave's rows are walked in stretches cut at the group's
// end, each a run of batches of U rows and then single rows, so a boundary inside a batch or a wave that starts inside a group
// needs nothing more; with one group these are the sums of k_cbwp_stream (a lane adds its rows in row order).  Everything that steers the walk (the
// wave's rows, the group, the stretch) is computed from blockIdx and the readfirstlane'd wave number: uniform, in SGPRs.  The
// lanes differ only in the centre they hold, picked by a clamped address and a select, never by a branch.
template <int BASE, int PLANES, int VB, int MT, typename XT>
__global__ __launch_bounds__(CB_THREADS) void k_cbwp_stream_grouped(const XT *__restrict__ x, int m, long long kdim, const unsigned char *__restrict__ packed,
                                                                    long long base_bytes, long long plane_bytes, long long ncols,
                                                                    const float *__restrict__ centers, int k, long long rows_per_split,
                                                                    long long group_rows, const float *__restrict__ bias, int relu, int direct,
                                                                    void *__restrict__ out_)
{
    constexpr int BITS = BASE + PLANES, E = 8 * VB / BASE, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BASE, ENTRIES = 1 << BITS;
    constexpr int COPIES = 1 << WPG_CSHIFT;
    constexpr int SH = WPG_CSHIFT + 2;                  // entry l of this lane's copy at byte l << SH
    constexpr uint32_t MASK = (1u << BASE) - 1;
    // rows in flight: k_cbwp_stream's, halved at 6 bits and 16 columns a lane, where the walk's registers on top of 8 rows of four
    // loads left one wave a SIMD.  A lane adds its rows in row order whatever the batch, so the sums do not depend on U.
    constexpr int U = (E >= 32 || (PLANES == 2 && E == 16)) ? 4 : CB_UNROLL;
    static_assert(E * MT <= PK_ACC && (E == 4 || E == 8 || E == 16 || E == 32), "columns per lane");
    static_assert(ENTRIES <= 64, "a wave's 64 lanes hold a table, one centre each");
    extern __shared__ float smem[];
    float *red = smem + CB_WAVES * ENTRIES * COPIES;    // [MT * E][64]
    float *out = reinterpret_cast<float *>(out_);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *cb = smem + wave * (ENTRIES * COPIES);       // this wave's table: [ENTRIES][COPIES]
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;                     // then the lane's VB base bytes and its plane bits lie inside the padded parts
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    const long long per_wave = (s_hi - s_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(s_hi, s_lo + wave * per_wave), i1 = std::min(s_hi, i0 + per_wave);
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *mine = packed + (active ? c0 * BASE / 8 : 0LL);
    const unsigned char *myplane = packed + base_bytes + (active ? c0 / 8 : 0LL);
    const char *tab = reinterpret_cast<const char *>(cb) + ((lane & (COPIES - 1)) << 2);

    float acc[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[r][e] = 0.0f;

    // lane j holds centre j of group g, rounded to XT as centers.to(dtype) does; 0 from k on (k <= 64 = the lanes of a wave)
    auto centre = [&](long long g) {
        const float c = centers[g * k + std::min(lane, k - 1)];
        return lane < k ? (float)(XT)c : 0.0f;
    };
    // the wave's table from the centres its lanes hold: word t * 64 + lane is copy lane & 31 of entry 2 t + (lane >> 5)
    auto fill = [&](float cv) {
#pragma unroll
        for (int t = 0; t < ENTRIES / 2; ++t) {
            const int lo = __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv), 2 * t);
            const int hi = __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv), 2 * t + 1);
            cb[t * 64 + lane] = __builtin_bit_cast(float, lane < 32 ? lo : hi);
            __builtin_amdgcn_sched_barrier(0);          // two broadcast values live at a time: read ahead, all 2^bits of them crowd the SGPRs
        }
        __builtin_amdgcn_wave_barrier();                // the lookups below read what other lanes of this wave wrote
    };
    auto load_row = [&](long long i, uint32_t *w, uint32_t *pl) {
        pk_load<VB>(mine + i * row_bytes, w);
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = wp_plane_load<E>(myplane + i * row_bytes + p * plane_bytes, lane);
    };
    auto load_x = [&](long long i, int U, float &xa, float &xb) { cb_load_x<MT>(x, kdim, m, lane, i, U, xa, xb); };
    auto consume = [&](const uint32_t *w, const uint32_t *pl, float xa, float xb, int u, int U) {
        float xv[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            const int f = r * U + u;
            xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            uint32_t a = wp_move(w[e / PER], BASE * (e % PER), SH, MASK);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) a |= wp_move(pl[p], e, SH + BASE + p, 1u);
            const float wv = *reinterpret_cast<const float *>(tab + a);
#pragma unroll
            for (int r = 0; r < MT; ++r) acc[r][e] = __builtin_fmaf(xv[r], wv, acc[r][e]);
        }
    };

    if (i0 < i1) {                                      // uniform over the wave
        long long group = i0 / group_rows;
        float cv = centre(group);
        long long i = i0;
        for (;;) {
            const long long e1 = std::min(i1, (group + 1) * group_rows);   // the end of the stretch: the group's or the wave's
            fill(cv);                                   // the lookups of the stretch before were issued ahead of these writes
            if (e1 < i1) cv = centre(group + 1);        // the next group's centres arrive while this stretch runs
            for (; i + U <= e1; i += U) {
                uint32_t w[U][N], pl[U][PLANES];
                float xa, xb;
#pragma unroll
                for (int u = 0; u < U; ++u) load_row(i + u, w[u], pl[u]);
                load_x(i, U, xa, xb);
#pragma unroll
                for (int u = 0; u < U; ++u) consume(w[u], pl[u], xa, xb, u, U);
            }
            for (; i < e1; ++i) {
                uint32_t w[N], pl[PLANES];
                float xa, xb;
                load_row(i, w, pl);
                load_x(i, 1, xa, xb);
                consume(w, pl, xa, xb, 0, 1);
            }
            if (e1 >= i1) break;
            ++group;
            __builtin_amdgcn_wave_barrier();            // the stretch's lookups stay ahead of the next fill
        }
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

// ------------------------------------------------------------------ tiled: m > 16, float32 x
// k_cbwp_tiled (nnc_cbwp.hip) with centers[groups][k]: the same grid, tile, decode and FMA order.  A split can start off a multiple
// of TB_K, so a TB_K step can lie across a boundary, in at most two groups (group_rows >= 32): LDS holds two tables of 2^bits
// entries, group g in slot g & 1, as k_cbpk_tiled_grouped holds them.  The table of a step's last row is written ahead of the
// step's first barrier when it is not there yet; the slot it replaces was last read two groups earlier, before a barrier every
// thread has passed.
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwp_tiled_grouped(const float *__restrict__ x, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                            long long base_bytes, long long plane_bytes, long long ncols,
                                                            const float *__restrict__ centers, int k, long long col_tiles, long long rows_per_split,
                                                            long long group_rows, const float *__restrict__ bias, int relu, int direct,
                                                            float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << (BASE + PLANES);
    constexpr uint32_t MASK = (1u << BASE) - 1;
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // two tables of 2^bits entries (zeros from k on)
    auto table = [&](long long g) {
        float *slot = cb + (g & 1) * ENTRIES;
        for (int j = threadIdx.x; j < ENTRIES; j += 256) slot[j] = j < k ? centers[g * k + j] : 0.0f;
    };
    long long g_top = (long long)blockIdx.y * rows_per_split / group_rows;   // the last group whose table is in LDS
    table(g_top);

    const TbTile T = tb_tile(col_tiles, rows_per_split, kdim);
    float acc[8][8];
    tb_clear(acc);

    const int wk = threadIdx.x >> 5, wc = (threadIdx.x & 31) * 4;      // W tile: k wk, columns wc..wc+3
    const long long c = T.n0 + wc, row_bytes = base_bytes + PLANES * plane_bytes;
    const long long wbyte = (c * BASE / 32) * 4, pbyte = base_bytes + (c / 32) * 4;
    const int wshift = (int)(c * BASE % 32), pshift = (int)(c % 32);
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        if (std::min(kb + TB_K, T.hi) > (g_top + 1) * group_rows) table(++g_top);   // the step's last row opens a group
        __syncthreads();
        tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
        const float *tab = cb + ((gk >= g_top * group_rows ? g_top : g_top - 1) & 1) * ENTRIES;   // a step's rows lie in g_top - 1 and g_top
        const bool live = gk < T.hi && c < ncols;       // c is a multiple of 4: then every dword below lies inside its padded part
        const unsigned char *row = packed + (live ? gk * row_bytes : 0LL);
        const uint32_t word = live ? *reinterpret_cast<const uint32_t *>(row + wbyte) >> wshift : 0u;
        uint32_t pl[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = live ? *reinterpret_cast<const uint32_t *>(row + pbyte + p * plane_bytes) >> pshift : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t l = (word >> (BASE * j)) & MASK;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) l |= ((pl[p] >> j) & 1u) << (BASE + p);
            ws[wk * TB_N + wc + j] = live ? tab[l] : 0.0f;
        }
        __syncthreads();
        tb_tile_fma(xs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_y(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, ncols, bias, relu, direct, out);
}

// ------------------------------------------------------------------ MFMA tile: m > 16, bf16 / fp16 x
// The 16 labels of columns c .. c + 15 of one index row, a byte each, label j in byte j % 4 of dword j / 4: the 16 base nibbles in
// `base` (column c at bit 0) spread to the low half of a byte each, bit j of plane p's 16 bits set at bit BASE + p of byte j.
template <int PLANES>
__device__ __forceinline__ uint4 wpg_labels16(uint2 base, const uint32_t (&pl)[PLANES])
{
    uint32_t d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t h = ((q < 2 ? base.x : base.y) >> (16 * (q & 1))) & 0xFFFFu;   // four nibbles
        uint32_t v = (h | (h << 8)) & 0x00FF00FFu;
        v = (v | (v << 4)) & 0x0F0F0F0Fu;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) {
            const uint32_t b = (pl[p] >> (4 * q)) & 0xFu;                             // four plane bits
            v |= ((b | (b << 7) | (b << 14) | (b << 21)) & 0x01010101u) << (4 + p);
        }
        d[q] = v;
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// grid (col_tiles * row_tiles, splits), HM_THREADS threads: k_cbmm_mfma_grouped (nnc_cbmm_grouped.hip) with the labels taken from the
// split-plane rows: the same grid, the same tile and k loop (nnc_cbmfma.hpp, the refill as hm_accumulate's `open`), the per-bank table
// of 2^bits entries (the centres rounded to XT, zeros from k on).  Splits start on whole k steps of HM_BK = 32 and group_rows is a
// multiple of 32, so a step lies in one group; a step that opens a group rewrites the first k table entries ahead of its first
// barrier: the lookups of the step before ended at that step's second barrier.
// The labels of a step travel in two hops.  Thread t fetches (load_w, one step ahead of the MFMAs) columns n0 + (t % 8) * 16 .. + 15
// of index row kb + t / 8: 8 bytes of the base part and 2 bytes of every plane, each naturally aligned and, when the first of the 16
// columns is < ncols, inside the padded parts; a row past k_hi or columns past ncols load nothing and stage label 0.  open(kb)
// assembles the 16 labels and writes them as one 16-byte store to the stage `labs` [row][column] (thread t at byte 16 t: linear, no
// bank conflict) in front of the step's first barrier.  Between the two barriers store_w(kb) reads, as the owner of column wc and rows
// wk0 .. wk0 + 15 of the W image, its 16 labels with byte reads (a wave reads 64 consecutive bytes of one stage row: 16 banks, four
// lanes on a dword) and looks them up (hm_lookup_w: zero past k_hi and past ncols, never the table).  The next write of the stage
// comes after the second barrier, so the loop's own two barriers order it.
template <int BASE, int PLANES, typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbwp_mfma_grouped(const XT *__restrict__ x, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                                  long long base_bytes, long long plane_bytes, long long ncols,
                                                                  const float *__restrict__ centers, int k, long long col_tiles, long long rows_per_split,
                                                                  long long group_rows, const float *__restrict__ bias, int relu, int direct,
                                                                  void *__restrict__ out_)
{
    static_assert(BASE == 4 && HM_BK * 8 == HM_THREADS && HM_BN == 128, "a thread stages 16 columns of one of the 32 rows of a k step");
    constexpr int ENTRIES = 1 << (BASE + PLANES);
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, ENTRIES, WPG_CSHIFT);   // the table: [ENTRIES][32 copies]
    unsigned char *labs = reinterpret_cast<unsigned char *>(L.ws + HM_BN * HM_LD);   // [HM_BK][HM_BN] labels of the step
    long long group = (long long)blockIdx.y * rows_per_split / group_rows;
    cb_fill<XT>(L.cb, L.stage, centers + group * k, k, ENTRIES, WPG_CSHIFT);

    const HmTile T = hm_tile(col_tiles, rows_per_split, kdim);
    const bool col_ok = T.n0 + T.wc < ncols;            // the thread's column of the W image exists
    const int sr = T.t >> 3, sc = (T.t & 7) * 16;       // the thread's row and first column of the stage
    const long long gc16 = T.n0 + sc, row_bytes = base_bytes + PLANES * plane_bytes;
    const bool cols_ok = gc16 < ncols;                  // gc16 is a multiple of 16: then the loads below lie inside the padded parts
    const unsigned char *brow = packed + (cols_ok ? gc16 / 2 : 0LL), *prow = packed + base_bytes + (cols_ok ? gc16 / 8 : 0LL);
    uint2 bw;
    uint32_t pw[PLANES];

    auto load_w = [&](long long kb) {
        const long long gk = kb + sr;
        const bool live = cols_ok && gk < T.k_hi;
        bw = live ? *reinterpret_cast<const uint2 *>(brow + gk * row_bytes) : make_uint2(0u, 0u);
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pw[p] = live ? (uint32_t)*reinterpret_cast<const uint16_t *>(prow + gk * row_bytes + p * plane_bytes) : 0u;
    };
    auto open = [&](long long kb) {
        if (kb >= (group + 1) * group_rows) cb_refill<XT>(L.cb, centers + ++group * k, k, WPG_CSHIFT);   // this step opens a group
        *reinterpret_cast<uint4 *>(labs + sr * HM_BN + sc) = wpg_labels16<PLANES>(bw, pw);
    };
    auto store_w = [&](long long kb) {
        uint32_t lab[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) lab[j] = labs[(T.wk0 + j) * HM_BN + T.wc];
        hm_lookup_w(L.ws, L.cb, T, col_ok, kb, lab, [&](uint32_t l) { return (l << WPG_CSHIFT) | (T.lane & ((1 << WPG_CSHIFT) - 1)); });
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(x, m, kdim, T, L.xs, L.ws, acc, load_w, store_w, HmNothing(), open);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, ncols, bias, relu, direct, out_);
}

// ------------------------------------------------------------------ launches
template <int BASE, int PLANES, int VB, int MT, typename XT>
static void launch_wpg_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, int m, long long kdim, const unsigned char *packed, long long base_bytes,
                              long long plane_bytes, long long ncols, const float *centers, int k, long long rps, long long group_rows, const float *bias,
                              int relu, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbwp_stream_grouped<BASE, PLANES, VB, MT, XT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), m, kdim, packed,
                       base_bytes, plane_bytes, ncols, centers, k, rps, group_rows, bias, relu, direct, out);
}

template <int BASE, int PLANES>
static void launch_wpg_tiled(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const unsigned char *packed, long long base_bytes,
                             long long plane_bytes, long long ncols, const float *centers, int k, long long col_tiles, long long rps, long long group_rows,
                             const float *bias, int relu, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbwp_tiled_grouped<BASE, PLANES>), grid, dim3(256), lds, s, reinterpret_cast<const float *>(x), m, kdim, packed, base_bytes,
                       plane_bytes, ncols, centers, k, col_tiles, rps, group_rows, bias, relu, direct, reinterpret_cast<float *>(out));
}

template <int BASE, int PLANES, typename XT>
static void launch_wpg_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const unsigned char *packed, long long base_bytes,
                            long long plane_bytes, long long ncols, const float *centers, int k, long long col_tiles, long long rps, long long group_rows,
                            const float *bias, int relu, int direct, void *out)
{
    hm_launch(x, kdim, k_cbwp_mfma_grouped<BASE, PLANES, XT, true>, k_cbwp_mfma_grouped<BASE, PLANES, XT, false>, grid, lds, s,
              reinterpret_cast<const XT *>(x), m, kdim, packed, base_bytes, plane_bytes, ncols, centers, k, col_tiles, rps, group_rows, bias, relu, direct, out);
}

// every instantiation of this unit: wp_plan's (VB, MT) pairs at base 4 for each width and type of x, and the tiles.  The plan is
// checked against these tables, and the launches go through them.
using WpgStreamLaunch = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const unsigned char *, long long, long long, long long, const float *,
                                 int, long long, long long, const float *, int, int, void *);
using WpgTileLaunch = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const unsigned char *, long long, long long, long long,
                               const float *, int, long long, long long, long long, const float *, int, int, void *);
struct WpgStreamCase {
    int dt, bits, vb, mt;
    WpgStreamLaunch fn;
};
struct WpgTileCase {
    int dt, bits;
    WpgTileLaunch fn;
};
#define WPG_CASE(DT, XT, P, V, M) {DT, 4 + P, V, M, launch_wpg_stream<4, P, V, M, XT>}
#define WPG_CASES(DT, XT, P)                                                                                                              \
    WPG_CASE(DT, XT, P, 16, 1), WPG_CASE(DT, XT, P, 16, 2), WPG_CASE(DT, XT, P, 8, 1), WPG_CASE(DT, XT, P, 8, 2), WPG_CASE(DT, XT, P, 8, 4), \
    WPG_CASE(DT, XT, P, 4, 1), WPG_CASE(DT, XT, P, 4, 2), WPG_CASE(DT, XT, P, 4, 4), WPG_CASE(DT, XT, P, 4, 8), WPG_CASE(DT, XT, P, 2, 16)
#define WPG_STREAM_CASES(DT, XT) WPG_CASES(DT, XT, 1), WPG_CASES(DT, XT, 2)
static const WpgStreamCase kWpgStreamCases[] = {WPG_STREAM_CASES(NNC_DT_F32, float), WPG_STREAM_CASES(NNC_DT_BF16, bf16_t), WPG_STREAM_CASES(NNC_DT_F16, f16_t)};
static const WpgTileCase kWpgTileCases[] = {
    {NNC_DT_F32, 5, launch_wpg_tiled<4, 1>},         {NNC_DT_F32, 6, launch_wpg_tiled<4, 2>},
    {NNC_DT_BF16, 5, launch_wpg_mfma<4, 1, bf16_t>}, {NNC_DT_BF16, 6, launch_wpg_mfma<4, 2, bf16_t>},
    {NNC_DT_F16, 5, launch_wpg_mfma<4, 1, f16_t>},   {NNC_DT_F16, 6, launch_wpg_mfma<4, 2, f16_t>},
};

// the launch of plan p for x of type dt; false after NNC_EINVAL was recorded: a plan with no instantiation
static bool wpg_find(const char *fn, const WpPlan &p, int dt, int bits, WpgStreamLaunch &stream, WpgTileLaunch &tile)
{
    stream = nullptr, tile = nullptr;
    if (p.path == NNC_CBMM_STREAM) {
        for (const WpgStreamCase &c : kWpgStreamCases)
            if (c.dt == dt && c.bits == bits && c.vb == p.vb && c.mt == p.mt) stream = c.fn;
    } else if (p.path == NNC_CBMM_TILED || p.path == NNC_CBMM_MFMA) {
        for (const WpgTileCase &c : kWpgTileCases)
            if (c.dt == dt && c.bits == bits) tile = c.fn;
    } else {
        return true;
    }
    if (stream || tile) return true;
    fail(NNC_EINVAL, std::string(fn) + ": no kernel instantiation for dtype " + std::to_string(dt) + ", bits " + std::to_string(bits) + ", vb " +
                         std::to_string(p.vb) + ", mt " + std::to_string(p.mt));
    return false;
}

// ------------------------------------------------------------------ the plan (host)
struct WpgPlan {
    WpPlan p;      // wp_plan's: path, vb, mt, cols, tiles, splits, rps; lds and copies those of the grouped kernels
    int tables;    // tables held in LDS: one per wave (stream), two (tiled), one (MFMA)
};

static WpgPlan wpg_plan(int x_dtype, long long m, long long kdim, long long ncols, int bits, int cus)
{
    WpgPlan g{wp_plan(x_dtype, m, kdim, ncols, bits, cus), 0};
    WpPlan &p = g.p;
    if (p.path == NNC_CBMM_STREAM) {
        g.tables = CB_WAVES;
        p.copies = 1 << WPG_CSHIFT;
        p.lds = ((long long)CB_WAVES * p.entries * p.copies + (long long)p.mt * p.cols * 64) * 4;
    } else if (p.path == NNC_CBMM_TILED) {
        g.tables = 2;
        p.lds += (long long)p.entries * 4;   // the second table
    } else if (p.path == NNC_CBMM_MFMA) {    // wp_plan took cb_grid's MFMA grid, which is nnc_cbmm_grouped's
        g.tables = 1;
        p.copies = 1 << WPG_CSHIFT;
        p.lds = (long long)hm_table_words(p.entries, WPG_CSHIFT) * 4 + (long long)(HM_BM + HM_BN) * HM_LD * 2 + WPG_STAGE_BYTES;
    }
    return g;
}

// ------------------------------------------------------------------ C ABI (wpg_check: nnc_cbwp.hpp)
extern "C" int64_t nnc_cbwp_grouped_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || wpg_check("nnc_cbwp_grouped_workspace_bytes", x_dtype, m, kdim, ncols, bits, 17, 32) != NNC_OK) return 0;
    return wp_ws_bytes(wpg_plan(x_dtype, m, kdim, ncols, bits, CB_PLAN_CUS).p, m, ncols);
}

extern "C" int nnc_cbwp_grouped_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    const int rc = wpg_check("nnc_cbwp_grouped_plan", x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbwp_grouped_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbwp_grouped_plan: out is NULL");
    const WpgPlan g = wpg_plan(x_dtype, m, kdim, ncols, bits, cus);
    const WpPlan &p = g.p;
    WpgStreamLaunch sf;
    WpgTileLaunch tf;
    if (!wpg_find("nnc_cbwp_grouped_plan", p, x_dtype, bits, sf, tf)) return NNC_EINVAL;
    const int64_t v[NNC_CBWP_GROUPED_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.base, p.planes, p.copies, p.entries, p.splits, p.rows_per_split, p.lds,
                                                  p.col_tiles, p.row_tiles, wp_ws_bytes(p, m, ncols), x_dtype, group_rows,
                                                  kdim > 0 ? cdiv(kdim, group_rows) : 0,
                                                  p.splits > 0 ? max_groups_per_split(p.splits, p.rows_per_split, kdim, group_rows) : 0, g.tables};
    for (int i = 0; i < NNC_CBWP_GROUPED_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbwp_grouped(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                                const float *centers_dev, int32_t k, int64_t group_rows, const float *bias_dev, int32_t relu, void *y, int y_dtype,
                                void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = wpg_check("nnc_cbwp_grouped", x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_buffer("nnc_cbwp_grouped", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if ((rc = cb_check_operands("nnc_cbwp_grouped", x, x_dtype, y, y_dtype, centers_dev, m, kdim, ncols, !x, "x")) != NNC_OK) return rc;
    const int64_t need = nnc_cbwp_grouped_workspace_bytes(x_dtype, m, kdim, ncols, bits);
    if ((rc = cb_check_workspace("nnc_cbwp_grouped", "nnc_cbwp_grouped_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) !=
        NNC_OK)
        return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = S(stream);
    const long long mn = m * ncols;
    const WpPlan p = wpg_plan(x_dtype, m, kdim, ncols, bits, cu_count()).p;
    if (p.path == NNC_CBMM_BIAS) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // kdim = 0: y = bias
    WpgStreamLaunch sf;
    WpgTileLaunch tf;
    if (!wpg_find("nnc_cbwp_grouped", p, x_dtype, bits, sf, tf)) return NNC_EINVAL;
    const int direct = cb_direct(p.splits, y_dtype);
    void *out = direct ? y : workspace;
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long bb = wp_base_bytes(ncols, bits), pb = wp_plane_bytes(ncols);
    if (sf) {
        sf(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, pk, bb, pb, ncols, centers_dev, k, p.rows_per_split, group_rows,
           bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbwp_stream_grouped");
    } else {
        tf(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, m, kdim, pk, bb, pb, ncols, centers_dev, k, p.col_tiles,
           p.rows_per_split, group_rows, bias_dev, relu, direct, out);
        LAUNCHCHK((p.path == NNC_CBMM_MFMA ? "k_cbwp_mfma_grouped" : "k_cbwp_tiled_grouped"));
    }
    return cb_finish(direct, workspace, p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
}
