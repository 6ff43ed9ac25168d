// nnc_cbpk_grouped.hip -- the group-wise codebook matmul on 2- and 4-bit packed indices (include/nnc.h, nnc_cbpk_grouped; DESIGN.md
// section 18): y = x @ W + bias, W[i, o] = centers[i / group_rows][label (i, o)], the labels in the packed form of nnc_cbpk.hip (the
// ordinary packed buffer of the whole row-major (kdim, ncols) index matrix), x float32, bf16 or fp16.
//
// The plan is the ungrouped packed one (pk_plan, nnc_cbpk.hpp) for the stream and the tiled kernel, and the MFMA grid of cb_grid
// (nnc_cbmm.hpp) for half x at m > 16, so the splits, the workspace and the summation order are those of nnc_cbpk_f32 (of
// nnc_cbmm_grouped for the MFMA tile).  The stream kernel is a copy of its ungrouped counterpart with the walk through the groups
// added, not an instantiation of a shared body (DESIGN.md section 17 records why); the tiled one is the tile skeleton of
// nnc_cbtile.hpp, the MFMA one the tile of nnc_cbmfma.hpp, each around its own tables, label decode and group walk:
//   k_cbpk_stream_grouped  m <= 16: k_cbpk_stream with x of type XT.  Every wave owns a table (2^BITS entries x 32 per-bank copies:
//                          2 KiB or 512 B), walks its own rows group by group and rewrites its table at a boundary from the K
//                          centres it loaded, one per lane, while the stretch before ran: no workgroup barrier, no exposed load.
//   k_cbpk_tiled_grouped   m > 16, float32 x: k_cbpk_tiled with two tables in LDS, group g in slot g & 1 (a TB_K step may lie
//                          across a boundary).
//   k_cbpk_mfma_grouped    m > 16, bf16 / fp16 x: k_cbmm_mfma_grouped's walk and the shared tile, the label of (gk, gc) taken from
//                          the packed row: on the same x and centres, the bits of nnc_cbmm_grouped on the unpacked labels.
// With one group the stream and the tiled kernel compute what k_cbpk_stream / k_cbpk_tiled compute, bit for bit.
#include "nnc_cbpk.hpp"
#include "nnc_cbmfma.hpp"
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ skinny: m <= 16
// grid (col_tiles, splits), CB_THREADS threads; `out` and `direct` as k_cbmm_stream (0: float32 partials, 1: float32 y, 2: y as XT).
// A split is divided among the four waves as k_cbpk_stream divides it.  A wave's rows are walked in stretches cut at the group's
// end, each a run of batches of U rows and then single rows, so a boundary inside a batch or a wave that starts inside a group
// needs nothing more; with one group these are the batches and the sums of k_cbpk_stream.  Everything that steers the walk (the
// wave's rows, the group, the stretch) is computed from blockIdx and the readfirstlane'd wave number: uniform, in SGPRs.  The
// lanes differ only in the centre they hold, picked by a clamped address and a select, never by a branch.
template <typename XT, int BITS, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS, 2) void k_cbpk_stream_grouped(const XT *__restrict__ x, int m, long long kdim,
                                                                       const unsigned char *__restrict__ packed, long long row_bytes, long long ncols,
                                                                       const float *__restrict__ centers, int k, long long rows_per_split,
                                                                       long long group_rows, const float *__restrict__ bias, int relu, int direct,
                                                                       void *__restrict__ out_)
{
    constexpr int E = 8 * VB / BITS, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BITS, ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    constexpr int U = E >= 32 ? 4 : CB_UNROLL;          // rows in flight, as k_cbpk_stream
    static_assert(E * MT <= PK_ACC, "accumulators per lane");
    extern __shared__ float smem[];
    float *red = smem + CB_WAVES * ENTRIES * PK_COPIES; // [MT * E][64]
    float *out = reinterpret_cast<float *>(out_);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *cb = smem + wave * (ENTRIES * PK_COPIES);    // this wave's table: [ENTRIES][PK_COPIES]
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;                     // then the lane's VB bytes lie inside the padded row
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    const long long per_wave = (s_hi - s_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(s_hi, s_lo + wave * per_wave), i1 = std::min(s_hi, i0 + per_wave);
    const unsigned char *mine = packed + (active ? (long long)blockIdx.x * (64 * VB) + lane * VB : 0LL);
    const char *tab = reinterpret_cast<const char *>(cb) + ((lane & (PK_COPIES - 1)) << 2);

    float acc[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[r][e] = 0.0f;

    // lane j holds centre j of group g, rounded to XT as centers.to(dtype) does; 0 from k on
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
        }
        __builtin_amdgcn_wave_barrier();                // the lookups below read what other lanes of this wave wrote
    };
    auto load_x = [&](long long i, int U, float &xa, float &xb) { cb_load_x<MT>(x, kdim, m, lane, i, U, xa, xb); };
    auto consume = [&](const uint32_t *w, float xa, float xb, int u, int U) {
        float xv[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            const int f = r * U + u;
            xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            constexpr int SH = 7;                                        // entry l of this lane's copy at byte l << 7
            const int bit = BITS * (e % PER);
            const uint32_t d = w[e / PER];
            const uint32_t a = (bit >= SH ? d >> (bit - SH) : d << (SH - bit)) & (MASK << SH);
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
                uint32_t w[U][N];
                float xa, xb;
#pragma unroll
                for (int u = 0; u < U; ++u) pk_load<VB>(mine + (i + u) * row_bytes, w[u]);
                load_x(i, U, xa, xb);
#pragma unroll
                for (int u = 0; u < U; ++u) consume(w[u], xa, xb, u, U);
            }
            for (; i < e1; ++i) {
                uint32_t w[N];
                float xa, xb;
                pk_load<VB>(mine + i * row_bytes, w);
                load_x(i, 1, xa, xb);
                consume(w, xa, xb, 0, 1);
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
// k_cbpk_tiled (nnc_cbpk.hip) with centers[groups][k]: the same grid, tile, decode and FMA order.  A split can start off a multiple
// of TB_K, so a TB_K step can lie across a boundary, in at most two groups (group_rows >= 32): LDS holds two tables of 2^BITS
// entries, group g in slot g & 1, as k_cbmm_tiled_grouped holds them.  The table of a step's last row is written ahead of the
// step's first barrier when it is not there yet; the slot it replaces was last read two groups earlier, before a barrier every
// thread has passed.
template <int BITS>
__global__ __launch_bounds__(256) void k_cbpk_tiled_grouped(const float *__restrict__ x, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                            long long row_bytes, long long ncols, const float *__restrict__ centers, int k,
                                                            long long col_tiles, long long rows_per_split, long long group_rows,
                                                            const float *__restrict__ bias, int relu, int direct, float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // two tables of 2^BITS entries (zeros from k on)
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
    const long long wbyte = T.n0 * BITS / 8 + (wc * BITS / 32) * 4;
    const int wshift = wc * BITS % 32;
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        if (std::min(kb + TB_K, T.hi) > (g_top + 1) * group_rows) table(++g_top);   // the step's last row opens a group
        __syncthreads();
        tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
        const float *tab = cb + ((gk >= g_top * group_rows ? g_top : g_top - 1) & 1) * ENTRIES;   // a step's rows lie in g_top - 1 and g_top
        const bool live = gk < T.hi && wbyte < row_bytes;
        const uint32_t word = live ? *reinterpret_cast<const uint32_t *>(packed + gk * row_bytes + wbyte) >> wshift : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[wk * TB_N + wc + j] = live ? tab[(word >> (BITS * j)) & MASK] : 0.0f;
        __syncthreads();
        tb_tile_fma(xs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_y(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, ncols, bias, relu, direct, out);
}

// ------------------------------------------------------------------ MFMA tile: m > 16, bf16 / fp16 x
// k_cbmm_mfma_grouped (nnc_cbmm_grouped.hip) with the label of (gk, gc) taken from the packed row: the same grid, the same tile and
// k loop (nnc_cbmfma.hpp, the refill as hm_accumulate's `open`), the per-bank table of 2^BITS entries (the centres rounded to XT, zeros from k on).  Thread t owns column wc of
// the tile and 16 rows of the k step: 16 byte loads, the threads of neighbouring columns reading the same byte.  Splits start on
// whole k steps of HM_BK = 32 and group_rows is a multiple of 32, so a step lies in one group; a step that opens a group rewrites
// the first k table entries ahead of its first barrier: the lookups of the step before ended at that step's second barrier.
template <typename XT, int BITS, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbpk_mfma_grouped(const XT *__restrict__ x, long long m, long long kdim,
                                                                  const unsigned char *__restrict__ packed, long long row_bytes, long long ncols,
                                                                  const float *__restrict__ centers, int k, long long col_tiles, long long rows_per_split,
                                                                  long long group_rows, const float *__restrict__ bias, int relu, int direct,
                                                                  void *__restrict__ out_)
{
    constexpr int ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, ENTRIES, PK_CSHIFT);   // the table: [ENTRIES][PK_COPIES]
    long long group = (long long)blockIdx.y * rows_per_split / group_rows;
    cb_fill<XT>(L.cb, L.stage, centers + group * k, k, ENTRIES, PK_CSHIFT);

    const HmTile T = hm_tile(col_tiles, rows_per_split, kdim);
    const long long gc = T.n0 + T.wc;
    const bool col_ok = gc < ncols;                     // then byte gc * BITS / 8 lies inside the row
    const long long cbyte = col_ok ? gc * BITS / 8 : 0;
    const int cshift = (int)(gc * BITS % 8);
    const long long k_end = col_ok ? T.k_hi : T.k_lo;   // the end of the thread's label rows: none in a column past ncols
    uint32_t lab[16];

    auto load_w = [&](long long kb) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long gk = kb + T.wk0 + j;
            lab[j] = gk < k_end ? ((uint32_t)packed[gk * row_bytes + cbyte] >> cshift) & MASK : 0u;
        }
    };
    auto store_w = [&](long long kb) {
        hm_lookup_w(L.ws, L.cb, T, col_ok, kb, lab, [&](uint32_t l) { return (l << PK_CSHIFT) | (T.lane & (PK_COPIES - 1)); });
    };
    auto open = [&](long long kb) {                     // this step opens a group
        if (kb >= (group + 1) * group_rows) cb_refill<XT>(L.cb, centers + ++group * k, k, PK_CSHIFT);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(x, m, kdim, T, L.xs, L.ws, acc, load_w, store_w, HmNothing(), open);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, ncols, bias, relu, direct, out_);
}

// ------------------------------------------------------------------ launches
template <typename XT, int BITS, int VB, int MT>
static void launch_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, int m, long long kdim, const unsigned char *packed, long long row_bytes,
                          long long ncols, const float *centers, int k, long long rps, long long group_rows, const float *bias, int relu, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbpk_stream_grouped<XT, BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), m, kdim, packed, row_bytes,
                       ncols, centers, k, rps, group_rows, bias, relu, direct, out);
}

template <typename XT, int BITS>
static void launch_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const unsigned char *packed, long long row_bytes,
                        long long ncols, const float *centers, int k, long long col_tiles, long long rps, long long group_rows, const float *bias, int relu,
                        int direct, void *out)
{
    hm_launch(x, kdim, k_cbpk_mfma_grouped<XT, BITS, true>, k_cbpk_mfma_grouped<XT, BITS, false>, grid, lds, s, reinterpret_cast<const XT *>(x), m, kdim,
              packed, row_bytes, ncols, centers, k, col_tiles, rps, group_rows, bias, relu, direct, out);
}

// every stream instantiation of this unit: the (bits, vb, mt) of nnc_cbpk.hip's table for each type of x.  The plan is checked
// against this table, and the launch goes through it.
using StreamLaunch = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const unsigned char *, long long, long long, const float *, int,
                              long long, long long, const float *, int, int, void *);
struct StreamCase {
    int dt, bits, vb, mt;
    StreamLaunch fn;
};
#define PKG_CASE(DT, XT, B, V, M) {DT, B, V, M, launch_stream<XT, B, V, M>}
#define PKG_STREAM_CASES(DT, XT)                                                                                                              \
    PKG_CASE(DT, XT, 4, 16, 1), PKG_CASE(DT, XT, 4, 16, 2), PKG_CASE(DT, XT, 4, 8, 1), PKG_CASE(DT, XT, 4, 8, 2), PKG_CASE(DT, XT, 4, 8, 4),  \
    PKG_CASE(DT, XT, 4, 4, 1), PKG_CASE(DT, XT, 4, 4, 2), PKG_CASE(DT, XT, 4, 4, 4), PKG_CASE(DT, XT, 4, 4, 8), PKG_CASE(DT, XT, 4, 2, 16),   \
    PKG_CASE(DT, XT, 2, 16, 1), PKG_CASE(DT, XT, 2, 8, 1), PKG_CASE(DT, XT, 2, 8, 2), PKG_CASE(DT, XT, 2, 4, 1), PKG_CASE(DT, XT, 2, 4, 2),   \
    PKG_CASE(DT, XT, 2, 4, 4), PKG_CASE(DT, XT, 2, 2, 8), PKG_CASE(DT, XT, 2, 1, 16)
static const StreamCase kStreamCases[] = {PKG_STREAM_CASES(NNC_DT_F32, float), PKG_STREAM_CASES(NNC_DT_BF16, bf16_t), PKG_STREAM_CASES(NNC_DT_F16, f16_t)};

static StreamLaunch find_stream(int dt, int bits, int vb, int mt)
{
    for (const StreamCase &c : kStreamCases)
        if (c.dt == dt && c.bits == bits && c.vb == vb && c.mt == mt) return c.fn;
    return nullptr;
}

// ------------------------------------------------------------------ the plan (host)
struct PkgPlan {
    PkPlan p;      // stream, tiled: pk_plan's; MFMA: the grid of cb_grid, the per-bank table
    int tables;    // tables held in LDS: one per wave (stream), two (tiled), one (MFMA)
};

static PkgPlan pkg_plan(int x_dtype, long long m, long long kdim, long long ncols, int bits, int cus)
{
    PkgPlan g{pk_plan(m, kdim, ncols, bits, cus), 0};
    PkPlan &p = g.p;
    if (p.path == NNC_CBMM_STREAM) {
        g.tables = CB_WAVES;
        p.lds = ((long long)CB_WAVES * p.entries * p.copies + (long long)p.mt * p.cols * 64) * 4;
    } else if (p.path == NNC_CBMM_TILED && x_dtype == NNC_DT_F32) {
        g.tables = 2;
        p.lds += (long long)p.entries * 4;   // the second table
    } else if (p.path == NNC_CBMM_TILED) {   // half x, m > 16: the MFMA tile on the grid nnc_cbmm_grouped takes for it
        CbPlan c{};
        cb_grid(c, m, kdim, ncols, 1, cus, true);
        p.path = NNC_CBMM_MFMA;
        p.copies = PK_COPIES;
        p.col_tiles = c.col_tiles;
        p.row_tiles = c.row_tiles;
        p.splits = c.splits;
        p.rows_per_split = c.rows_per_split;
        p.lds = (long long)hm_table_words(p.entries, PK_CSHIFT) * 4 + (long long)(HM_BM + HM_BN) * HM_LD * 2;
        g.tables = 1;
    }
    return g;
}

static int have_kernel(const PkPlan &p, int dt, int bits)
{
    if (p.path == NNC_CBMM_STREAM && !find_stream(dt, bits, p.vb, p.mt))
        return fail(NNC_EINVAL, "nnc_cbpk_grouped: no k_cbpk_stream_grouped instantiation for dtype " + std::to_string(dt) + ", bits " + std::to_string(bits) +
                                    ", vb " + std::to_string(p.vb) + ", mt " + std::to_string(p.mt));
    return NNC_OK;
}

// ------------------------------------------------------------------ C ABI
static int grouped_check(const char *fn, int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows)
{
    if (x_dtype != NNC_DT_F32 && x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16)
        return fail(NNC_EINVAL, std::string(fn) + ": x_dtype must be NNC_DT_F32, NNC_DT_BF16 or NNC_DT_F16");
    const int rc = pk_check(fn, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    return cb_check_group_rows(fn, kdim, group_rows);
}

extern "C" int64_t nnc_cbpk_grouped_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || grouped_check("nnc_cbpk_grouped_workspace_bytes", x_dtype, m, kdim, ncols, bits, 1, 32) != NNC_OK) return 0;
    return pk_ws_bytes(pkg_plan(x_dtype, m, kdim, ncols, bits, CB_PLAN_CUS).p, m, ncols);
}

extern "C" int nnc_cbpk_grouped_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out)
{
    int rc = grouped_check("nnc_cbpk_grouped_plan", x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbpk_grouped_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbpk_grouped_plan: out is NULL");
    const PkgPlan g = pkg_plan(x_dtype, m, kdim, ncols, bits, cus);
    const PkPlan &p = g.p;
    if ((rc = have_kernel(p, x_dtype, bits)) != NNC_OK) return rc;
    const int64_t v[NNC_CBPK_GROUPED_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.xrows, p.table, p.copies, p.entries, p.splits, p.rows_per_split, p.lds,
                                                  p.col_tiles, p.row_tiles, pk_ws_bytes(p, m, ncols), x_dtype, group_rows,
                                                  kdim > 0 ? cdiv(kdim, group_rows) : 0, p.splits > 0 ? max_groups_per_split(p.splits, p.rows_per_split, kdim, group_rows) : 0,
                                                  g.tables};
    for (int i = 0; i < NNC_CBPK_GROUPED_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbpk_grouped(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                                const float *centers_dev, int32_t k, int64_t group_rows, const float *bias_dev, int32_t relu, void *y, int y_dtype,
                                void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = grouped_check("nnc_cbpk_grouped", x_dtype, m, kdim, ncols, bits, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer("nnc_cbpk_grouped", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if ((rc = cb_check_operands("nnc_cbpk_grouped", x, x_dtype, y, y_dtype, centers_dev, m, kdim, ncols, !x, "x")) != NNC_OK) return rc;
    const int64_t need = nnc_cbpk_grouped_workspace_bytes(x_dtype, m, kdim, ncols, bits);
    if ((rc = cb_check_workspace("nnc_cbpk_grouped", "nnc_cbpk_grouped_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const PkPlan p = pkg_plan(x_dtype, m, kdim, ncols, bits, cu_count()).p;
    if (p.path == NNC_CBMM_BIAS) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // kdim = 0: y = bias
    if ((rc = have_kernel(p, x_dtype, bits)) != NNC_OK) return rc;
    const int direct = cb_direct(p.splits, y_dtype);
    void *out = direct ? y : workspace;
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    if (p.path == NNC_CBMM_STREAM) {
        find_stream(x_dtype, bits, p.vb, p.mt)(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, pk, row_bytes, ncols,
                                               centers_dev, k, p.rows_per_split, group_rows, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbpk_stream_grouped");
    } else if (p.path == NNC_CBMM_TILED) {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        if (bits == 4)
            hipLaunchKernelGGL(k_cbpk_tiled_grouped<4>, grid, dim3(256), (size_t)p.lds, s, reinterpret_cast<const float *>(x), (long long)m, (long long)kdim, pk,
                               row_bytes, (long long)ncols, centers_dev, (int)k, p.col_tiles, p.rows_per_split, (long long)group_rows, bias_dev, (int)relu,
                               direct, reinterpret_cast<float *>(out));
        else
            hipLaunchKernelGGL(k_cbpk_tiled_grouped<2>, grid, dim3(256), (size_t)p.lds, s, reinterpret_cast<const float *>(x), (long long)m, (long long)kdim, pk,
                               row_bytes, (long long)ncols, centers_dev, (int)k, p.col_tiles, p.rows_per_split, (long long)group_rows, bias_dev, (int)relu,
                               direct, reinterpret_cast<float *>(out));
        LAUNCHCHK("k_cbpk_tiled_grouped");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        auto fn = x_dtype == NNC_DT_BF16 ? (bits == 4 ? launch_mfma<bf16_t, 4> : launch_mfma<bf16_t, 2>) : (bits == 4 ? launch_mfma<f16_t, 4> : launch_mfma<f16_t, 2>);
        fn(grid, (size_t)p.lds, s, x, m, kdim, pk, row_bytes, ncols, centers_dev, k, p.col_tiles, p.rows_per_split, group_rows, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbpk_mfma_grouped");
    }
    return cb_finish(direct, workspace, p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
}
