// nnc_cbmm_grouped.hip -- the codebook matmul with one codebook per block of input rows (include/nnc.h, nnc_cbmm_grouped; DESIGN.md
// section 17): y = x @ W + bias, W[i, o] = centers[i / group_rows][labels[i * ncols + o]], uint8 labels, x float32, bf16 or fp16.
//
// The plan is the ungrouped one (cb_plan, nnc_cbmm.hpp) for the same shape, so the splits, the workspace and the summation order are
// those of nnc_cbmm_f32 / nnc_cbmm_h16.  The kernels are the ungrouped ones with one addition: a workgroup that walks from one group's
// rows into the next changes its LDS table.  They are kernels of their own and not instantiations of a body shared with the
// ungrouped ones: called through a device function, k_cbmm_stream compiles to another instruction stream.  The tiled one is, like
// k_cbmm_tiled, the tile skeleton of nnc_cbtile.hpp around its decode; the MFMA one is, like k_cbmm_mfma, the tile and the k loop
// of nnc_cbmfma.hpp around its table (cb_fill, cb_refill where a step opens a group), its label load and its lookup.
//   k_cbmm_stream_grouped  m <= 16: the split is walked group by group, the four waves share each stretch and the table.
//   k_cbmm_tiled_grouped   m > 16, float32 x: two small tables in LDS, a TB_K step may lie across a boundary.
//   k_cbmm_mfma_grouped    m > 16, bf16 / fp16 x: a k step of HM_BK never lies across a boundary (group_rows is a multiple of 32).
// With one group every kernel computes what its ungrouped counterpart computes, bit for bit.
#include "nnc_cbmfma.hpp"
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ skinny: m <= 16
// k_cbmm_stream (nnc_cbmm.hpp) with uint8 labels and centers[groups][k]: grid (col_tiles, splits), CB_THREADS threads, the same
// arguments and `direct` values.  The waves share one LDS table, so they stay inside one group at a time: the rows of the split
// are walked group by group, each stretch divided among the four waves as k_cbmm_stream divides a whole split, and the first k
// table entries are rewritten between two barriers at every boundary.  A stretch is cut at the split's ends and at the group's,
// so a boundary inside a batch of CB_UNROLL rows or a split that starts inside a group needs nothing more.  With one group these
// are the rows per wave and the sums of k_cbmm_stream.
template <typename XT, int VB, int MT, bool ALIGNED>
__global__ __launch_bounds__(CB_THREADS) void k_cbmm_stream_grouped(const XT *__restrict__ x, int m, long long kdim, const unsigned char *__restrict__ labels,
                                                                    long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                                    long long rows_per_split, long long group_rows, const float *__restrict__ bias,
                                                                    int relu, int direct, void *__restrict__ out_)
{
    using LT = uint8_t;
    constexpr int LB = sizeof(LT), E = VB / LB, N = VB / 4, PER = 32 / (8 * LB) /* labels per dword */;
    extern __shared__ float smem[];
    float *cb = smem;
    float *red = smem + (entries << cshift);
    float *stage = red + MT * E * 64;
    float *out = reinterpret_cast<float *>(out_);
    long long group = (long long)blockIdx.y * rows_per_split / group_rows;
    cb_fill<XT>(cb, stage, centers + group * k, k, entries, cshift);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    long long g_lo = s_lo, g_hi, i0, i1;   // the rows of the split that lie in `group`, and the wave's share of them
    cb_group_step(group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
    const uintptr_t base = reinterpret_cast<uintptr_t>(labels);
    const long long row_bytes = ncols * LB;
    const long long lane_off = (long long)blockIdx.x * (64 * VB) + lane * VB;   // byte offset of the lane's window in its row

    float acc[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[r][e] = 0.0f;
    __syncthreads();

    auto row_words = [&](long long i, uint32_t *w, uint32_t &s) { cb_row_words<VB, ALIGNED>(base, row_bytes, lane_off, active, i, w, s); };
    auto load_x = [&](long long i, int U, float &xa, float &xb) { cb_load_x<MT>(x, kdim, m, lane, i, U, xa, xb); };
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
            const uint32_t l = (o[e / PER] >> (8 * LB * (e % PER))) & (LB == 1 ? 0xFFu : 0xFFFFu);
            const float wv = cb[CbTable<LT>::index(l, k, cshift, lane)];
#pragma unroll
            for (int r = 0; r < MT; ++r) acc[r][e] = __builtin_fmaf(xv[r], wv, acc[r][e]);
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
        if (g_hi >= s_hi) break;
        // on to the next group's rows, divided among the waves as a whole split is
        g_lo = g_hi;
        cb_group_step(++group, group_rows, g_lo, s_hi, wave, g_hi, i0, i1);
        __syncthreads();   // every wave has left the rows of the group before
        cb_refill<XT>(cb, centers + group * k, k, cshift);
        __syncthreads();
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
// k_cbmm_tiled (nnc_cbmm.hip) with uint8 labels and centers[groups][k]: the same grid, tile and FMA order.  A split can start off a
// multiple of TB_K, so a TB_K step can lie across a boundary, in at most two groups (group_rows >= 32): LDS holds two tables, group
// g in slot g & 1.  The table of a step's last row is written ahead of the step's first barrier when it is not there yet; the slot
// it replaces was last read two groups earlier, before a barrier every thread has passed.
__global__ __launch_bounds__(256) void k_cbmm_tiled_grouped(const float *__restrict__ x, long long m, long long kdim, const uint8_t *__restrict__ labels,
                                                            long long ncols, const float *__restrict__ centers, int k, long long col_tiles,
                                                            long long rows_per_split, long long group_rows, const float *__restrict__ bias, int relu,
                                                            int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // two tables of k + 1 entries (entry k = 0)
    auto table = [&](long long g) {
        float *slot = cb + (g & 1) * (k + 1);
        for (int j = threadIdx.x; j <= k; j += 256) slot[j] = j < k ? centers[g * k + j] : 0.0f;
    };
    long long g_top = (long long)blockIdx.y * rows_per_split / group_rows;   // the last group whose table is in LDS
    table(g_top);

    const TbTile T = tb_tile(col_tiles, rows_per_split, kdim);
    float acc[8][8];
    tb_clear(acc);

    const int wk = threadIdx.x >> 5, wc = (threadIdx.x & 31) * 4;      // W tile: k wk, columns wc..wc+3
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        if (std::min(kb + TB_K, T.hi) > (g_top + 1) * group_rows) table(++g_top);   // the step's last row opens a group
        __syncthreads();
        tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
        const float *tab = cb + ((gk >= g_top * group_rows ? g_top : g_top - 1) & 1) * (k + 1);   // a step's rows lie in g_top - 1 and g_top
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long gc = T.n0 + wc + j;
            float v = 0.0f;
            if (gk < T.hi && gc < ncols) v = tab[std::min((uint32_t)labels[gk * ncols + gc], (uint32_t)k)];
            ws[wk * TB_N + wc + j] = v;
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
// k_cbmm_mfma (nnc_cbmm_h16.hip) with uint8 labels and centers[groups][k]: the same grid and the same tile (nnc_cbmfma.hpp: images,
// k loop, epilogue); its own are the group walk, the label load and the lookup.  Splits start on
// whole k steps of HM_BK = 32 and group_rows is a multiple of 32, so a step lies in one group.  A step that opens a group rewrites
// the first k table entries ahead of its first barrier (hm_accumulate's `open`): the lookups of the step before ended at that
// step's second barrier.
template <typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbmm_mfma_grouped(const XT *__restrict__ x, long long m, long long kdim, const uint8_t *__restrict__ labels,
                                                                  long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                                  long long col_tiles, long long rows_per_split, long long group_rows,
                                                                  const float *__restrict__ bias, int relu, int direct, void *__restrict__ out_)
{
    using LT = uint8_t;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, entries, cshift);
    long long group = (long long)blockIdx.y * rows_per_split / group_rows;
    cb_fill<XT>(L.cb, L.stage, centers + group * k, k, entries, cshift);

    const HmTile T = hm_tile(col_tiles, rows_per_split, kdim);
    const long long gc = T.n0 + T.wc;
    const bool col_ok = gc < ncols;
    const long long k_end = col_ok ? T.k_hi : T.k_lo;   // the end of the thread's label rows: none in a column past ncols
    uint32_t lab[16];

    auto load_w = [&](long long kb) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long gk = kb + T.wk0 + j;
            lab[j] = gk < k_end ? (uint32_t)labels[gk * ncols + gc] : 0u;
        }
    };
    auto store_w = [&](long long kb) {
        hm_lookup_w(L.ws, L.cb, T, col_ok, kb, lab, [&](uint32_t l) { return CbTable<LT>::index(l, k, cshift, T.lane); });
    };
    auto open = [&](long long kb) {                     // this step opens a group
        if (kb >= (group + 1) * group_rows) cb_refill<XT>(L.cb, centers + ++group * k, k, cshift);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(x, m, kdim, T, L.xs, L.ws, acc, load_w, store_w, HmNothing(), open);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, ncols, bias, relu, direct, out_);
}

// ------------------------------------------------------------------ launches
template <typename XT, int VB, int MT>
static void launch_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const void *x, int m, long long kdim, const void *labels, long long ncols,
                          const float *centers, int k, int entries, int cshift, long long rps, long long group_rows, const float *bias, int relu, int direct,
                          void *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    const XT *xp = reinterpret_cast<const XT *>(x);
    if (aligned)
        hipLaunchKernelGGL((k_cbmm_stream_grouped<XT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, xp, m, kdim, lab, ncols, centers, k, entries, cshift, rps, group_rows, bias, relu, direct, out);
    else
        hipLaunchKernelGGL((k_cbmm_stream_grouped<XT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, xp, m, kdim, lab, ncols, centers, k, entries, cshift, rps, group_rows, bias, relu, direct, out);
}

template <typename XT>
static void launch_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const void *labels, long long ncols,
                        const float *centers, int k, int entries, int cshift, long long col_tiles, long long rps, long long group_rows, const float *bias,
                        int relu, int direct, void *out)
{
    hm_launch(x, kdim, k_cbmm_mfma_grouped<XT, true>, k_cbmm_mfma_grouped<XT, false>, grid, lds, s, reinterpret_cast<const XT *>(x), m, kdim,
              reinterpret_cast<const uint8_t *>(labels), ncols, centers, k, entries, cshift, col_tiles, rps, group_rows, bias, relu, direct, out);
}

// every stream instantiation of this unit; the plan is checked against this table, and the launch goes through it
using StreamLaunch = void (*)(bool, dim3, size_t, hipStream_t, const void *, int, long long, const void *, long long, const float *, int, int, int, long long,
                              long long, const float *, int, int, void *);
struct StreamCase {
    int dt, vb, mt;
    StreamLaunch fn;
};
#define GROUPED_STREAM_CASES(DT, XT)                                                                                                  \
    {DT, 16, 1, launch_stream<XT, 16, 1>}, {DT, 16, 2, launch_stream<XT, 16, 2>}, {DT, 16, 4, launch_stream<XT, 16, 4>},              \
    {DT, 8, 8, launch_stream<XT, 8, 8>}, {DT, 4, 16, launch_stream<XT, 4, 16>}
static const StreamCase kStreamCases[] = {GROUPED_STREAM_CASES(NNC_DT_F32, float), GROUPED_STREAM_CASES(NNC_DT_BF16, bf16_t),
                                          GROUPED_STREAM_CASES(NNC_DT_F16, f16_t)};

static StreamLaunch find_stream(int dt, int vb, int mt)
{
    for (const StreamCase &c : kStreamCases)
        if (c.dt == dt && c.vb == vb && c.mt == mt) return c.fn;
    return nullptr;
}

static int have_kernel(const CbPlan &p, int dt)
{
    if (p.path == NNC_CBMM_STREAM && !find_stream(dt, p.vb, p.mt))
        return fail(NNC_EINVAL, "nnc_cbmm_grouped: no k_cbmm_stream_grouped instantiation for dtype " + std::to_string(dt) + ", vb " + std::to_string(p.vb) +
                                    ", mt " + std::to_string(p.mt));
    return NNC_OK;
}

// ------------------------------------------------------------------ C ABI
static int grouped_check(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows)
{
    if (x_dtype != NNC_DT_F32 && x_dtype != NNC_DT_BF16 && x_dtype != NNC_DT_F16)
        return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_grouped: x_dtype must be NNC_DT_F32, NNC_DT_BF16 or NNC_DT_F16");
    if (m < 0 || kdim < 0 || ncols < 0) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_grouped: negative size");
    if (k < 1 || k > 256) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_grouped: k outside 1..256 (group codebooks take uint8 labels only)");
    const int rc = cb_check_group_rows("nnc_cbmm_grouped", kdim, group_rows);
    if (rc != NNC_OK) return rc;
    if (m > (1LL << 40) || kdim > (1LL << 40) || ncols > (1LL << 40)) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_grouped: size too large");
    return NNC_OK;
}

static CbPlan grouped_plan(int x_dtype, long long m, long long kdim, long long ncols, int k, int cus, uintptr_t labels)
{
    CbPlan p = cb_plan(m, kdim, ncols, 1, k, cus, labels, x_dtype != NNC_DT_F32);
    if (p.path == NNC_CBMM_TILED) p.lds += (long long)(k + 1) * 4;   // the second table
    return p;
}

extern "C" int64_t nnc_cbmm_grouped_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols)
{
    return x_dtype == NNC_DT_F32 ? nnc_cbmm_workspace_bytes(m, kdim, ncols, 1) : nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, 1);
}

extern "C" int nnc_cbmm_grouped_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, uint64_t labels_addr,
                                     int64_t *out)
{
    int rc = grouped_check(x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_grouped_plan: cus < 1");
    if (!out) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_grouped_plan: out is NULL");
    const CbPlan p = grouped_plan(x_dtype, m, kdim, ncols, k, cus, (uintptr_t)labels_addr);
    rc = have_kernel(p, x_dtype);
    if (rc != NNC_OK) return rc;
    const int64_t v[NNC_CBMM_GROUPED_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_TILED ? 2 : (p.entries ? 1LL << p.cshift : 0), p.entries, p.splits,
                                                  p.rows_per_split, p.aligned, p.lds, p.col_tiles, p.row_tiles, cb_ws_bytes(p, m, ncols), x_dtype, group_rows,
                                                  kdim > 0 ? cdiv(kdim, group_rows) : 0, p.splits > 0 ? max_groups_per_split(p.splits, p.rows_per_split, kdim, group_rows) : 0};
    for (int i = 0; i < NNC_CBMM_GROUPED_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_grouped(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *labels, int64_t ncols, const float *centers_dev, int32_t k,
                                int64_t group_rows, const float *bias_dev, int32_t relu, void *y, int y_dtype, void *workspace, int64_t workspace_bytes,
                                void *stream)
{
    int rc = grouped_check(x_dtype, m, kdim, ncols, k, group_rows);
    if (rc != NNC_OK) return rc;
    if ((rc = cb_check_operands("nnc_cbmm_grouped", x, x_dtype, y, y_dtype, centers_dev, m, kdim, ncols, !x || !labels, "x or labels")) != NNC_OK) return rc;
    const int64_t need = nnc_cbmm_grouped_workspace_bytes(x_dtype, m, kdim, ncols);
    if ((rc = cb_check_workspace("nnc_cbmm_grouped", "nnc_cbmm_grouped_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const CbPlan p = grouped_plan(x_dtype, m, kdim, ncols, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    if (p.path == NNC_CBMM_BIAS) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // kdim = 0: y = bias
    rc = have_kernel(p, x_dtype);
    if (rc != NNC_OK) return rc;
    const int direct = cb_direct(p.splits, y_dtype);
    void *out = direct ? y : workspace;
    if (p.path == NNC_CBMM_STREAM) {
        const dim3 grid((unsigned)p.col_tiles, (unsigned)p.splits);
        find_stream(x_dtype, p.vb, p.mt)(p.aligned != 0, grid, (size_t)p.lds, s, x, (int)m, kdim, labels, ncols, centers_dev, k, p.entries, p.cshift,
                                         p.rows_per_split, group_rows, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbmm_stream_grouped");
    } else if (p.path == NNC_CBMM_TILED) {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        hipLaunchKernelGGL(k_cbmm_tiled_grouped, grid, dim3(256), (size_t)p.lds, s, reinterpret_cast<const float *>(x), (long long)m, (long long)kdim,
                           reinterpret_cast<const uint8_t *>(labels), (long long)ncols, centers_dev, (int)k, p.col_tiles, p.rows_per_split,
                           (long long)group_rows, bias_dev, (int)relu, direct, reinterpret_cast<float *>(out));
        LAUNCHCHK("k_cbmm_tiled_grouped");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        (x_dtype == NNC_DT_BF16 ? launch_mfma<bf16_t> : launch_mfma<f16_t>)(grid, (size_t)p.lds, s, x, m, kdim, labels, ncols, centers_dev, k, p.entries, p.cshift,
                                                                            p.col_tiles, p.rows_per_split, group_rows, bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbmm_mfma_grouped");
    }
    return cb_finish(direct, workspace, p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
}
