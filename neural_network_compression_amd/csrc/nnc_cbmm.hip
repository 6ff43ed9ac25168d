// nnc_cbmm.hip -- the quantized layer run from its codebook and centroid indices: y[m, ncols] = x[m, kdim] @ W + bias (then
// ReLU if asked), W[i, o] = centers[labels[i * ncols + o]], the fp32 W never stored (include/nnc.h, nnc_cbmm_f32).
//
// Two regimes ("Running the compressed layer"):
//   k_cbmm_stream  m <= 16: bound by the index stream.  A wave owns 64 lanes x VB bytes of a label row (VB = 16, 8 or 4: the
//                  widest load that keeps the m x (VB / label_bytes) accumulators of a lane within 64 registers), loaded straight
//                  to VGPRs, CB_UNROLL rows in flight; x[r, i] is uniform over the wave (vector load + v_readlane).  The codebook sits in LDS
//                  with one copy per bank: entry j of lane l at word j * C + (l mod C), C = 32 where it fits (K <= 256: every
//                  lane always hits its own bank, 2 LDS cycles per 64 lookups), fewer copies for K > 256.  The 4 waves of a
//                  workgroup split its rows and are summed in LDS in wave order; workgroups split K.
//   k_cbmm_tiled   m > 16: bound by compute.  128 x 128 output tiles, the W tile dequantized from its indices into LDS once per
//                  workgroup and reused by all 128 rows of x (register-blocked FMA, 8 x 8 outputs per thread).
//   k_cbmm_reduce  the split-K partials summed in split order, + bias, ReLU.  No float atomics anywhere: the number of splits
//                  depends only on the shape and the CU count, so the same call gives the same bits.
// Label rows need not be aligned (any ncols, any storage offset): a lane loads the two aligned VB-byte chunks around its window
// and funnel-shifts them (v_alignbyte) by the row's misalignment, which is uniform over the wave.  An aligned chunk that holds
// one byte of the tensor lies in the tensor's page, so no load leaves the allocation; lanes past the last column load their
// row's first chunk and store nothing.  An index >= K reads 0, as nnc_gather_f32 does.
#include "nnc_cbmm.hpp"

// ------------------------------------------------------------------ the plan (host)
// Every decision nnc_cbmm_f32 takes before it launches: which kernel, its instantiation, the LDS table, the grid and the K
// splits.  nnc_cbmm_plan reports it (include/nnc.h), so the tests can see which regime a call hits.
struct CbPlan {
    int path;                // NNC_CBMM_NONE / _STREAM / _TILED / _BIAS
    int vb, mt;              // stream: bytes per lane per row, rows of x per launch (a power of two >= m)
    int entries, cshift;     // the LDS codebook: entries (centres, then zeros) x (1 << cshift) copies
    int aligned;             // stream: every label row starts on a VB-byte boundary (no funnel shift)
    long long col_tiles, row_tiles;
    long long splits, rows_per_split;
    long long lds;           // dynamic LDS bytes of the main kernel
};

// the splits and tiles (m >= 1, kdim >= 1, ncols >= 1)
static void cb_grid(CbPlan &p, long long m, long long kdim, long long ncols, int lb, int cus)
{
    cus = std::max(1, std::min(cus, CB_PLAN_CUS));
    long long s;
    if (m <= CB_SKINNY_M) {
        p.path = NNC_CBMM_STREAM;
        p.mt = m <= 1 ? 1 : (m <= 2 ? 2 : (m <= 4 ? 4 : (m <= 8 ? 8 : 16)));
        const int e_max = 64 / p.mt;                                 // accumulators per lane <= 64
        p.vb = std::min(16, e_max * lb);
        p.row_tiles = 1;
        p.col_tiles = cdiv(ncols, 64LL * (p.vb / lb));
        // enough workgroups for two per CU; every wave keeps at least one batch of rows; the partials (splits x m x ncols x 4 B)
        // stay within a quarter of the index stream
        s = std::min({cdiv(2LL * cus, p.col_tiles), kdim / (CB_WAVES * CB_UNROLL), kdim * lb / (16 * m)});
    } else {
        p.path = NNC_CBMM_TILED;
        p.col_tiles = cdiv(ncols, TB_N);
        p.row_tiles = cdiv(m, TB_M);
        s = std::min({cdiv(2LL * cus, p.col_tiles * p.row_tiles), kdim / (16 * TB_K), 16LL});
    }
    s = std::max(1LL, s);
    p.rows_per_split = cdiv(kdim, s);
    p.splits = cdiv(kdim, p.rows_per_split);
}

static CbPlan cb_plan(long long m, long long kdim, long long ncols, int lb, int k, int cus, uintptr_t labels)
{
    CbPlan p{};
    if (m == 0 || ncols == 0) return p;                              // NNC_CBMM_NONE: nothing to write
    if (kdim == 0) {                                                 // y = bias (zeros without one), by k_cbmm_reduce
        p.path = NNC_CBMM_BIAS;
        return p;
    }
    cb_grid(p, m, kdim, ncols, lb, cus);
    if (p.path == NNC_CBMM_STREAM) {
        if (lb == 1) {
            p.entries = 256;
            p.cshift = __builtin_ctz(CB_U8_COPIES);
        } else {
            p.entries = k + 1;
            while ((1 << p.cshift) < CB_U8_COPIES && (long long)p.entries << (p.cshift + 1) <= CB_U16_WORDS) ++p.cshift;
        }
        p.aligned = labels % p.vb == 0 && (ncols * lb) % p.vb == 0;
        p.lds = ((long long)p.entries << p.cshift) * 4 + (long long)p.mt * (p.vb / lb) * 64 * 4 + (long long)p.entries * 4;
    } else {
        p.entries = k + 1;
        p.lds = (long long)(TB_K * TB_M + TB_K * TB_N + k + 1) * 4;
    }
    return p;
}

static int64_t cb_ws_bytes(const CbPlan &p, long long m, long long ncols) { return p.splits > 1 ? (int64_t)p.splits * m * ncols * 4 : 0; }

// ------------------------------------------------------------------ skinny: m <= 16
// grid (col_tiles, splits), CB_THREADS threads.  `out` is y (splits == 1: + bias, ReLU here) or the partials [split][m][ncols].
template <typename LT, int VB, int MT, bool ALIGNED>
__global__ __launch_bounds__(CB_THREADS) void k_cbmm_stream(const float *__restrict__ x, int m, long long kdim, const unsigned char *__restrict__ labels,
                                                            long long ncols, const float *__restrict__ centers, int k, int entries, int cshift,
                                                            long long rows_per_split, const float *__restrict__ bias, int relu, int direct,
                                                            float *__restrict__ out)
{
    constexpr int LB = sizeof(LT), E = VB / LB, N = VB / 4, PER = 32 / (8 * LB) /* labels per dword */;
    extern __shared__ float smem[];
    float *cb = smem;
    float *red = smem + (entries << cshift);
    float *stage = red + MT * E * 64;
    cb_fill(cb, stage, centers, k, entries, cshift);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    const long long per_wave = (s_hi - s_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(s_hi, s_lo + wave * per_wave), i1 = std::min(s_hi, i0 + per_wave);
    const uintptr_t base = reinterpret_cast<uintptr_t>(labels);
    const long long row_bytes = ncols * LB;
    const long long lane_off = (long long)blockIdx.x * (64 * VB) + lane * VB;   // byte offset of the lane's window in its row

    float acc[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[r][e] = 0.0f;
    __syncthreads();

    auto row_words = [&](long long i, uint32_t *w, uint32_t &s) {
        const uintptr_t row = base + (uintptr_t)(i * row_bytes);
        if constexpr (ALIGNED) {
            s = 0;
            load_chunk<VB>(reinterpret_cast<const unsigned char *>(active ? row + lane_off : row), w);
        } else {
            const uintptr_t first = row & ~(uintptr_t)(VB - 1);          // the chunk that holds the row's first byte
            s = (uint32_t)(__builtin_amdgcn_readfirstlane((uint32_t)((row + blockIdx.x * (64 * VB)) & (VB - 1))));
            const uintptr_t a = ((row + lane_off) & ~(uintptr_t)(VB - 1));
            const uintptr_t a0 = active ? a : first;
            const uintptr_t a1 = (active && a + VB < row + row_bytes) ? a + VB : a0;
            load_chunk<VB>(reinterpret_cast<const unsigned char *>(a0), w);
            load_chunk<VB>(reinterpret_cast<const unsigned char *>(a1), w + N);
        }
    };
    // x[r, i + u] of a batch of U rows: lane f holds value f = r * U + u (and f + 64), broadcast by v_readlane.  Vector loads
    // keep the x reads off the LGKM counter that every LDS lookup waits on.
    auto load_x = [&](long long i, int U, float &xa, float &xb) {
        const int f0 = lane, f1 = lane + 64;
        const int r0 = f0 / U, r1 = f1 / U;
        xa = r0 < m ? x[(long long)r0 * kdim + i + f0 % U] : 0.0f;
        xb = (MT * CB_UNROLL > 64 && r1 < m) ? x[(long long)r1 * kdim + i + f1 % U] : 0.0f;
    };
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
                out[(long long)r * ncols + c] = v;
            } else {
                out[((long long)blockIdx.y * m + r) * ncols + c] = v;
            }
        }
    }
}

// ------------------------------------------------------------------ tiled: m > 16
// grid (col_tiles * row_tiles, splits), 256 threads; thread (tx, ty) = (t % 16, t / 16) owns rows ty*8.. and columns tx*8.. of
// the 128 x 128 tile.
template <typename LT>
__global__ __launch_bounds__(256) void k_cbmm_tiled(const float *__restrict__ x, long long m, long long kdim, const LT *__restrict__ labels, long long ncols,
                                                    const float *__restrict__ centers, int k, long long col_tiles, long long rows_per_split,
                                                    const float *__restrict__ bias, int relu, int direct, float *__restrict__ out)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // k + 1 entries (entry k = 0)
    for (int j = threadIdx.x; j <= k; j += 256) cb[j] = j < k ? centers[j] : 0.0f;

    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long long n0 = (blockIdx.x % col_tiles) * TB_N, m0 = (blockIdx.x / col_tiles) * TB_M;
    const long long k_lo = (long long)blockIdx.y * rows_per_split, k_hi = std::min(kdim, k_lo + rows_per_split);
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.0f;

    const int xr = t >> 1, xk = (t & 1) * 4;       // x tile: row xr, k xk..xk+3
    const int wk = t >> 5, wc = (t & 31) * 4;      // W tile: k wk, columns wc..wc+3
    for (long long kb = k_lo; kb < k_hi; kb += TB_K) {
        __syncthreads();
        {
            const long long gr = m0 + xr;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long gk = kb + xk + j;
                xs[(xk + j) * TB_M + xr] = (gr < m && gk < k_hi) ? x[gr * kdim + gk] : 0.0f;
            }
            const long long gk = kb + wk;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long gc = n0 + wc + j;
                float v = 0.0f;
                if (gk < k_hi && gc < ncols) v = cb[std::min((uint32_t)labels[gk * ncols + gc], (uint32_t)k)];
                ws[wk * TB_N + wc + j] = v;
            }
        }
        __syncthreads();
        tb_tile_fma(xs, ws, tx, ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const long long r = m0 + ty * 8 + a;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const long long c = n0 + tx * 8 + b;
            if (r >= m || c >= ncols) continue;
            float v = acc[a][b];
            if (direct) {
                if (bias) v += bias[c];
                if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
                out[r * ncols + c] = v;
            } else {
                out[((long long)blockIdx.y * m + r) * ncols + c] = v;
            }
        }
    }
}

// ------------------------------------------------------------------ split-K combine
// y = ((q0 + q1) + q2) + q3 + bias, q = the in-order sum of a quarter of the splits: 64 outputs per workgroup, a quarter per wave
// (one thread per output summing all splits serially was 25-37 us at m = 1 with ~100 splits).  The order depends on `splits` only.
#define RED_Q 4
__global__ __launch_bounds__(256) void k_cbmm_reduce(const float *__restrict__ part, long long splits, long long mn, long long ncols,
                                                     const float *__restrict__ bias, int relu, float *__restrict__ y)
{
    __shared__ float qs[RED_Q - 1][64];
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long per_q = (splits + RED_Q - 1) / RED_Q;
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
            for (int j = 0; j < RED_Q - 1; ++j) v += qs[j][o];
            if (bias) v += bias[idx % ncols];
            if (relu) v = v < 0.0f ? 0.0f : v;   // NaN stays NaN, as torch.relu
            y[idx] = v;
        }
    }
}

int cbmm_reduce(const float *part, long long splits, long long mn, long long ncols, const float *bias, int relu, float *y, hipStream_t s)
{
    const int rgrid = (int)std::max(1LL, std::min(cdiv(mn, 64), 8192LL));
    hipLaunchKernelGGL(k_cbmm_reduce, dim3(rgrid), dim3(256), 0, s, part, splits, mn, ncols, bias, relu, y);
    LAUNCHCHK("k_cbmm_reduce");
    return NNC_OK;
}

// ------------------------------------------------------------------ C ABI
static int cb_check(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k)
{
    if (m < 0 || kdim < 0 || ncols < 0) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: negative size");
    if (label_bytes != 1 && label_bytes != 2) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: label_bytes must be 1 or 2");
    if (k < 1 || k > NNC_KMAX) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: k outside 1..NNC_KMAX");
    if (label_bytes == 1 && k > 256) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: k > 256 needs 2-byte labels");
    if (m > (1LL << 40) || kdim > (1LL << 40) || ncols > (1LL << 40)) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: size too large");
    return NNC_OK;
}

extern "C" int64_t nnc_cbmm_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || (label_bytes != 1 && label_bytes != 2) || cb_check(m, kdim, ncols, label_bytes, 1) != NNC_OK) return 0;
    return cb_ws_bytes(cb_plan(m, kdim, ncols, label_bytes, 1, CB_PLAN_CUS, 0), m, ncols);
}

template <typename LT, int VB, int MT>
static void launch_stream(bool aligned, dim3 grid, size_t lds, hipStream_t s, const float *x, int m, long long kdim, const void *labels, long long ncols,
                          const float *centers, int k, int entries, int cshift, long long rps, const float *bias, int relu, int direct, float *out)
{
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (aligned)
        hipLaunchKernelGGL((k_cbmm_stream<LT, VB, MT, true>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, lab, ncols, centers, k, entries, cshift, rps, bias, relu, direct, out);
    else
        hipLaunchKernelGGL((k_cbmm_stream<LT, VB, MT, false>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, lab, ncols, centers, k, entries, cshift, rps, bias, relu, direct, out);
}

// every k_cbmm_stream instantiation there is; the plan is checked against this table, and the launch goes through it
using StreamLaunch = void (*)(bool, dim3, size_t, hipStream_t, const float *, int, long long, const void *, long long, const float *, int, int, int,
                              long long, const float *, int, int, float *);
struct StreamCase {
    int lb, vb, mt;
    StreamLaunch fn;
};
static const StreamCase kStreamCases[] = {
    {1, 16, 1, launch_stream<uint8_t, 16, 1>},  {1, 16, 2, launch_stream<uint8_t, 16, 2>},  {1, 16, 4, launch_stream<uint8_t, 16, 4>},
    {1, 8, 8, launch_stream<uint8_t, 8, 8>},    {1, 4, 16, launch_stream<uint8_t, 4, 16>},
    {2, 16, 1, launch_stream<uint16_t, 16, 1>}, {2, 16, 2, launch_stream<uint16_t, 16, 2>}, {2, 16, 4, launch_stream<uint16_t, 16, 4>},
    {2, 16, 8, launch_stream<uint16_t, 16, 8>}, {2, 8, 16, launch_stream<uint16_t, 8, 16>},
};

static StreamLaunch find_stream(int lb, int vb, int mt)
{
    for (const StreamCase &c : kStreamCases)
        if (c.lb == lb && c.vb == vb && c.mt == mt) return c.fn;
    return nullptr;
}

static int no_stream_case(int lb, int vb, int mt)
{
    return fail(NNC_EINVAL, "nnc_cbmm: no k_cbmm_stream instantiation for label_bytes " + std::to_string(lb) + ", vb " + std::to_string(vb) +
                                ", mt " + std::to_string(mt));
}

static int dispatch_stream(const CbPlan &p, int lb, dim3 grid, hipStream_t s, const float *x, int m, long long kdim, const void *labels, long long ncols,
                           const float *centers, int k, const float *bias, int relu, int direct, float *out)
{
    const StreamLaunch fn = find_stream(lb, p.vb, p.mt);
    if (!fn) return no_stream_case(lb, p.vb, p.mt);
    fn(p.aligned != 0, grid, (size_t)p.lds, s, x, m, kdim, labels, ncols, centers, k, p.entries, p.cshift, p.rows_per_split, bias, relu, direct, out);
    return NNC_OK;
}

extern "C" int nnc_cbmm_plan(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr, int64_t *out)
{
    const int rc = cb_check(m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_plan: cus < 1");
    if (!out) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_plan: out is NULL");
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cus, (uintptr_t)labels_addr);
    if (p.path == NNC_CBMM_STREAM && !find_stream(label_bytes, p.vb, p.mt)) return no_stream_case(label_bytes, p.vb, p.mt);
    const int64_t v[NNC_CBMM_PLAN_LEN] = {p.path, p.vb, p.mt, p.path == NNC_CBMM_STREAM ? 1LL << p.cshift : (p.entries ? 1 : 0), p.entries,
                                          p.splits, p.rows_per_split, p.aligned, p.lds, p.col_tiles, p.row_tiles, cb_ws_bytes(p, m, ncols)};
    for (int i = 0; i < NNC_CBMM_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbmm_f32(const float *x, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols, const float *centers_dev,
                            int32_t k, const float *bias_dev, int32_t relu, float *y, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = cb_check(m, kdim, ncols, label_bytes, k);
    if (rc != NNC_OK) return rc;
    if (!centers_dev) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: centers is NULL");
    if (m > 0 && ncols > 0 && !y) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: y is NULL");
    if (m > 0 && ncols > 0 && kdim > 0 && (!x || !labels)) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: x or labels is NULL");
    if (workspace_bytes < 0) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: negative workspace size");
    const int64_t need = nnc_cbmm_workspace_bytes(m, kdim, ncols, label_bytes);
    if (workspace_bytes < need) return nnc_set_error_(NNC_ENOSPACE, "nnc_cbmm_f32: workspace smaller than nnc_cbmm_workspace_bytes()");
    if (need > 0 && !workspace) return nnc_set_error_(NNC_EINVAL, "nnc_cbmm_f32: workspace is NULL");
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const CbPlan p = cb_plan(m, kdim, ncols, label_bytes, k, cu_count(), reinterpret_cast<uintptr_t>(labels));
    if (p.path == NNC_CBMM_BIAS) {   // kdim = 0: y = bias (zeros without one)
        return cbmm_reduce(nullptr, 0, mn, ncols, bias_dev, relu, y, s);
    }
    const int direct = p.splits == 1;
    float *out = direct ? y : reinterpret_cast<float *>(workspace);
    if (p.path == NNC_CBMM_STREAM) {
        const dim3 grid((unsigned)p.col_tiles, (unsigned)p.splits);
        rc = dispatch_stream(p, label_bytes, grid, s, x, (int)m, kdim, labels, ncols, centers_dev, k, bias_dev, relu, direct, out);
        if (rc != NNC_OK) return rc;
        LAUNCHCHK("k_cbmm_stream");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        if (label_bytes == 1)
            hipLaunchKernelGGL(k_cbmm_tiled<uint8_t>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, reinterpret_cast<const uint8_t *>(labels),
                               (long long)ncols, centers_dev, (int)k, p.col_tiles, p.rows_per_split, bias_dev, (int)relu, direct, out);
        else
            hipLaunchKernelGGL(k_cbmm_tiled<uint16_t>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, reinterpret_cast<const uint16_t *>(labels),
                               (long long)ncols, centers_dev, (int)k, p.col_tiles, p.rows_per_split, bias_dev, (int)relu, direct, out);
        LAUNCHCHK("k_cbmm_tiled");
    }
    if (!direct) {
        return cbmm_reduce(reinterpret_cast<const float *>(workspace), p.splits, mn, ncols, bias_dev, relu, y, s);
    }
    return NNC_OK;
}
