// nnc_cbpk.hip -- the quantized layer of at most 16 centres run from 2- or 4-bit packed indices (include/nnc.h, nnc_cbpk_*;
// DESIGN.md section 14).
//
// The form of a (kdim, ncols) index matrix at `bits` = 2 or 4: one buffer of kdim rows of row_bytes = 16 * ceil(ncols * bits /
// 128) bytes; label (i, o) in byte i * row_bytes + o * bits / 8 at bit o * bits % 8, low bits first; the fields past ncols are 0.
// Every row starts on a 16-byte boundary: a lane's load of 1..16 bytes is aligned and never leaves the buffer.
//
// Kernels:
//   k_cbpk_pack / k_cbpk_unpack   one pass each, a thread per dword of the packed form (8 or 16 labels), whole-dword stores on
//                  the packed side; the pack counts the labels >= 2^bits (an integer atomic per wave that saw one).
//   k_cbpk_stream  m <= 16: k_cbmm_stream without its unaligned half.  A wave owns 64 lanes x VB bytes of a packed row (VB = 16
//                  .. 1: at most the load whose 8 * VB / BITS columns times the MT rows of x stay within 64 accumulators per
//                  lane; narrower where the shape leaves wide lanes idle or the device short of workgroups, see pk_plan), 8 rows in flight (4 of 16-byte loads) straight to VGPRs, x[r, i] broadcast by vector load + v_readlane.  The table:
//                  2^BITS floats (centres, then zeros) with 32 per-bank copies, 2 KiB or 512 B of LDS, one ds_read_b32 per
//                  weight at byte (label << 7 | (lane & 31) << 2): a shift and an and-or per lookup, no bank conflict.  The 4
//                  waves of a workgroup split its rows and are summed in LDS in wave order; workgroups split K.
//   k_cbpk_tiled   m > 16: the 128 x 128 tile of k_cbmm_tiled (the tile skeleton of nnc_cbtile.hpp); a thread decodes 4 columns
//                  of a tile row from the packed dword that holds them into the LDS W tile, then tb_tile_fma.
//   the split-K partials are summed by k_cbmm_reduce (cbmm_reduce) in split order.  No float atomics anywhere.
// An index >= K reads 0 (the table's zero entries).  Columns past ncols are computed from the padding and never stored.
#include "nnc_cbpk.hpp"
#include "nnc_cbtile.hpp"

// ------------------------------------------------------------------ the layout (host; the arithmetic is nnc_cbpk.hpp's)
extern "C" int64_t nnc_cbpk_row_bytes(int64_t ncols, int bits)
{
    if (ncols < 0 || ncols > (1LL << 40) || !pk_bits_ok(bits)) return 0;
    return pk_row_bytes(ncols, bits);
}

extern "C" int64_t nnc_cbpk_pack_bytes(int64_t kdim, int64_t ncols, int bits)
{
    if (kdim < 0 || ncols < 0 || !pk_bits_ok(bits) || !pk_size_ok(kdim, ncols)) return 0;
    return kdim * pk_row_bytes(ncols, bits);
}

// ------------------------------------------------------------------ pack / unpack
__device__ __forceinline__ uint32_t pk_label(const unsigned char *labels, int lb, long long idx)
{
    return lb == 1 ? (uint32_t)labels[idx] : (uint32_t)reinterpret_cast<const uint16_t *>(labels)[idx];
}

// thread -> dword d of row i: the labels of columns d * PER .. d * PER + PER - 1 (0 past ncols)
template <int BITS>
__global__ __launch_bounds__(256) void k_cbpk_pack(const unsigned char *__restrict__ labels, int lb, long long kdim, long long ncols, long long row_dwords,
                                                   uint32_t *__restrict__ packed, unsigned int *__restrict__ bad)
{
    constexpr int PER = 32 / BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    const long long total = kdim * row_dwords;
    uint32_t nbad = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long i = t / row_dwords, c0 = (t - i * row_dwords) * PER;
        uint32_t word = 0;
#pragma unroll
        for (int f = 0; f < PER; ++f) {
            if (c0 + f < ncols) {
                const uint32_t l = pk_label(labels, lb, i * ncols + c0 + f);
                nbad += l > MASK;
                word |= (l & MASK) << (BITS * f);
            }
        }
        packed[t] = word;
    }
    if (bad && __any(nbad != 0)) {
        for (int o = 32; o > 0; o >>= 1) nbad += __shfl_down(nbad, o);
        if ((threadIdx.x & 63) == 0) atomicAdd(bad, nbad);
    }
}

template <int BITS>
__global__ __launch_bounds__(256) void k_cbpk_unpack(const uint32_t *__restrict__ packed, long long kdim, long long ncols, long long row_dwords, int lb,
                                                     unsigned char *__restrict__ labels)
{
    constexpr int PER = 32 / BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    const long long total = kdim * row_dwords;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long i = t / row_dwords, c0 = (t - i * row_dwords) * PER;
        if (c0 >= ncols) continue;
        const uint32_t word = packed[t];
#pragma unroll
        for (int f = 0; f < PER; ++f) {
            if (c0 + f < ncols) {
                const uint32_t l = (word >> (BITS * f)) & MASK;
                if (lb == 1) labels[i * ncols + c0 + f] = (unsigned char)l;
                else reinterpret_cast<uint16_t *>(labels)[i * ncols + c0 + f] = (uint16_t)l;
            }
        }
    }
}

static int pk_check_labels(const char *fn, const void *labels, int label_bytes, int64_t kdim, int64_t ncols)
{
    if (label_bytes != 1 && label_bytes != 2) return fail(NNC_EINVAL, std::string(fn) + ": label_bytes must be 1 or 2");
    if (kdim > 0 && ncols > 0 && !labels) return fail(NNC_EINVAL, std::string(fn) + ": labels is NULL");
    if (label_bytes == 2 && reinterpret_cast<uintptr_t>(labels) % 2) return fail(NNC_EINVAL, std::string(fn) + ": 2-byte labels must be 2-byte aligned");
    return NNC_OK;
}

static int pk_grid(long long dwords) { return (int)std::max(1LL, std::min(cdiv(dwords, 256), 65536LL)); }

extern "C" int nnc_cbpk_pack(const void *labels, int label_bytes, int64_t kdim, int64_t ncols, int bits, void *packed, int64_t packed_bytes,
                             uint32_t *bad_count_dev, void *stream)
{
    int rc = pk_check_form("nnc_cbpk_pack", kdim, ncols, bits);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_labels("nnc_cbpk_pack", labels, label_bytes, kdim, ncols)) != NNC_OK) return rc;
    if ((rc = pk_check_buffer("nnc_cbpk_pack", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (reinterpret_cast<uintptr_t>(bad_count_dev) % 4) return fail(NNC_EINVAL, "nnc_cbpk_pack: bad_count_dev must be 4-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (bad_count_dev) HIPCHK(hipMemsetAsync(bad_count_dev, 0, 4, s));
    if (packed_bytes == 0) return NNC_OK;
    const long long rd = pk_row_bytes(ncols, bits) / 4;
    const unsigned char *lab = reinterpret_cast<const unsigned char *>(labels);
    if (bits == 4)
        hipLaunchKernelGGL(k_cbpk_pack<4>, dim3(pk_grid(kdim * rd)), dim3(256), 0, s, lab, label_bytes, (long long)kdim, (long long)ncols, rd,
                           reinterpret_cast<uint32_t *>(packed), bad_count_dev);
    else
        hipLaunchKernelGGL(k_cbpk_pack<2>, dim3(pk_grid(kdim * rd)), dim3(256), 0, s, lab, label_bytes, (long long)kdim, (long long)ncols, rd,
                           reinterpret_cast<uint32_t *>(packed), bad_count_dev);
    LAUNCHCHK("k_cbpk_pack");
    return NNC_OK;
}

extern "C" int nnc_cbpk_unpack(const void *packed, int64_t packed_bytes, int bits, int64_t kdim, int64_t ncols, void *labels_out, int label_bytes_out,
                               void *stream)
{
    int rc = pk_check_form("nnc_cbpk_unpack", kdim, ncols, bits);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_labels("nnc_cbpk_unpack", labels_out, label_bytes_out, kdim, ncols)) != NNC_OK) return rc;
    if ((rc = pk_check_buffer("nnc_cbpk_unpack", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (packed_bytes == 0) return NNC_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long rd = pk_row_bytes(ncols, bits) / 4;
    if (bits == 4)
        hipLaunchKernelGGL(k_cbpk_unpack<4>, dim3(pk_grid(kdim * rd)), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(packed), (long long)kdim,
                           (long long)ncols, rd, label_bytes_out, reinterpret_cast<unsigned char *>(labels_out));
    else
        hipLaunchKernelGGL(k_cbpk_unpack<2>, dim3(pk_grid(kdim * rd)), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(packed), (long long)kdim,
                           (long long)ncols, rd, label_bytes_out, reinterpret_cast<unsigned char *>(labels_out));
    LAUNCHCHK("k_cbpk_unpack");
    return NNC_OK;
}

// ------------------------------------------------------------------ skinny: m <= 16
// grid (col_tiles, splits), CB_THREADS threads.  `out` is y (splits == 1: + bias, ReLU here) or the partials [split][m][ncols].
template <int BITS, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS, 2) void k_cbpk_stream(const float *__restrict__ x, int m, long long kdim, const unsigned char *__restrict__ packed,
                                                            long long row_bytes, long long ncols, const float *__restrict__ centers, int k,
                                                            long long rows_per_split, const float *__restrict__ bias, int relu, int direct,
                                                            float *__restrict__ out)
{
    constexpr int E = 8 * VB / BITS, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BITS, ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    constexpr int U = E >= 32 ? 4 : CB_UNROLL;          // rows in flight: a 16-byte row keeps a lane busy for 32 or 64 lookups
    static_assert(E * MT <= PK_ACC, "accumulators per lane");
    extern __shared__ float smem[];
    float *cb = smem;                                   // [ENTRIES][PK_COPIES]
    float *red = smem + ENTRIES * PK_COPIES;            // [MT * E][64]
    float *stage = red + MT * E * 64;
    cb_fill(cb, stage, centers, k, ENTRIES, PK_CSHIFT);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
    __syncthreads();

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

    long long i = i0;
    for (; i + U <= i1; i += U) {
        uint32_t w[U][N];
        float xa, xb;
#pragma unroll
        for (int u = 0; u < U; ++u) pk_load<VB>(mine + (i + u) * row_bytes, w[u]);
        load_x(i, U, xa, xb);
#pragma unroll
        for (int u = 0; u < U; ++u) consume(w[u], xa, xb, u, U);
    }
    for (; i < i1; ++i) {
        uint32_t w[N];
        float xa, xb;
        pk_load<VB>(mine + i * row_bytes, w);
        load_x(i, 1, xa, xb);
        consume(w, xa, xb, 0, 1);
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
// grid (col_tiles * row_tiles, splits), 256 threads, thread (tx, ty) as in k_cbmm_tiled.  The W tile of a TB_K step is TB_K rows
// of TB_N * BITS / 32 packed dwords (a tile starts on a dword: 128 columns are 64 or 32 bytes).  Thread t decodes columns
// (t % 32) * 4 .. + 3 of row t / 32 from the dword that holds them: the 2 (4 bits) or 4 (2 bits) threads of a dword load the same
// address, one request, and all 256 threads share the lookups and the LDS stores.
template <int BITS>
__global__ __launch_bounds__(256) void k_cbpk_tiled(const float *__restrict__ x, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                    long long row_bytes, long long ncols, const float *__restrict__ centers, int k, long long col_tiles,
                                                    long long rows_per_split, const float *__restrict__ bias, int relu, int direct, float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // 2^BITS entries (zeros from k on)
    for (int j = threadIdx.x; j < ENTRIES; j += 256) cb[j] = j < k ? centers[j] : 0.0f;

    const TbTile T = tb_tile(col_tiles, rows_per_split, kdim);
    float acc[8][8];
    tb_clear(acc);

    const int wk = threadIdx.x >> 5, wc = (threadIdx.x & 31) * 4;      // W tile: k wk, columns wc..wc+3
    const long long wbyte = T.n0 * BITS / 8 + (wc * BITS / 32) * 4;
    const int wshift = wc * BITS % 32;
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        __syncthreads();
        tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
        const bool live = gk < T.hi && wbyte < row_bytes;
        const uint32_t word = live ? *reinterpret_cast<const uint32_t *>(packed + gk * row_bytes + wbyte) >> wshift : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[wk * TB_N + wc + j] = live ? cb[(word >> (BITS * j)) & MASK] : 0.0f;
        __syncthreads();
        tb_tile_fma(xs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_y(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, ncols, bias, relu, direct, out);
}

// ------------------------------------------------------------------ C ABI
extern "C" int64_t nnc_cbpk_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || pk_check("nnc_cbpk_workspace_bytes", m, kdim, ncols, bits, 1) != NNC_OK) return 0;
    return pk_ws_bytes(pk_plan(m, kdim, ncols, bits, CB_PLAN_CUS), m, ncols);
}

template <int BITS, int VB, int MT>
static void launch_pk_stream(dim3 grid, size_t lds, hipStream_t s, const float *x, int m, long long kdim, const unsigned char *packed, long long row_bytes,
                             long long ncols, const float *centers, int k, long long rps, const float *bias, int relu, int direct, float *out)
{
    hipLaunchKernelGGL((k_cbpk_stream<BITS, VB, MT>), grid, dim3(CB_THREADS), lds, s, x, m, kdim, packed, row_bytes, ncols, centers, k, rps, bias, relu,
                       direct, out);
}

// every k_cbpk_stream instantiation there is; the plan is checked against this table, and the launch goes through it
using PkStreamLaunch = void (*)(dim3, size_t, hipStream_t, const float *, int, long long, const unsigned char *, long long, long long, const float *, int,
                                long long, const float *, int, int, float *);
struct PkStreamCase {
    int bits, vb, mt;
    PkStreamLaunch fn;
};
#define PK_CASE(B, V, M) {B, V, M, launch_pk_stream<B, V, M>}
static const PkStreamCase kPkStreamCases[] = {
    PK_CASE(4, 16, 1), PK_CASE(4, 16, 2), PK_CASE(4, 8, 1), PK_CASE(4, 8, 2), PK_CASE(4, 8, 4), PK_CASE(4, 4, 1), PK_CASE(4, 4, 2),
    PK_CASE(4, 4, 4),  PK_CASE(4, 4, 8),  PK_CASE(4, 2, 16),
    PK_CASE(2, 16, 1), PK_CASE(2, 8, 1),  PK_CASE(2, 8, 2), PK_CASE(2, 4, 1), PK_CASE(2, 4, 2), PK_CASE(2, 4, 4), PK_CASE(2, 2, 8),
    PK_CASE(2, 1, 16),
};

static PkStreamLaunch find_pk_stream(int bits, int vb, int mt)
{
    for (const PkStreamCase &c : kPkStreamCases)
        if (c.bits == bits && c.vb == vb && c.mt == mt) return c.fn;
    return nullptr;
}

static int no_pk_stream_case(int bits, int vb, int mt)
{
    return fail(NNC_EINVAL, "nnc_cbpk: no k_cbpk_stream instantiation for bits " + std::to_string(bits) + ", vb " + std::to_string(vb) + ", mt " +
                                std::to_string(mt));
}

extern "C" int nnc_cbpk_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    const int rc = pk_check("nnc_cbpk_plan", m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbpk_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbpk_plan: out is NULL");
    const PkPlan p = pk_plan(m, kdim, ncols, bits, cus);
    if (p.path == NNC_CBMM_STREAM && !find_pk_stream(bits, p.vb, p.mt)) return no_pk_stream_case(bits, p.vb, p.mt);
    const int64_t v[NNC_CBPK_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.xrows, p.table, p.copies, p.entries, p.splits, p.rows_per_split,
                                          p.lds, p.col_tiles, p.row_tiles, pk_ws_bytes(p, m, ncols)};
    for (int i = 0; i < NNC_CBPK_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbpk_f32(const float *x, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                            const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, float *y, void *workspace, int64_t workspace_bytes,
                            void *stream)
{
    int rc = pk_check("nnc_cbpk_f32", m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = pk_check_buffer("nnc_cbpk_f32", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbpk_f32: centers is NULL");
    if (m > 0 && ncols > 0 && !y) return fail(NNC_EINVAL, "nnc_cbpk_f32: y is NULL");
    if (m > 0 && ncols > 0 && kdim > 0 && !x) return fail(NNC_EINVAL, "nnc_cbpk_f32: x is NULL");
    const int64_t need = nnc_cbpk_workspace_bytes(m, kdim, ncols, bits);
    if ((rc = cb_check_workspace("nnc_cbpk_f32", "nnc_cbpk_workspace_bytes", workspace, workspace_bytes, need)) != NNC_OK) return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long mn = m * ncols;
    const PkPlan p = pk_plan(m, kdim, ncols, bits, cu_count());
    if (p.path == NNC_CBMM_BIAS) return cbmm_reduce(nullptr, 0, mn, ncols, bias_dev, relu, y, s);   // kdim = 0: y = bias (zeros without one)
    const int direct = p.splits == 1;
    float *out = direct ? y : reinterpret_cast<float *>(workspace);
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long row_bytes = pk_row_bytes(ncols, bits);
    if (p.path == NNC_CBMM_STREAM) {
        const PkStreamLaunch fn = find_pk_stream(bits, p.vb, p.mt);
        if (!fn) return no_pk_stream_case(bits, p.vb, p.mt);
        fn(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, pk, row_bytes, ncols, centers_dev, k, p.rows_per_split,
           bias_dev, relu, direct, out);
        LAUNCHCHK("k_cbpk_stream");
    } else {
        const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
        if (bits == 4)
            hipLaunchKernelGGL(k_cbpk_tiled<4>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, pk, row_bytes, (long long)ncols,
                               centers_dev, (int)k, p.col_tiles, p.rows_per_split, bias_dev, (int)relu, direct, out);
        else
            hipLaunchKernelGGL(k_cbpk_tiled<2>, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, pk, row_bytes, (long long)ncols,
                               centers_dev, (int)k, p.col_tiles, p.rows_per_split, bias_dev, (int)relu, direct, out);
        LAUNCHCHK("k_cbpk_tiled");
    }
    if (!direct) return cbmm_reduce(reinterpret_cast<const float *>(workspace), p.splits, mn, ncols, bias_dev, relu, y, s);
    return NNC_OK;
}
