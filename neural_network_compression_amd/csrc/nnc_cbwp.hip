// nnc_cbwp.hip -- the quantized layer of 17 .. 512 centres run from 5-, 6- and 9-bit split-plane ("wide packed") indices
// (include/nnc_cbwp.h).  Inference only.
//
// The form of a (kdim, ncols) index matrix at `bits` = BASE + PLANES: kdim rows of row_bytes = base_bytes + PLANES * plane_bytes;
// a row is its base part (base_bytes = 16 * ceil(ncols * BASE / 128): the low BASE bits of every label, section 14's packed row at
// BASE = 4, a byte per label at BASE = 8) followed by PLANES bit planes of plane_bytes = 16 * ceil(ncols / 128), bit o of plane p =
// bit BASE + p of label (i, o).  Every part starts on a 16-byte boundary and is zero past ncols, so every load below is naturally
// aligned and inside the buffer whenever its first column is inside the matrix.
//
// Kernels, all templated on <BASE, PLANES> = <4, 1> (5 bits), <4, 2> (6 bits), <8, 1> (9 bits):
//   k_cbwp_pack / k_cbwp_unpack  one pass each.  Pack: a thread per dword written, of the base part (8 or 4 labels) or of a plane (32
//                  labels); the base threads count the labels >= 2^bits.  Unpack: a thread per base dword, which also takes its 8 or
//                  4 bits of every plane from the plane dword that holds them.
//   k_cbwp_stream  m <= 16.  A wave owns 64 lanes x VB bytes of a row's base part, so a lane E = 8 * VB / BASE = 4, 8, 16 or 32
//                  consecutive columns, whose plane bits are a nibble, a byte, two bytes or a dword of each plane: one more aligned
//                  load per plane, never a straddle.  U rows of base and plane loads in flight to VGPRs, x[r, i] broadcast by vector
//                  load + v_readlane (cb_load_x).  The table: 2^bits floats (centres, then zeros: a label >= K reads 0) with
//                  per-bank copies (32 at 32 and 64 entries, 16 at 512), one ds_read_b32 per weight; the label is never assembled in
//                  the low bits, every part is shifted straight to its place in the byte address.  The 4 waves of a workgroup split
//                  its rows and are summed in LDS in wave order; workgroups split K.
//   k_cbwp_tiled   m > 16, float32 x: section 10's 128 x 128 tile (nnc_cbtile.hpp); thread t decodes columns (t % 32) * 4 .. + 3 of
//                  row t / 32 from the base dword and the plane dwords that hold them into the LDS W tile, then tb_tile_fma.
//   k_cbwp_mfma    m > 16, bf16 / fp16 x: the MFMA tile and k loop of nnc_cbmfma.hpp; thread t owns column t % 128 of the tile and 16
//                  rows of the k step, per row a byte of the base part and a byte of each plane.
//   the split-K partials are summed by k_cbmm_reduce (cbmm_reduce_dt) in split order.  No float atomics anywhere.
// Columns past ncols are computed from the padding (label 0) in the stream kernel and never stored; in the tiles they are zero.
#include "nnc_cbwp.hpp"
#include "nnc_cbmfma.hpp"
#include "nnc_cbtile.hpp"

extern "C" int64_t nnc_cbwp_pack_bytes(int64_t kdim, int64_t ncols, int bits)
{
    if (kdim < 0 || ncols < 0 || !wp_bits_ok(bits) || !pk_size_ok(kdim, ncols)) return 0;
    return kdim * wp_row_bytes(ncols, bits);
}

// ------------------------------------------------------------------ pack / unpack
__device__ __forceinline__ uint32_t wp_label(const unsigned char *labels, int lb, long long idx)
{
    return lb == 1 ? (uint32_t)labels[idx] : (uint32_t)reinterpret_cast<const uint16_t *>(labels)[idx];
}

// thread -> dword d of row i.  d < base_dwords: the base fields of columns d * PER .. + PER - 1; else dword q of plane p: bit
// BASE + p of columns q * 32 .. + 31.  0 past ncols.
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwp_pack(const unsigned char *__restrict__ labels, int lb, long long kdim, long long ncols, long long base_dwords,
                                                   long long plane_dwords, uint32_t *__restrict__ packed, unsigned int *__restrict__ bad)
{
    constexpr int PER = 32 / BASE;
    constexpr uint32_t MASK = (1u << BASE) - 1;
    const long long row_dwords = base_dwords + PLANES * plane_dwords, total = kdim * row_dwords;
    uint32_t nbad = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long i = t / row_dwords, d = t - i * row_dwords;
        const unsigned char *row = labels + i * ncols * lb;
        uint32_t word = 0;
        if (d < base_dwords) {
            const long long c0 = d * PER;
#pragma unroll
            for (int f = 0; f < PER; ++f) {
                if (c0 + f < ncols) {
                    const uint32_t l = wp_label(row, lb, c0 + f);
                    nbad += (l >> (BASE + PLANES)) != 0;
                    word |= (l & MASK) << (BASE * f);
                }
            }
        } else {
            const int p = (int)((d - base_dwords) / plane_dwords);
            const long long c0 = (d - base_dwords - p * plane_dwords) * 32;
            for (int f = 0; f < 32 && c0 + f < ncols; ++f) word |= ((wp_label(row, lb, c0 + f) >> (BASE + p)) & 1u) << f;
        }
        packed[t] = word;
    }
    if (bad && __any(nbad != 0)) {
        for (int o = 32; o > 0; o >>= 1) nbad += __shfl_down(nbad, o);
        if ((threadIdx.x & 63) == 0) atomicAdd(bad, nbad);
    }
}

// thread -> base dword d of row i: its PER labels, the plane bits from bit d * PER % 32 of plane dword d * PER / 32
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwp_unpack(const uint32_t *__restrict__ packed, long long kdim, long long ncols, long long base_dwords,
                                                     long long plane_dwords, int lb, unsigned char *__restrict__ labels)
{
    constexpr int PER = 32 / BASE;
    constexpr uint32_t MASK = (1u << BASE) - 1;
    const long long row_dwords = base_dwords + PLANES * plane_dwords, total = kdim * base_dwords;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long i = t / base_dwords, d = t - i * base_dwords, c0 = d * PER;
        if (c0 >= ncols) continue;
        const uint32_t *row = packed + i * row_dwords;
        const uint32_t word = row[d];
        uint32_t pl[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = row[base_dwords + p * plane_dwords + c0 / 32] >> (c0 % 32);
#pragma unroll
        for (int f = 0; f < PER; ++f) {
            if (c0 + f < ncols) {
                uint32_t l = (word >> (BASE * f)) & MASK;
#pragma unroll
                for (int p = 0; p < PLANES; ++p) l |= ((pl[p] >> f) & 1u) << (BASE + p);
                if (lb == 1) labels[i * ncols + c0 + f] = (unsigned char)l;
                else reinterpret_cast<uint16_t *>(labels)[i * ncols + c0 + f] = (uint16_t)l;
            }
        }
    }
}

static int wp_check_labels(const char *fn, const void *labels, int label_bytes, int64_t kdim, int64_t ncols)
{
    if (label_bytes != 1 && label_bytes != 2) return fail(NNC_EINVAL, std::string(fn) + ": label_bytes must be 1 or 2");
    if (kdim > 0 && ncols > 0 && !labels) return fail(NNC_EINVAL, std::string(fn) + ": labels is NULL");
    if (label_bytes == 2 && reinterpret_cast<uintptr_t>(labels) % 2) return fail(NNC_EINVAL, std::string(fn) + ": 2-byte labels must be 2-byte aligned");
    return NNC_OK;
}

static int wp_grid(long long dwords) { return (int)std::max(1LL, std::min(cdiv(dwords, 256), 65536LL)); }

extern "C" int nnc_cbwp_pack(const void *labels, int label_bytes, int64_t kdim, int64_t ncols, int bits, void *packed, int64_t packed_bytes,
                             uint32_t *bad_count_dev, void *stream)
{
    int rc = wp_check_form("nnc_cbwp_pack", kdim, ncols, bits);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_labels("nnc_cbwp_pack", labels, label_bytes, kdim, ncols)) != NNC_OK) return rc;
    if ((rc = wp_check_buffer("nnc_cbwp_pack", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (reinterpret_cast<uintptr_t>(bad_count_dev) % 4) return fail(NNC_EINVAL, "nnc_cbwp_pack: bad_count_dev must be 4-byte aligned");
    hipStream_t s = S(stream);
    if (bad_count_dev) HIPCHK(hipMemsetAsync(bad_count_dev, 0, 4, s));
    if (packed_bytes == 0) return NNC_OK;
    const long long bd = wp_base_bytes(ncols, bits) / 4, pd = wp_plane_bytes(ncols) / 4;
#define WP_PACK(B, P) k_cbwp_pack<B, P>
    hipLaunchKernelGGL(WP_BY_BITS(bits, WP_PACK), dim3(wp_grid(kdim * (wp_row_bytes(ncols, bits) / 4))), dim3(256), 0, s,
                       reinterpret_cast<const unsigned char *>(labels), label_bytes, (long long)kdim, (long long)ncols, bd, pd,
                       reinterpret_cast<uint32_t *>(packed), bad_count_dev);
#undef WP_PACK
    LAUNCHCHK("k_cbwp_pack");
    return NNC_OK;
}

extern "C" int nnc_cbwp_unpack(const void *packed, int64_t packed_bytes, int bits, int64_t kdim, int64_t ncols, void *labels_out, int label_bytes_out,
                               void *stream)
{
    int rc = wp_check_form("nnc_cbwp_unpack", kdim, ncols, bits);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_labels("nnc_cbwp_unpack", labels_out, label_bytes_out, kdim, ncols)) != NNC_OK) return rc;
    if (bits > 8 && label_bytes_out != 2) return fail(NNC_EINVAL, "nnc_cbwp_unpack: 9-bit labels need label_bytes_out = 2");
    if ((rc = wp_check_buffer("nnc_cbwp_unpack", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (packed_bytes == 0) return NNC_OK;
    const long long bd = wp_base_bytes(ncols, bits) / 4, pd = wp_plane_bytes(ncols) / 4;
#define WP_UNPACK(B, P) k_cbwp_unpack<B, P>
    hipLaunchKernelGGL(WP_BY_BITS(bits, WP_UNPACK), dim3(wp_grid(kdim * bd)), dim3(256), 0, S(stream), reinterpret_cast<const uint32_t *>(packed),
                       (long long)kdim, (long long)ncols, bd, pd, label_bytes_out, reinterpret_cast<unsigned char *>(labels_out));
#undef WP_UNPACK
    LAUNCHCHK("k_cbwp_unpack");
    return NNC_OK;
}

// ------------------------------------------------------------------ skinny: m <= 16
// grid (col_tiles, splits), CB_THREADS threads.  `out` is y (direct 1: float32, 2: XT; + bias, ReLU here) or the float32 partials
// [split][m][ncols] (direct 0).  base_bytes / plane_bytes: the parts of a row (row_bytes = base_bytes + PLANES * plane_bytes).
template <int BASE, int PLANES, int VB, int MT, typename XT>
__global__ __launch_bounds__(CB_THREADS) void k_cbwp_stream(const XT *__restrict__ x, int m, long long kdim, const unsigned char *__restrict__ packed,
                                                            long long base_bytes, long long plane_bytes, long long ncols,
                                                            const float *__restrict__ centers, int k, long long rows_per_split,
                                                            const float *__restrict__ bias, int relu, int direct, void *__restrict__ out_)
{
    constexpr int BITS = BASE + PLANES, E = 8 * VB / BASE, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BASE, ENTRIES = 1 << BITS;
    constexpr int CSHIFT = BITS == 9 ? 4 : 5;           // wp_cshift(BITS)
    constexpr int SH = CSHIFT + 2;                      // entry l of this lane's copy at byte l << SH
    constexpr uint32_t MASK = (1u << BASE) - 1;
    constexpr int U = E >= 32 ? 4 : CB_UNROLL;          // rows in flight, as k_cbpk_stream
    static_assert(E * MT <= PK_ACC && (E == 4 || E == 8 || E == 16 || E == 32), "columns per lane");
    extern __shared__ float smem[];
    float *cb = smem;                                   // [ENTRIES][1 << CSHIFT]
    float *red = smem + (ENTRIES << CSHIFT);            // [MT * E][64]
    float *stage = red + MT * E * 64;
    float *out = reinterpret_cast<float *>(out_);
    cb_fill<XT>(cb, stage, centers, k, ENTRIES, CSHIFT);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;                     // then the lane's VB base bytes and its plane bits lie inside the padded parts
    const long long s_lo = (long long)blockIdx.y * rows_per_split, s_hi = std::min(kdim, s_lo + rows_per_split);
    const long long per_wave = (s_hi - s_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(s_hi, s_lo + wave * per_wave), i1 = std::min(s_hi, i0 + per_wave);
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *mine = packed + (active ? c0 * BASE / 8 : 0LL);
    const unsigned char *myplane = packed + base_bytes + (active ? c0 / 8 : 0LL);
    const char *tab = reinterpret_cast<const char *>(cb) + ((lane & ((1 << CSHIFT) - 1)) << 2);

    float acc[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[r][e] = 0.0f;
    __syncthreads();

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

    long long i = i0;
    for (; i + U <= i1; i += U) {
        uint32_t w[U][N], pl[U][PLANES];
        float xa, xb;
#pragma unroll
        for (int u = 0; u < U; ++u) load_row(i + u, w[u], pl[u]);
        load_x(i, U, xa, xb);
#pragma unroll
        for (int u = 0; u < U; ++u) consume(w[u], pl[u], xa, xb, u, U);
    }
    for (; i < i1; ++i) {
        uint32_t w[N], pl[PLANES];
        float xa, xb;
        load_row(i, w, pl);
        load_x(i, 1, xa, xb);
        consume(w, pl, xa, xb, 0, 1);
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
// grid (col_tiles * row_tiles, splits), 256 threads, thread (tx, ty) as in k_cbmm_tiled.  Thread t decodes columns c = n0 + (t % 32)
// * 4 .. + 3 of row t / 32 of a TB_K step: the base dword that holds them (4 bits: two threads share a dword; 8 bits: the thread's
// own) and bits c % 32 .. + 3 of dword c / 32 of every plane (eight threads share it).  c is a multiple of 4, so c < ncols puts
// every one of these dwords inside its padded part.
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwp_tiled(const float *__restrict__ x, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                    long long base_bytes, long long plane_bytes, long long ncols, const float *__restrict__ centers, int k,
                                                    long long col_tiles, long long rows_per_split, const float *__restrict__ bias, int relu, int direct,
                                                    float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << (BASE + PLANES);
    constexpr uint32_t MASK = (1u << BASE) - 1;
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]
    float *ws = xs + TB_K * TB_M;          // [TB_K][TB_N]
    float *cb = ws + TB_K * TB_N;          // 2^bits entries (zeros from k on)
    for (int j = threadIdx.x; j < ENTRIES; j += 256) cb[j] = j < k ? centers[j] : 0.0f;

    const TbTile T = tb_tile(col_tiles, rows_per_split, kdim);
    float acc[8][8];
    tb_clear(acc);

    const int wk = threadIdx.x >> 5, wc = (threadIdx.x & 31) * 4;      // W tile: k wk, columns wc..wc+3
    const long long c = T.n0 + wc, row_bytes = base_bytes + PLANES * plane_bytes;
    const long long wbyte = (c * BASE / 32) * 4, pbyte = base_bytes + (c / 32) * 4;
    const int wshift = (int)(c * BASE % 32), pshift = (int)(c % 32);
    for (long long kb = T.lo; kb < T.hi; kb += TB_K) {
        __syncthreads();
        tb_load_rows(xs, x, m, kdim, T.m0, kb, T.hi);
        const long long gk = kb + wk;
        const bool live = gk < T.hi && c < ncols;
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
            ws[wk * TB_N + wc + j] = live ? cb[l] : 0.0f;
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
// grid (col_tiles * row_tiles, splits), HM_THREADS threads: the tile, the k loop and the W lookup of nnc_cbmfma.hpp, the per-bank
// table of 2^bits entries (the centres rounded to XT, zeros from k on).  Thread t owns column gc = n0 + t % 128 of the tile and 16
// rows of the k step; per row the byte of the base part that holds the column's field and the byte of every plane that holds its
// bit, the threads of neighbouring columns reading the same bytes.  A column past ncols loads nothing and is zero in the image.
template <int BASE, int PLANES, typename XT, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbwp_mfma(const XT *__restrict__ x, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                          long long base_bytes, long long plane_bytes, long long ncols, const float *__restrict__ centers,
                                                          int k, long long col_tiles, long long rows_per_split, const float *__restrict__ bias, int relu,
                                                          int direct, void *__restrict__ out_)
{
    constexpr int BITS = BASE + PLANES, ENTRIES = 1 << BITS, CSHIFT = BITS == 9 ? 4 : 5;
    constexpr uint32_t MASK = (1u << BASE) - 1;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, ENTRIES, CSHIFT);
    cb_fill<XT>(L.cb, L.stage, centers, k, ENTRIES, CSHIFT);

    const HmTile T = hm_tile(col_tiles, rows_per_split, kdim);
    const long long gc = T.n0 + T.wc, row_bytes = base_bytes + PLANES * plane_bytes;
    const bool col_ok = gc < ncols;                     // then the column's bytes lie inside the parts
    const unsigned char *bcol = packed + (col_ok ? gc * BASE / 8 : 0LL), *pcol = packed + base_bytes + (col_ok ? gc / 8 : 0LL);
    const int bshift = (int)(gc * BASE % 8), pshift = (int)(gc % 8);
    const long long k_end = col_ok ? T.k_hi : T.k_lo;   // the end of the thread's label rows: none in a column past ncols
    uint32_t lab[16];

    auto load_w = [&](long long kb) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long gk = kb + T.wk0 + j;
            uint32_t l = 0u;
            if (gk < k_end) {
                l = ((uint32_t)bcol[gk * row_bytes] >> bshift) & MASK;
#pragma unroll
                for (int p = 0; p < PLANES; ++p) l |= (((uint32_t)pcol[gk * row_bytes + p * plane_bytes] >> pshift) & 1u) << (BASE + p);
            }
            lab[j] = l;
        }
    };
    auto store_w = [&](long long kb) {
        hm_lookup_w(L.ws, L.cb, T, col_ok, kb, lab, [&](uint32_t l) { return (l << CSHIFT) | (T.lane & ((1 << CSHIFT) - 1)); });
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(x, m, kdim, T, L.xs, L.ws, acc, load_w, store_w);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, ncols, bias, relu, direct, out_);
}

// ------------------------------------------------------------------ launches
template <int BASE, int PLANES, int VB, int MT, typename XT>
static void launch_wp_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, int m, long long kdim, const unsigned char *packed, long long base_bytes,
                             long long plane_bytes, long long ncols, const float *centers, int k, long long rps, const float *bias, int relu, int direct,
                             void *out)
{
    hipLaunchKernelGGL((k_cbwp_stream<BASE, PLANES, VB, MT, XT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x), m, kdim, packed, base_bytes,
                       plane_bytes, ncols, centers, k, rps, bias, relu, direct, out);
}

template <int BASE, int PLANES>
static void launch_wp_tiled(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const unsigned char *packed, long long base_bytes,
                            long long plane_bytes, long long ncols, const float *centers, int k, long long col_tiles, long long rps, const float *bias,
                            int relu, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbwp_tiled<BASE, PLANES>), grid, dim3(256), lds, s, reinterpret_cast<const float *>(x), m, kdim, packed, base_bytes, plane_bytes, ncols,
                       centers, k, col_tiles, rps, bias, relu, direct, reinterpret_cast<float *>(out));
}

template <int BASE, int PLANES, typename XT>
static void launch_wp_mfma(dim3 grid, size_t lds, hipStream_t s, const void *x, long long m, long long kdim, const unsigned char *packed, long long base_bytes,
                           long long plane_bytes, long long ncols, const float *centers, int k, long long col_tiles, long long rps, const float *bias,
                           int relu, int direct, void *out)
{
    hm_launch(x, kdim, k_cbwp_mfma<BASE, PLANES, XT, true>, k_cbwp_mfma<BASE, PLANES, XT, false>, grid, lds, s, reinterpret_cast<const XT *>(x), m, kdim, packed,
              base_bytes, plane_bytes, ncols, centers, k, col_tiles, rps, bias, relu, direct, out);
}

// every instantiation of this unit; the plan is checked against these tables, and the launches go through them
using WpStreamLaunch = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const unsigned char *, long long, long long, long long, const float *,
                                int, long long, const float *, int, int, void *);
using WpTileLaunch = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const unsigned char *, long long, long long, long long,
                              const float *, int, long long, long long, const float *, int, int, void *);
struct WpStreamCase {
    int dt, bits, vb, mt;
    WpStreamLaunch fn;
};
struct WpTileCase {
    int dt, bits;
    WpTileLaunch fn;
};
#define WP_CASE(DT, XT, B, P, V, M) {DT, B + P, V, M, launch_wp_stream<B, P, V, M, XT>}
#define WP_CASES_BASE4(DT, XT, P)                                                                                                                   \
    WP_CASE(DT, XT, 4, P, 16, 1), WP_CASE(DT, XT, 4, P, 16, 2), WP_CASE(DT, XT, 4, P, 8, 1), WP_CASE(DT, XT, 4, P, 8, 2), WP_CASE(DT, XT, 4, P, 8, 4), \
    WP_CASE(DT, XT, 4, P, 4, 1), WP_CASE(DT, XT, 4, P, 4, 2), WP_CASE(DT, XT, 4, P, 4, 4), WP_CASE(DT, XT, 4, P, 4, 8), WP_CASE(DT, XT, 4, P, 2, 16)
#define WP_CASES_BASE8(DT, XT)                                                                                                                      \
    WP_CASE(DT, XT, 8, 1, 16, 1), WP_CASE(DT, XT, 8, 1, 16, 2), WP_CASE(DT, XT, 8, 1, 16, 4), WP_CASE(DT, XT, 8, 1, 8, 1), WP_CASE(DT, XT, 8, 1, 8, 2), \
    WP_CASE(DT, XT, 8, 1, 8, 4), WP_CASE(DT, XT, 8, 1, 8, 8), WP_CASE(DT, XT, 8, 1, 4, 1), WP_CASE(DT, XT, 8, 1, 4, 2), WP_CASE(DT, XT, 8, 1, 4, 4),   \
    WP_CASE(DT, XT, 8, 1, 4, 8), WP_CASE(DT, XT, 8, 1, 4, 16)
#define WP_STREAM_CASES(DT, XT) WP_CASES_BASE4(DT, XT, 1), WP_CASES_BASE4(DT, XT, 2), WP_CASES_BASE8(DT, XT)
static const WpStreamCase kWpStreamCases[] = {WP_STREAM_CASES(NNC_DT_F32, float), WP_STREAM_CASES(NNC_DT_BF16, bf16_t), WP_STREAM_CASES(NNC_DT_F16, f16_t)};
static const WpTileCase kWpTileCases[] = {
    {NNC_DT_F32, 5, launch_wp_tiled<4, 1>},        {NNC_DT_F32, 6, launch_wp_tiled<4, 2>},        {NNC_DT_F32, 9, launch_wp_tiled<8, 1>},
    {NNC_DT_BF16, 5, launch_wp_mfma<4, 1, bf16_t>}, {NNC_DT_BF16, 6, launch_wp_mfma<4, 2, bf16_t>}, {NNC_DT_BF16, 9, launch_wp_mfma<8, 1, bf16_t>},
    {NNC_DT_F16, 5, launch_wp_mfma<4, 1, f16_t>},   {NNC_DT_F16, 6, launch_wp_mfma<4, 2, f16_t>},   {NNC_DT_F16, 9, launch_wp_mfma<8, 1, f16_t>},
};

// the launch of plan p for x of type dt, or nullptr after NNC_EINVAL was recorded: a plan with no instantiation
static bool wp_find(const char *fn, const WpPlan &p, int dt, int bits, WpStreamLaunch &stream, WpTileLaunch &tile)
{
    stream = nullptr, tile = nullptr;
    if (p.path == NNC_CBMM_STREAM) {
        for (const WpStreamCase &c : kWpStreamCases)
            if (c.dt == dt && c.bits == bits && c.vb == p.vb && c.mt == p.mt) stream = c.fn;
    } else if (p.path == NNC_CBMM_TILED || p.path == NNC_CBMM_MFMA) {
        for (const WpTileCase &c : kWpTileCases)
            if (c.dt == dt && c.bits == bits) tile = c.fn;
    } else {
        return true;
    }
    if (stream || tile) return true;
    fail(NNC_EINVAL, std::string(fn) + ": no kernel instantiation for dtype " + std::to_string(dt) + ", bits " + std::to_string(bits) + ", vb " +
                         std::to_string(p.vb) + ", mt " + std::to_string(p.mt));
    return false;
}

// ------------------------------------------------------------------ C ABI
extern "C" int64_t nnc_cbwp_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || wp_check("nnc_cbwp_workspace_bytes", x_dtype, m, kdim, ncols, bits, 1) != NNC_OK) return 0;
    return wp_ws_bytes(wp_plan(x_dtype, m, kdim, ncols, bits, CB_PLAN_CUS), m, ncols);
}

extern "C" int nnc_cbwp_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    const int rc = wp_check("nnc_cbwp_plan", x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbwp_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbwp_plan: out is NULL");
    const WpPlan p = wp_plan(x_dtype, m, kdim, ncols, bits, cus);
    WpStreamLaunch sf;
    WpTileLaunch tf;
    if (!wp_find("nnc_cbwp_plan", p, x_dtype, bits, sf, tf)) return NNC_EINVAL;
    const int64_t v[NNC_CBWP_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, p.base, p.planes, p.copies, p.entries, p.splits, p.rows_per_split,
                                          p.lds, p.col_tiles, p.row_tiles, wp_ws_bytes(p, m, ncols), x_dtype};
    for (int i = 0; i < NNC_CBWP_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbwp(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                        const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, void *y, int y_dtype, void *workspace,
                        int64_t workspace_bytes, void *stream)
{
    int rc = wp_check("nnc_cbwp", x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_buffer("nnc_cbwp", packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if ((rc = cb_check_operands("nnc_cbwp", x, x_dtype, y, y_dtype, centers_dev, m, kdim, ncols, !x, "x")) != NNC_OK) return rc;
    const int64_t need = nnc_cbwp_workspace_bytes(x_dtype, m, kdim, ncols, bits);
    if ((rc = cb_check_workspace("nnc_cbwp", "nnc_cbwp_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK)
        return rc;
    if (m == 0 || ncols == 0) return NNC_OK;

    hipStream_t s = S(stream);
    const long long mn = m * ncols;
    const WpPlan p = wp_plan(x_dtype, m, kdim, ncols, bits, cu_count());
    if (p.path == NNC_CBMM_BIAS) return cbmm_reduce_dt(nullptr, 0, mn, ncols, bias_dev, relu, y, y_dtype, s);   // kdim = 0: y = bias
    WpStreamLaunch sf;
    WpTileLaunch tf;
    if (!wp_find("nnc_cbwp", p, x_dtype, bits, sf, tf)) return NNC_EINVAL;
    const int direct = cb_direct(p.splits, y_dtype);
    void *out = direct ? y : workspace;
    const unsigned char *pk = reinterpret_cast<const unsigned char *>(packed);
    const long long bb = wp_base_bytes(ncols, bits), pb = wp_plane_bytes(ncols);
    if (sf) {
        sf(dim3((unsigned)p.col_tiles, (unsigned)p.splits), (size_t)p.lds, s, x, (int)m, kdim, pk, bb, pb, ncols, centers_dev, k, p.rows_per_split, bias_dev,
           relu, direct, out);
        LAUNCHCHK("k_cbwp_stream");
    } else {
        tf(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, m, kdim, pk, bb, pb, ncols, centers_dev, k, p.col_tiles,
           p.rows_per_split, bias_dev, relu, direct, out);
        LAUNCHCHK((p.path == NNC_CBMM_MFMA ? "k_cbwp_mfma" : "k_cbwp_tiled"));
    }
    return cb_finish(direct, workspace, p.splits, mn, ncols, bias_dev, relu, y, y_dtype, s);
}
