// nnc_cbwpgrad.hip -- the backward pass of the 5-, 6- and 9-bit split-plane ("wide packed") codebook matmul (nnc_cbwp.hip) from the
// buffer nnc_cbwp_pack wrote: the indices are never unpacked and dW is never written (include/nnc_cbwpgrad.h, nnc_cbwp_dx /
// nnc_cbwp_dc).  With W[i, o] = c[label (i, o)] (a label >= K reads 0), y = x @ W and g = dL/dy:
//
//   dx[r, i] = sum_o g[r, o] * c[label (i, o)]    a column past ncols forms no product: the padding fields hold label 0 and meet a 0
//   dc[k]    = the byte form's call on the unpacked labels, bit for bit: every dW[i, o] is formed as nnc_cbmm_dc_f32 / nnc_cbmm_dc_h16
//              form it (the same loops, splits of m and scaling) and binned as rint(dW * 2^S) with the same S.  Integer sums do not
//              depend on order.  A label >= K falls into no bin; a padding field or plane bit is never binned.
//
// A row of the buffer is its base part (the low BASE bits of every label) followed by PLANES bit planes (nnc_cbwp.hip); every part
// starts on 16 bytes and is zero past ncols.  All six kernels are templated on <BASE, PLANES> = <4, 1>, <4, 2>, <8, 1>:
//   k_cbwpdx_stream  m <= 16.  k_cbpkdx_stream's geometry: a lane owns E = 8 * VB / BASE consecutive columns of g (E * MT <= PKG_G
//                    values in registers); a wave walks index rows with CB_UNROLL base loads in flight and one aligned load per
//                    plane (the lane's plane bits are a nibble, a byte, two bytes or a dword: wp_plane_load).  The table has 2^bits
//                    entries in per-bank copies (wp_cshift); the base field and every plane bit are shifted straight into its byte
//                    address (wp_move).  wave_reduce_rows gives dx[r, i]; column blocks are the splits, summed in block order.
//   k_cbwpdc_stream  m <= 16.  k_cbpkdc_stream's loop (cbdc_load_x / v_readlane, dW' with r ascending, cbdc_fix); K reaches 512,
//                    so the bins keep 1 << dc_rlog2(K) copies (the byte form's rule) and a lane adds into copy lane mod copies.
//   k_cbwpdx_tiled   m > 16, float32.  Section 12's dx tile over W^T; thread t decodes 4 columns of an index row from one base
//                    dword and the matching bits of each plane dword.  Splits of ncols are multiples of 32 columns.
//   k_cbwpdc_tiled   m > 16, float32.  The byte form's dc tile and splits of m; the labels of a thread's accumulators come from
//                    whole dwords of the base part and the planes.
//   k_cbwpdx_mfma    m > 16, bf16 / fp16.  k_cbdx_mfma's tile, loop and splits.  Thread t owns index row n0 + (t mod 128) and 16
//                    consecutive o of the step: one 8- or 16-byte load of the base part and one 2-byte load per plane, all
//                    naturally aligned (a part starts on 16 bytes, a split on a multiple of 32 columns).
//   k_cbwpdc_mfma    m > 16, bf16 / fp16.  dcm_accumulate; in the epilogue the 32 lanes of an accumulator row read 32 consecutive
//                    fields of one packed row: the dword of the lane's base field and the plane dword(s) all 32 share.
// k_cbgrad_absmax, k_cbdc_finish and k_cbgrad_reduce are nnc_cbgrad.hip's; the sequences of HIP calls are cbg_run_dx / cbg_run_dc.
// No load leaves the packed buffer.  No float atomics; no host read.
#include "nnc_cbwpgrad.hpp"
#include "nnc_cbgrad_h16.hpp"

// ------------------------------------------------------------------ dx, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  out: dx (one column block; direct 1: float32, 2: XT) or the float32 partials
// [block][m][kdim].
template <typename XT, int BASE, int PLANES, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbwpdx_stream(const XT *__restrict__ g, int m, long long kdim, const unsigned char *__restrict__ packed,
                                                              long long base_bytes, long long plane_bytes, long long ncols,
                                                              const float *__restrict__ centers, int k, long long rows_per_group, int direct,
                                                              void *__restrict__ out_)
{
    constexpr int BITS = BASE + PLANES, E = 8 * VB / BASE, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BASE, ENTRIES = 1 << BITS;
    constexpr int CSHIFT = BITS == 9 ? 4 : 5;           // wp_cshift(BITS)
    constexpr int SH = CSHIFT + 2;                      // entry l of this lane's copy at byte l << SH
    constexpr uint32_t MASK = (1u << BASE) - 1;
    static_assert(E * MT <= PKG_G && (E == 4 || E == 8 || E == 16 || E == 32), "g values per lane");
    extern __shared__ float smem[];
    float *cb = smem;                                   // [ENTRIES][1 << CSHIFT]
    float *stage = smem + (ENTRIES << CSHIFT);
    float *out = reinterpret_cast<float *>(out_);
    cb_fill<XT>(cb, stage, centers, k, ENTRIES, CSHIFT);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;                     // then the lane's VB base bytes and its plane bits lie inside the padded parts
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));   // the lane's columns inside the matrix
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (r < m && e < ne) ? (float)g[(long long)r * ncols + c0 + e] : 0.0f;

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *mine = packed + (active ? c0 * BASE / 8 : 0LL);
    const unsigned char *myplane = packed + base_bytes + (active ? c0 / 8 : 0LL);
    const char *tab = reinterpret_cast<const char *>(cb) + ((lane & ((1 << CSHIFT) - 1)) << 2);
    float *dst = direct ? out : out + (long long)blockIdx.x * m * kdim;
    __syncthreads();

    auto load_row = [&](long long i, uint32_t *w, uint32_t *pl) {
        pk_load<VB>(mine + i * row_bytes, w);
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = wp_plane_load<E>(myplane + i * row_bytes + p * plane_bytes, lane);
    };
    auto consume = [&](const uint32_t *w, const uint32_t *pl, long long i) {
        float s[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) s[r] = 0.0f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            uint32_t a = wp_move(w[e / PER], BASE * (e % PER), SH, MASK);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) a |= wp_move(pl[p], e, SH + BASE + p, 1u);
            const float wv = e < ne ? *reinterpret_cast<const float *>(tab + a) : 0.0f;   // (columns past the row: no Inf * 0)
#pragma unroll
            for (int r = 0; r < MT; ++r) s[r] = __builtin_fmaf(gv[r][e], wv, s[r]);
        }
        int row;
        const float v = wave_reduce_rows<MT>(s, lane, row);
        if ((lane & (64 / MT - 1)) == 0 && row < m) {
            if (!std::is_same<XT, float>::value && direct == 2)
                reinterpret_cast<XT *>(out_)[(long long)row * kdim + i] = (XT)v;
            else
                dst[(long long)row * kdim + i] = v;
        }
    };

    long long i = i0;
    for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
        uint32_t w[CB_UNROLL][N], pl[CB_UNROLL][PLANES];
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) load_row(i + u, w[u], pl[u]);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], pl[u], i + u);
    }
    for (; i < i1; ++i) {
        uint32_t w[N], pl[PLANES];
        load_row(i, w, pl);
        consume(w, pl, i);
    }
}

// ------------------------------------------------------------------ dc, m <= 16
// grid (column blocks, row groups), CB_THREADS threads.  LDS: the bins, [k][1 << rlog2] int64; a lane adds into copy lane mod copies.
template <typename XT, int BASE, int PLANES, int VB, int MT>
__global__ __launch_bounds__(CB_THREADS) void k_cbwpdc_stream(const XT *__restrict__ x, const XT *__restrict__ g, int m, long long kdim,
                                                              const unsigned char *__restrict__ packed, long long base_bytes, long long plane_bytes,
                                                              long long ncols, int k, int rlog2, int terms_log2, long long rows_per_group,
                                                              uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    constexpr int E = 8 * VB / BASE, N = VB >= 4 ? VB / 4 : 1, PER = 32 / BASE;
    constexpr uint32_t MASK = (1u << BASE) - 1;
    static_assert(E * MT <= PKG_G && (E == 4 || E == 8 || E == 16 || E == 32), "g values per lane");
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
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long c0 = (long long)blockIdx.x * (64 * E) + lane * E;
    const bool active = c0 < ncols;
    const int ne = (int)std::max(0LL, std::min((long long)E, ncols - c0));
    float gv[MT][E];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = (float)g[cbdc_idx((long long)r * ncols + c0 + e, r < m && e < ne)];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) gv[r][e] = cbdc_scaled(gv[r][e], r < m && e < ne, scg);

    const long long g_lo = (long long)blockIdx.y * rows_per_group, g_hi = std::min(kdim, g_lo + rows_per_group);
    const long long per_wave = (g_hi - g_lo + CB_WAVES - 1) / CB_WAVES;
    const long long i0 = std::min(g_hi, g_lo + wave * per_wave), i1 = std::min(g_hi, i0 + per_wave);
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *mine = packed + (active ? c0 * BASE / 8 : 0LL);
    const unsigned char *myplane = packed + base_bytes + (active ? c0 / 8 : 0LL);
    unsigned long long *mybins = bins + (lane & ((1 << rlog2) - 1));
    __syncthreads();

    auto load_row = [&](long long i, uint32_t *w, uint32_t *pl) {
        pk_load<VB>(mine + i * row_bytes, w);
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = wp_plane_load<E>(myplane + i * row_bytes + p * plane_bytes, lane);
    };
    auto load_x = [&](long long i, int U, float &xa, float &xb) { cbdc_load_x<MT>(x, kdim, m, scx, lane, i, U, xa, xb); };
    auto consume = [&](const uint32_t *w, const uint32_t *pl, float xa, float xb, int u, int U) {
        float xv[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            const int f = r * U + u;
            xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f < 64 ? xa : xb), f & 63));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            uint32_t l = (w[e / PER] >> (BASE * (e % PER))) & MASK;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) l |= ((pl[p] >> e) & 1u) << (BASE + p);
            float d = 0.0f;
#pragma unroll
            for (int r = 0; r < MT; ++r) d = __builtin_fmaf(xv[r], gv[r][e], d);   // dW'[i, o], r ascending
            if (e < ne && l < (uint32_t)k) atomicAdd(&mybins[l << rlog2], cbdc_fix(d, Sw));
        }
    };

    long long i = i0;
    for (; i + CB_UNROLL <= i1; i += CB_UNROLL) {
        uint32_t w[CB_UNROLL][N], pl[CB_UNROLL][PLANES];
        float xa, xb;
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) load_row(i + u, w[u], pl[u]);
        load_x(i, CB_UNROLL, xa, xb);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; ++u) consume(w[u], pl[u], xa, xb, u, CB_UNROLL);
    }
    for (; i < i1; ++i) {
        uint32_t w[N], pl[PLANES];
        float xa, xb;
        load_row(i, w, pl);
        load_x(i, 1, xa, xb);
        consume(w, pl, xa, xb, 0, 1);
    }
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ dx, m > 16, float32
// grid (kdim tiles * m tiles, splits of ncols), 256 threads; thread (tx, ty) owns rows ty*8.. (of g) and columns tx*8.. (i) of the
// tile.  Thread t decodes columns c = ob + (t & 1) * 4 .. + 3 of index row n0 + t / 2: the base dword that holds them (c is a multiple
// of 4: 16 bits of a dword at BASE 4, a whole dword at BASE 8) and bits c % 32 .. + 3 of dword c / 32 of every plane.  c < T.hi <= ncols
// puts every one of these dwords inside its padded part.
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwpdx_tiled(const float *__restrict__ g, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                      long long base_bytes, long long plane_bytes, long long ncols, const float *__restrict__ centers,
                                                      int k, long long col_tiles, long long cols_per_split, int direct, float *__restrict__ out)
{
    constexpr int ENTRIES = 1 << (BASE + PLANES);
    extern __shared__ float smem[];
    float *gs = smem;                      // [TB_K][TB_M]: g[m0 + r, o]
    float *ws = gs + TB_K * TB_M;          // [TB_K][TB_N]: W^T[o, n0 + i] = c[label (n0 + i, o)]
    float *cb = ws + TB_K * TB_N;          // 2^bits entries (zeros from k on)
    for (int j = threadIdx.x; j < ENTRIES; j += 256) cb[j] = j < k ? centers[j] : 0.0f;

    const TbTile T = tb_tile(col_tiles, cols_per_split, ncols);
    float acc[8][8];
    tb_clear(acc);

    const int lr = threadIdx.x >> 1, lo = (threadIdx.x & 1) * 4;   // W^T tile: index row n0 + lr, o lo..lo+3
    const long long wi = T.n0 + lr, row_bytes = base_bytes + PLANES * plane_bytes;
    const unsigned char *row = packed + (wi < kdim ? wi * row_bytes : 0LL);
    for (long long ob = T.lo; ob < T.hi; ob += TB_K) {
        __syncthreads();
        tb_load_rows(gs, g, m, ncols, T.m0, ob, T.hi);
        const long long c = ob + lo;
        const bool live = wi < kdim && c < T.hi;
        const uint32_t word = live ? *reinterpret_cast<const uint32_t *>(row + (c * BASE / 32) * 4) : 0u;
        uint32_t pl[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = live ? *reinterpret_cast<const uint32_t *>(row + base_bytes + p * plane_bytes + (c / 32) * 4) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[(lo + j) * TB_N + lr] = (live && c + j < T.hi) ? cb[wg_label<BASE, PLANES>(word, pl, c + j)] : 0.0f;
        __syncthreads();
        tb_tile_fma(gs, ws, T.tx, T.ty, acc);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) tb_store_dx(acc[a][b], T.m0 + T.ty * 8 + a, T.n0 + T.tx * 8 + b, m, kdim, direct, out);
}

// ------------------------------------------------------------------ dc, m > 16, float32
// grid (ncols tiles * kdim tiles, splits of m), 256 threads; thread (tx, ty) forms dW for index rows ty*8.. and columns tx*8.. of the
// 128 x 128 tile over its split's rows of m, then bins the 64 values.  The 8 labels of a row start on a multiple of 8 columns: one
// base dword (BASE 4) or two (BASE 8) and one dword of every plane, inside the padded parts when the column lies inside the matrix.
template <int BASE, int PLANES>
__global__ __launch_bounds__(256) void k_cbwpdc_tiled(const float *__restrict__ x, const float *__restrict__ g, long long m, long long kdim,
                                                      const unsigned char *__restrict__ packed, long long base_bytes, long long plane_bytes,
                                                      long long ncols, int k, int rlog2, int terms_log2, long long col_tiles, long long rows_per_split,
                                                      uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    extern __shared__ float smem[];
    float *xs = smem;                      // [TB_K][TB_M]: x[r, i0 + i]
    float *gs = xs + TB_K * TB_M;          // [TB_K][TB_N]: g[r, o0 + o]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + TB_K * TB_N);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, k << rlog2, scx, scg, Sw)) return;

    const TbTile T = tb_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i
    float acc[8][8];
    tb_clear(acc);
    for (long long rb = T.lo; rb < T.hi; rb += TB_K) {
        __syncthreads();
        cbdc_load_tiles(xs, gs, x, g, kdim, ncols, T.m0, T.n0, rb, T.hi, scx, scg);
        __syncthreads();
        tb_tile_fma(xs, gs, T.tx, T.ty, acc);
    }
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    cbdc_bin_tile(acc, T, kdim, ncols, k, Sw, bins, rlog2, threadIdx.x & ((1 << rlog2) - 1), [&](long long i, long long o) {
        const unsigned char *row = packed + i * row_bytes;
        const uint32_t word = *reinterpret_cast<const uint32_t *>(row + (o * BASE / 32) * 4);
        uint32_t pl[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = *reinterpret_cast<const uint32_t *>(row + base_bytes + p * plane_bytes + (o / 32) * 4);
        return wg_label<BASE, PLANES>(word, pl, o);
    });
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ dx, m > 16, bf16 / fp16
// grid (kdim tiles * m tiles, splits of ncols), HM_THREADS threads; out, direct and cols_per_split as k_cbdx_mfma.  The thread's 16
// columns start at o0 = ob + wk0, a multiple of 16: 8 (BASE 4) or 16 (BASE 8) aligned bytes of the base part, 2 aligned bytes of
// every plane; o0 < k_hi <= ncols puts them inside the padded parts.
template <typename XT, int BASE, int PLANES, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbwpdx_mfma(const XT *__restrict__ g, long long m, long long kdim, const unsigned char *__restrict__ packed,
                                                            long long base_bytes, long long plane_bytes, long long ncols,
                                                            const float *__restrict__ centers, int k, long long col_tiles, long long cols_per_split,
                                                            int direct, void *__restrict__ out_)
{
    constexpr int BITS = BASE + PLANES, ENTRIES = 1 << BITS, CSHIFT = BITS == 9 ? 4 : 5, PER = 32 / BASE, NW = 16 / PER;
    constexpr uint32_t MASK = (1u << BASE) - 1;
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const HmLds<XT> L = hm_lds<XT>(hm_smem, ENTRIES, CSHIFT);   // xs: the g tile, row-major in o; ws: the W^T tile, [i][o]
    cb_fill<XT>(L.cb, L.stage, centers, k, ENTRIES, CSHIFT);

    const HmTile T = hm_tile(col_tiles, cols_per_split, ncols);   // n0: the first index row i, m0: the first row of g, [k_lo, k_hi): columns o
    const long long gi = T.n0 + T.wc, row_bytes = base_bytes + PLANES * plane_bytes;
    const bool row_ok = gi < kdim;
    const unsigned char *prow = packed + (row_ok ? gi * row_bytes : 0LL);
    const float *tab = L.cb + (T.lane & ((1 << CSHIFT) - 1));
    uint32_t lw[NW], pl[PLANES];

    auto load_w = [&](long long ob) {
        const long long o0 = ob + T.wk0;
#pragma unroll
        for (int d = 0; d < NW; ++d) lw[d] = 0u;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) pl[p] = 0u;
        if (row_ok && o0 < T.k_hi) {
            load_chunk<4 * NW>(prow + o0 * BASE / 8, lw);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) pl[p] = *reinterpret_cast<const uint16_t *>(prow + base_bytes + p * plane_bytes + o0 / 8);
        }
    };
    auto store_w = [&](long long ob) {
        float w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint32_t l = (lw[j / PER] >> (BASE * (j % PER))) & MASK;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) l |= ((pl[p] >> j) & 1u) << (BASE + p);
            // a column past the split, so every column past ncols, is 0 and not table[label 0 of the padding]
            w[j] = (row_ok && ob + T.wk0 + j < T.k_hi) ? tab[l << CSHIFT] : 0.0f;
        }
        hm_store_w(L.ws, T.wc, T.wk0, w);
    };

    typename HFrag<XT>::C acc[2][2];
    hm_accumulate<XT, XVEC>(g, m, ncols, T, L.xs, L.ws, acc, load_w, store_w);
    hm_store_y<XT>(acc, T.n0, T.m0, T.wm, T.wn, T.lane, m, kdim, nullptr, 0, direct, out_);
}

// ------------------------------------------------------------------ dc, m > 16, bf16 / fp16
// grid (ncols tiles * kdim tiles, splits of m), HM_THREADS threads.  LDS: the two images, then the bins [k][1 << rlog2] int64.
// rows_per_split and XVEC as k_cbdc_mfma.
template <typename XT, int BASE, int PLANES, bool XVEC>
__global__ __launch_bounds__(HM_THREADS) void k_cbwpdc_mfma(const XT *__restrict__ x, const XT *__restrict__ g, long long m, long long kdim,
                                                            const unsigned char *__restrict__ packed, long long base_bytes, long long plane_bytes,
                                                            long long ncols, int k, int rlog2, int terms_log2, long long col_tiles,
                                                            long long rows_per_split, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ sums)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    XT *xs = reinterpret_cast<XT *>(hm_smem);           // [HM_BM][HM_LD]: x^T tile, [i][r]
    XT *gs = xs + HM_BM * HM_LD;                        // [HM_BN][HM_LD]: g^T tile, [o][r]
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(gs + HM_BN * HM_LD);
    int scx, scg, Sw;
    if (!cbdc_begin(hdr, m, terms_log2, bins, k << rlog2, scx, scg, Sw)) return;   // (uniform over the launch)
    dcm_scales<XT>(scx, scg, Sw);

    const HmTile T = hm_tile(col_tiles, rows_per_split, m);   // n0: the first column o, m0: the first index row i, [k_lo, k_hi): rows r
    typename HFrag<XT>::C acc[2][2];
    dcm_accumulate<XT, XVEC>(x, g, kdim, ncols, T, scx, scg, xs, gs, acc);

    // accumulator (a, b) holds dW'[i][o] (hm_acc_row, hm_acc_col): the 32 lanes of a row read 32 consecutive fields of packed row i,
    // which start on a multiple of 32 columns: the lane's base dword and the plane dwords all 32 share lie inside the padded parts
    // when the lane's column lies inside the matrix
    const long long row_bytes = base_bytes + PLANES * plane_bytes;
    unsigned long long *mybins = bins + (T.lane & ((1 << rlog2) - 1));
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const long long o = hm_acc_col(T.n0 + T.wn, b, T.lane);
            if (o >= ncols) continue;
            const unsigned char *bcol = packed + (o * BASE / 32) * 4, *pcol = packed + base_bytes + (o / 32) * 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = hm_acc_row(T.m0 + T.wm, a, r, T.lane);
                if (i >= kdim) continue;
                uint32_t pl[PLANES];
#pragma unroll
                for (int p = 0; p < PLANES; ++p) pl[p] = *reinterpret_cast<const uint32_t *>(pcol + i * row_bytes + p * plane_bytes);
                const uint32_t l = wg_label<BASE, PLANES>(*reinterpret_cast<const uint32_t *>(bcol + i * row_bytes), pl, o);
                if (l < (uint32_t)k) atomicAdd(&mybins[l << rlog2], cbdc_fix(acc[a][b][r], Sw));
            }
        }
    }
    cbdc_flush(bins, k, rlog2, sums);
}

// ------------------------------------------------------------------ launches
// one signature per direction and path for the three dtypes: g, x and out travel as void * (WgArgs: nnc_cbwpgrad.hpp)

template <typename XT, int BASE, int PLANES, int VB, int MT>
static void launch_dx_stream(dim3 grid, size_t lds, hipStream_t s, const void *g, int m, long long kdim, const WgArgs &w, const float *centers, int k,
                             long long rpg, int direct, void *out)
{
    hipLaunchKernelGGL((k_cbwpdx_stream<XT, BASE, PLANES, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(g), m, kdim, w.packed,
                       w.base_bytes, w.plane_bytes, w.ncols, centers, k, rpg, direct, out);
}

template <typename XT, int BASE, int PLANES, int VB, int MT>
static void launch_dc_stream(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, int m, long long kdim, const WgArgs &w, int k, int rlog2,
                             int tl, long long rpg, uint32_t *hdr, unsigned long long *sums)
{
    hipLaunchKernelGGL((k_cbwpdc_stream<XT, BASE, PLANES, VB, MT>), grid, dim3(CB_THREADS), lds, s, reinterpret_cast<const XT *>(x),
                       reinterpret_cast<const XT *>(g), m, kdim, w.packed, w.base_bytes, w.plane_bytes, w.ncols, k, rlog2, tl, rpg, hdr, sums);
}

template <typename XT, int BASE, int PLANES>
static void launch_dx_tile(dim3 grid, size_t lds, hipStream_t s, const void *g, long long m, long long kdim, const WgArgs &w, const float *centers, int k,
                           long long col_tiles, long long cps, int direct, void *out)
{
    if constexpr (std::is_same<XT, float>::value)
        hipLaunchKernelGGL((k_cbwpdx_tiled<BASE, PLANES>), grid, dim3(256), lds, s, reinterpret_cast<const float *>(g), m, kdim, w.packed, w.base_bytes,
                           w.plane_bytes, w.ncols, centers, k, col_tiles, cps, direct, reinterpret_cast<float *>(out));
    else
        hm_launch(g, w.ncols, k_cbwpdx_mfma<XT, BASE, PLANES, true>, k_cbwpdx_mfma<XT, BASE, PLANES, false>, grid, lds, s, reinterpret_cast<const XT *>(g), m,
                  kdim, w.packed, w.base_bytes, w.plane_bytes, w.ncols, centers, k, col_tiles, cps, direct, out);
}

template <typename XT, int BASE, int PLANES>
static void launch_dc_tile(dim3 grid, size_t lds, hipStream_t s, const void *x, const void *g, long long m, long long kdim, const WgArgs &w, int k,
                           int rlog2, int tl, long long col_tiles, long long rps, uint32_t *hdr, unsigned long long *sums)
{
    if constexpr (std::is_same<XT, float>::value)
        hipLaunchKernelGGL((k_cbwpdc_tiled<BASE, PLANES>), grid, dim3(256), lds, s, reinterpret_cast<const float *>(x), reinterpret_cast<const float *>(g), m,
                           kdim, w.packed, w.base_bytes, w.plane_bytes, w.ncols, k, rlog2, tl, col_tiles, rps, hdr, sums);
    else
        hipLaunchKernelGGL((dcm_xvec(x, g, kdim, w.ncols) ? k_cbwpdc_mfma<XT, BASE, PLANES, true> : k_cbwpdc_mfma<XT, BASE, PLANES, false>), grid,
                           dim3(HM_THREADS), lds, s, reinterpret_cast<const XT *>(x), reinterpret_cast<const XT *>(g), m, kdim, w.packed, w.base_bytes,
                           w.plane_bytes, w.ncols, k, rlog2, tl, col_tiles, rps, hdr, sums);
}

// every kernel instantiation of this unit: a table of the stream ones (the list of nnc_cbwpgrad.hpp) per dtype and one of the tiles
// (the float32 tile or the MFMA tile, by dtype); the plans are checked against these tables, and the launches go through them
using WgDxStream = void (*)(dim3, size_t, hipStream_t, const void *, int, long long, const WgArgs &, const float *, int, long long, int, void *);
using WgDcStream = void (*)(dim3, size_t, hipStream_t, const void *, const void *, int, long long, const WgArgs &, int, int, int, long long, uint32_t *,
                            unsigned long long *);
using WgDxTile = void (*)(dim3, size_t, hipStream_t, const void *, long long, long long, const WgArgs &, const float *, int, long long, long long, int,
                          void *);
using WgDcTile = void (*)(dim3, size_t, hipStream_t, const void *, const void *, long long, long long, const WgArgs &, int, int, int, long long, long long,
                          uint32_t *, unsigned long long *);
struct WgStreamCase {
    int a, vb, mt;            // a: bits
    WgDxStream dx;
    WgDcStream dc;
};
struct WgTileCase {
    int dt, a;                // a: bits
    WgDxTile dx;
    WgDcTile dc;
};
#define WG_F32(B, P, V, M) {B + P, V, M, launch_dx_stream<float, B, P, V, M>, launch_dc_stream<float, B, P, V, M>},
#define WG_BF16(B, P, V, M) {B + P, V, M, launch_dx_stream<bf16_t, B, P, V, M>, launch_dc_stream<bf16_t, B, P, V, M>},
#define WG_F16(B, P, V, M) {B + P, V, M, launch_dx_stream<f16_t, B, P, V, M>, launch_dc_stream<f16_t, B, P, V, M>},
static const WgStreamCase kWgF32Cases[] = {WPG_STREAM_CASES(WG_F32)};
static const WgStreamCase kWgBf16Cases[] = {WPG_STREAM_CASES(WG_BF16)};
static const WgStreamCase kWgF16Cases[] = {WPG_STREAM_CASES(WG_F16)};
#undef WG_F32
#undef WG_BF16
#undef WG_F16
#define WG_TILES(DT, XT) {DT, 5, launch_dx_tile<XT, 4, 1>, launch_dc_tile<XT, 4, 1>}, {DT, 6, launch_dx_tile<XT, 4, 2>, launch_dc_tile<XT, 4, 2>}, \
                         {DT, 9, launch_dx_tile<XT, 8, 1>, launch_dc_tile<XT, 8, 1>}
static const WgTileCase kWgTileCases[] = {WG_TILES(NNC_DT_F32, float), WG_TILES(NNC_DT_BF16, bf16_t), WG_TILES(NNC_DT_F16, f16_t)};
#undef WG_TILES
static const CbgCaseNames kWgNames = {false, "bits", true};

// The instantiations plan p asks for: sc on the stream path, tc on a tile path (NNC_EINVAL and a message if a table has none), both
// NULL on the paths that launch nothing of this unit.
static int wg_find(const char *fn, const PgPlan &p, int dt, int bits, const WgStreamCase *&sc, const WgTileCase *&tc)
{
    tc = nullptr;
    const int rc = cbg_stream_case(fn, wg_cases(dt, kWgF32Cases, kWgBf16Cases, kWgF16Cases), kWgNames, p.path, bits, p.vb, p.mt, sc);
    if (rc != NNC_OK || (p.path != NNC_CBMM_TILED && p.path != NNC_CBMM_MFMA)) return rc;
    for (const WgTileCase &c : kWgTileCases)
        if (c.dt == dt && c.a == bits) tc = &c;
    if (tc) return NNC_OK;
    return fail(NNC_EINVAL, std::string(fn) + ": no tile instantiation for dtype " + std::to_string(dt) + ", bits " + std::to_string(bits));
}

// ------------------------------------------------------------------ C ABI
extern "C" int64_t nnc_cbwp_dx_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits)
{
    if (wg_check("nnc_cbwp_dx_workspace_bytes", x_dtype, m, kdim, ncols, bits, 1) != NNC_OK) return 0;
    return cbg_dx_ws_bytes(wg_dx_plan(x_dtype, m, kdim, ncols, bits, CB_PLAN_CUS).splits, m, kdim);
}

extern "C" int nnc_cbwp_dx_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbwp_dx_plan";
    int rc = wg_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbwp_dx_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbwp_dx_plan: out is NULL");
    const PgPlan p = wg_dx_plan(x_dtype, m, kdim, ncols, bits, cus);
    const WgStreamCase *sc;
    const WgTileCase *tc;
    if ((rc = wg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    const bool none = p.path == NNC_CBMM_NONE || p.path == NNC_CBMM_ZERO;
    const int64_t v[NNC_CBWPDX_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, none ? 0 : wp_base(bits), none ? 0 : bits - wp_base(bits), p.copies, p.entries,
                                            p.splits, p.per_split, p.lds, p.col_tiles, p.row_tiles, cbg_dx_ws_bytes(p.splits, m, kdim), x_dtype};
    for (int i = 0; i < NNC_CBWPDX_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbwp_dx(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                           const float *centers_dev, int32_t k, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbwp_dx";
    int rc = wg_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (dx_dtype != NNC_DT_F32 && dx_dtype != x_dtype) return fail(NNC_EINVAL, "nnc_cbwp_dx: dx_dtype must be NNC_DT_F32 or x_dtype");
    if (!centers_dev) return fail(NNC_EINVAL, "nnc_cbwp_dx: centers is NULL");
    if (m > 0 && kdim > 0 && !dx) return fail(NNC_EINVAL, "nnc_cbwp_dx: dx is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && !g) return fail(NNC_EINVAL, "nnc_cbwp_dx: g is NULL");
    if (reinterpret_cast<uintptr_t>(g) % (x_dtype == NNC_DT_F32 ? 4 : 2) || reinterpret_cast<uintptr_t>(dx) % (dx_dtype == NNC_DT_F32 ? 4 : 2))
        return fail(NNC_EINVAL, "nnc_cbwp_dx: g or dx is not aligned to its element size");
    const int64_t need = nnc_cbwp_dx_workspace_bytes(x_dtype, m, kdim, ncols, bits);
    if ((rc = cb_check_workspace(fn, "nnc_cbwp_dx_workspace_bytes", workspace, workspace_bytes, need, 4, "workspace must be 4-byte aligned")) != NNC_OK) return rc;
    PgPlan p = wg_dx_plan(x_dtype, m, kdim, ncols, bits, CB_PLAN_CUS);
    const WgStreamCase *sc;
    const WgTileCase *tc;
    if ((rc = wg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM) p = wg_dx_plan(x_dtype, m, kdim, ncols, bits, cu_count());   // (the row groups of this device)
    const WgArgs w = {reinterpret_cast<const unsigned char *>(packed), wp_base_bytes(ncols, bits), wp_plane_bytes(ncols), ncols};
    return cbg_run_dx(p.path, p.splits, m, kdim, dx, dx_dtype, workspace, s, [&](int direct, void *out) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dx(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, g, (int)m, kdim, w, centers_dev, k, p.rows_per_group, direct, out);
            LAUNCHCHK("k_cbwpdx_stream");
        } else {
            tc->dx(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, g, m, kdim, w, centers_dev, k, p.col_tiles, p.per_split,
                   direct, out);
            LAUNCHCHK((p.path == NNC_CBMM_MFMA ? "k_cbwpdx_mfma" : "k_cbwpdx_tiled"));
        }
        return NNC_OK;
    });
}

extern "C" int64_t nnc_cbwp_dc_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    if (wg_check("nnc_cbwp_dc_workspace_bytes", x_dtype, m, kdim, ncols, bits, k) != NNC_OK) return 0;
    PgPlan p;
    if (wg_dc_plan(x_dtype, m, kdim, ncols, bits, k, CB_PLAN_CUS, p) != NNC_OK) return 0;
    return h16_dc_ws_bytes(p.path, k);
}

extern "C" int nnc_cbwp_dc_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out)
{
    const char *fn = "nnc_cbwp_dc_plan";
    int rc = wg_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if (cus < 1) return fail(NNC_EINVAL, "nnc_cbwp_dc_plan: cus < 1");
    if (!out) return fail(NNC_EINVAL, "nnc_cbwp_dc_plan: out is NULL");
    PgPlan p;
    if ((rc = wg_dc_plan(x_dtype, m, kdim, ncols, bits, k, cus, p)) != NNC_OK) return rc;
    const WgStreamCase *sc;
    const WgTileCase *tc;
    if ((rc = wg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    const bool zero = p.path == NNC_CBMM_ZERO;
    const int64_t v[NNC_CBWPDC_PLAN_LEN] = {p.path, p.vb, p.mt, p.cols, zero ? 0 : wp_base(bits), zero ? 0 : bits - wp_base(bits), p.copies, p.splits,
                                            p.per_split, p.lds, p.col_tiles, p.row_tiles, p.terms_log2, h16_dc_ws_bytes(p.path, k), x_dtype};
    for (int i = 0; i < NNC_CBWPDC_PLAN_LEN; ++i) out[i] = v[i];
    return NNC_OK;
}

extern "C" int nnc_cbwp_dc(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                           int64_t ncols, int32_t k, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "nnc_cbwp_dc";
    int rc = wg_check(fn, x_dtype, m, kdim, ncols, bits, k);
    if (rc != NNC_OK) return rc;
    if ((rc = wp_check_buffer(fn, packed, packed_bytes, kdim, ncols, bits)) != NNC_OK) return rc;
    if (!dc) return fail(NNC_EINVAL, "nnc_cbwp_dc: dc is NULL");
    if (m > 0 && kdim > 0 && ncols > 0 && (!x || !g)) return fail(NNC_EINVAL, "nnc_cbwp_dc: x or g is NULL");
    const int eb = x_dtype == NNC_DT_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(x) % eb || reinterpret_cast<uintptr_t>(g) % eb) return fail(NNC_EINVAL, "nnc_cbwp_dc: x or g is not aligned to its element size");
    PgPlan p;
    if ((rc = wg_dc_plan(x_dtype, m, kdim, ncols, bits, k, CB_PLAN_CUS, p)) != NNC_OK) return rc;
    const int64_t need = h16_dc_ws_bytes(p.path, k);
    if ((rc = cb_check_workspace(fn, "nnc_cbwp_dc_workspace_bytes", workspace, workspace_bytes, need, 8, "workspace not 8-byte aligned")) != NNC_OK) return rc;
    const WgStreamCase *sc;
    const WgTileCase *tc;
    if ((rc = wg_find(fn, p, x_dtype, bits, sc, tc)) != NNC_OK) return rc;
    hipStream_t s = S(stream);
    if (p.path == NNC_CBMM_STREAM && (rc = wg_dc_plan(x_dtype, m, kdim, ncols, bits, k, cu_count(), p)) != NNC_OK) return rc;   // (the row groups of this device)
    const WgArgs w = {reinterpret_cast<const unsigned char *>(packed), wp_base_bytes(ncols, bits), wp_plane_bytes(ncols), ncols};
    const int rlog2 = dc_rlog2(k);
    return cbg_run_dc(p.path, x, g, x_dtype, m, kdim, ncols, (int)k, dc, out_f64, workspace, need, s, [&](uint32_t *hdr, unsigned long long *sums) {
        if (p.path == NNC_CBMM_STREAM) {
            sc->dc(dim3((unsigned)p.col_tiles, (unsigned)p.row_tiles), (size_t)p.lds, s, x, g, (int)m, kdim, w, k, rlog2, p.terms_log2, p.rows_per_group, hdr,
                   sums);
            LAUNCHCHK("k_cbwpdc_stream");
        } else {
            tc->dc(dim3((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits), (size_t)p.lds, s, x, g, m, kdim, w, k, rlog2, p.terms_log2, p.col_tiles,
                   p.per_split, hdr, sums);
            LAUNCHCHK((p.path == NNC_CBMM_MFMA ? "k_cbwpdc_mfma" : "k_cbwpdc_tiled"));
        }
        return NNC_OK;
    });
}
