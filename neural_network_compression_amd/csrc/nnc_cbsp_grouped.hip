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
// k_cbspg_rowterm, k_cbspg_stream and k_cbspg_combine live in nnc_cbsp_grouped.hpp, templated on the type of x (and of y), with their
// launches: this unit instantiates them for float32, nnc_cbsp_grouped_h16.hip for bf16 / fp16 activations (section 30).
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
#include "nnc_cbsp_grouped.hpp"
#include "nnc_cbtile.hpp"

#define SPG_PLAN_LEN NNC_CBSP_GROUPED_PLAN_LEN

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

// ------------------------------------------------------------------ C ABI
static int spg_grid(long long g) { return (int)std::max(1LL, std::min(cdiv(g, 4), 65536LL)); }

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

extern "C" int64_t nnc_cbsp_grouped_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols)
{
    if (m <= 0 || kdim <= 0 || ncols <= 0 || m > (1LL << 40) || !sp_size_ok(kdim, ncols)) return 0;
    return spg_ws_bytes(sp_plan(m, kdim, ncols, 1, 1, CB_PLAN_CUS), m, ncols);
}

// every k_cbspg_stream instantiation of this unit; the plan is checked against this table, and the launch goes through it
static const SpgStreamCase kSpgStreamCases[] = {SPG_STREAM_CASES(NNC_DT_F32, float)};

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
    const SpPlan p = sp_plan(m, kdim, ncols, 1, k, cu_count());
    if (p.path == NNC_CBMM_BIAS) {   // kdim = 0: y = bias (zeros without one)
        launch_spg_combine<float>(s, nullptr, 0, m, ncols, nullptr, nullptr, bias_dev, relu, y);
        LAUNCHCHK("k_cbspg_combine");
        return NNC_OK;
    }
    const SpgForm f = spg_form(packed, L, nnz, zero_symbols_dev, group_rows, centers_dev, k);
    if (p.path == NNC_CBMM_STREAM) {
        const SpgStreamLaunch fn_stream = find_spg_stream(p.mt);
        if (!fn_stream) return no_spg_stream_case(p.mt);
        return spg_run_stream<float>(fn_stream, p, s, x, m, kdim, f, ncols, bias_dev, relu, y, NNC_DT_F32, workspace);
    }
    const int direct = p.splits == 1;
    float *part = reinterpret_cast<float *>(workspace);
    float *t = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + sp_part_bytes(p, m, ncols));
    uint32_t *applies = reinterpret_cast<uint32_t *>(t + m);
    launch_spg_rowterm<float>(s, x, m, kdim, f, t, applies);
    LAUNCHCHK("k_cbspg_rowterm");
    const dim3 grid((unsigned)(p.col_tiles * p.row_tiles), (unsigned)p.splits);
    hipLaunchKernelGGL(k_cbspg_tiled, grid, dim3(256), (size_t)p.lds, s, x, (long long)m, (long long)kdim, f.bitmap, f.lo, f.hi, f.sym, (long long)nnz,
                       (long long)ncols, L.segs, centers_dev, (int)k, f.zsym, (long long)group_rows, p.col_tiles, p.rows_per_split, t, applies, bias_dev,
                       (int)relu, direct, direct ? y : part);
    LAUNCHCHK("k_cbspg_tiled");
    if (!direct) {
        launch_spg_combine<float>(s, part, p.splits, m, ncols, t, applies, bias_dev, relu, y);
        LAUNCHCHK("k_cbspg_combine");
    }
    return NNC_OK;
}
