// nnc_cbgrad.hpp -- what the backward pass of the codebook matmul (nnc_cbgrad.hip) shares with those of its bitmap-sparse and
// packed siblings (nnc_cbspgrad.hip, nnc_cbpkgrad.hip): the fixed-order wave reduction of the dx stream kernels, the scaling and fixed-point binning of dc (DESIGN.md
// section 12), the workspace sizes and the launches of the kernels both use (defined in nnc_cbgrad.hip).  The tiled kernels' shared
// text is in nnc_cbtile.hpp.
#pragma once
#include "nnc_cbmm.hpp"

#define CBG_FLAG_OK 0
#define CBG_FLAG_NONFINITE 1   // x or g holds Inf / NaN, or m * max|x| * max|g| >= 2^127: dc is NaN
#define CBG_FLAG_ZERO 2        // max|x| or max|g| is 0: every dW is 0
#define CBG_HDR_BYTES 64       // dc workspace: {max|x| bits, max|g| bits, S, flag} then int64 sums[K] at byte 64

// The m partials of every lane summed over the wave: a reduce-scatter (at lane bit 32 >> t the lanes with the bit set keep the upper
// half of the rows they hold and take their partner's; then the rest of the butterfly on one value).  N + log2(64 / N) shuffles
// instead of 6 N; every pair adds in a fixed order, so the sum depends on the data only.  Returns the total of row `row`, the
// same on every lane of a group of 64 / N lanes.  Both candidates of an exchange are read into values before the select: a select
// between two elements of the array is a select between two addresses to the compiler, which at N = 16 keeps the array in scratch.
template <int N>
__device__ __forceinline__ float wave_reduce_rows(float (&v)[N], int lane, int &row)
{
    row = 0;
#pragma unroll
    for (int t = 0; (N >> t) > 1; ++t) {
        const int half = N >> (t + 1), bit = 32 >> t;
        const bool up = (lane & bit) != 0;
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const float a = v[j], b = v[j + half];
            v[j] = (up ? b : a) + __shfl_xor(up ? a : b, bit);
        }
        row += up ? half : 0;
    }
    float s = v[0];
#pragma unroll
    for (int bit = 64 / N / 2; bit >= 1; bit >>= 1) s += __shfl_xor(s, bit);
    return s;
}

// the workspaces of the backward entry points: dx, the partials [splits][m][kdim] when ncols is split; dc, the header and int64 sums[k]
static inline int64_t cbg_dx_ws_bytes(long long splits, long long m, long long kdim) { return splits > 1 ? (int64_t)splits * m * kdim * 4 : 0; }
static inline int64_t cbg_dc_ws_bytes(int path, int k) { return path == NNC_CBMM_STREAM || path == NNC_CBMM_TILED ? CBG_HDR_BYTES + 8LL * k : 0; }

// S of the dc sums from the maxima k_cbgrad_absmax left (uniform over the launch); flag as CBG_FLAG_*
__device__ __forceinline__ int cbdc_shift(const uint32_t *amax, long long m, int terms_log2, int &flag)
{
    const uint32_t ux = amax[0], ug = amax[1];
    flag = CBG_FLAG_OK;
    if (ux >= 0x7F800000u || ug >= 0x7F800000u) {
        flag = CBG_FLAG_NONFINITE;
        return 0;
    }
    const double bound = (double)m * (double)__uint_as_float(ux) * (double)__uint_as_float(ug);
    if (!(bound > 0.0)) {
        flag = CBG_FLAG_ZERO;
        return 0;
    }
    int P = 0;
    (void)frexp(bound, &P);   // bound = f * 2^P, f in [0.5, 1): 2^P > bound
    if (P > 127) {
        flag = CBG_FLAG_NONFINITE;
        return 0;
    }
    return 62 - terms_log2 - P;
}

// e with |v| = f * 2^e, f in [0.5, 1), of a finite non-zero |v| given as bits (subnormals included)
__device__ __forceinline__ int cbdc_exp(uint32_t bits)
{
    const int E = (int)(bits >> 23);
    return E ? E - 126 : (32 - __clz((int)bits)) - 149;
}

// The exponents scx, scg that bring max |x| and max |g| (k_cbgrad_absmax's bits, finite and non-zero: CBG_FLAG_OK) to [0.5, 1).
// The dc kernels scale every x by 2^scx and every g by 2^scg as they load them (v_ldexp_f32: exact, a float32 multiplier cannot
// hold 2^+-149), so dW' = dW * 2^(scx + scg) is formed in float32's normal range whatever the magnitudes; they bin
// rint(dW' * 2^(S - scx - scg)).
__device__ __forceinline__ void cbdc_scales(const uint32_t *amax, int &scx, int &scg)
{
    scx = -cbdc_exp(amax[0]);
    scg = -cbdc_exp(amax[1]);
}

// The loads of the dc kernels are made whatever the guard says (of v[0], which they always have, finite, where it is false) and
// cbdc_scaled(value, guard, s) is value * 2^s, or +-0 (the value * 2^-512) where the guard is false: a guarded load followed by
// the scaling compiles to a branch that waits for each load in turn.  A batch of loads goes first, then a sched_barrier, then
// the scaling, so that the loads of the batch are in flight together.
__device__ __forceinline__ long long cbdc_idx(long long idx, bool ok) { return ok ? idx : 0; }
__device__ __forceinline__ float cbdc_scaled(float v, bool ok, int s) { return ldexpf(v, ok ? s : -512); }

// the fixed-point image of one dW: exact scaling by 2^S (|v * 2^S| < 2^63), nearest integer, ties to even
__device__ __forceinline__ unsigned long long cbdc_fix(float v, int S) { return (unsigned long long)(long long)rintf(ldexpf(v, S)); }

// the workgroup's bins into the global sums (integer atomics), copies summed in order; zero bins are skipped
__device__ __forceinline__ void cbdc_flush(const unsigned long long *bins, int k, int rlog2, unsigned long long *__restrict__ sums)
{
    __syncthreads();
    const int R = 1 << rlog2;
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        unsigned long long s = 0;
        for (int r = 0; r < R; ++r) s += bins[(j << rlog2) + r];
        if (s) atomicAdd(&sums[j], s);
    }
}

// the shared kernels of nnc_cbgrad.hip, launched on `s` (NNC_OK, or the launch error):
//   cbgrad_absmax  amax[0..1] = bits of max |x[0, nx)|, max |g[0, ng)| (amax zeroed by the caller)   k_cbgrad_absmax
//   cbgrad_reduce  out[idx] = sum over s < splits of part[s * mn + idx], in split order                k_cbgrad_reduce
//   cbdc_finish    dc[j] = ldexp(sums[j], -S), float64 or float32; NaN on CBG_FLAG_NONFINITE          k_cbdc_finish
int cbgrad_absmax(const float *x, long long nx, const float *g, long long ng, uint32_t *amax, hipStream_t s);
int cbgrad_reduce(const float *part, long long splits, long long mn, float *out, hipStream_t s);
int cbdc_finish(const uint32_t *hdr, const long long *sums, int k, int f64, void *out, hipStream_t s);
