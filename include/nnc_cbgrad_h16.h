/*
 * nnc_cbgrad_h16.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the backward pass
 * of the byte-form codebook layer on bf16 / fp16 activations.  The conventions, the error codes, NNC_DT_*, NNC_CBMM_* and the
 * NNC_CBDX_P_* / NNC_CBDC_P_* plan fields are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBGRAD_H16_H
#define NNC_CBGRAD_H16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbmm_h16 from the same codebook and indices (csrc/nnc_cbgrad_h16.hip).
 * x_dtype is NNC_DT_BF16 or NNC_DT_F16, the type of g (and x).  W_h[i, o] = rn_dtype(centers_dev[labels[i * ncols + o]]), exactly the
 * forward's W_h; an index >= k reads 0 in dx and falls into no bin in dc.  centers_dev stays float32 (master values): the rounding to
 * the dtype is treated as the identity in the gradient, so dc is the gradient with respect to the float32 centres.  A product of two
 * bf16 or two fp16 values is exact in float32; every sum is float32.  g and x are contiguous on any 2-byte aligned address; labels
 * are uint8 or uint16 (label_bytes) on any storage offset.
 * nnc_cbmm_dx_h16   dx = g @ W_h^T, g of x_dtype (m, ncols).  The sums are float32 in an order fixed by the shape alone: the splits of
 *                   ncols are planned for 256 compute units whatever the device and never shrink with more (cus changes only the
 *                   grid of the stream path).  No float atomics: split partials are float32 in the workspace and summed in split
 *                   order.  dx_dtype is NNC_DT_F32, or x_dtype: the float32 value rounded once to nearest even.
 * nnc_cbmm_dc_h16   dc[j] = sum over the (i, o) with labels[i, o] = j of dW[i, o], dW = x^T g, x and g of x_dtype.  dW is formed in
 *                   float32 from exact products, one value per split of m, and binned as nnc_cbmm_dc_f32 bins it: the exact integer
 *                   rint(dW * 2^S), S = 62 - T - P, T = ceil(log2(kdim * ncols * splits)), 2^P > m * max|x| * max|g|, the maxima
 *                   reduced on the device from the widened values.  The int64 sums are exact and order-independent; dc is
 *                   float64[k] (out_f64 != 0) or float32[k].  A non-finite x or g, or P > 127: all NaN.  A zero maximum: dc = 0.
 * Scaling.  fp16 needs none: every product lies in [2^-48, 2^32], and a float32 sum of m <= 2^23 of them is normal, so the fp16
 * kernels bin rint(dW * 2^S) directly (a scaled fp16 operand could become an fp16 subnormal and lose bits).  bf16 has float32's
 * exponent range: on the stream path (m <= 16) x and g are widened and scaled in float32 exactly as nnc_cbmm_dc_f32 scales them; on
 * the MFMA path each bf16 operand is scaled by the same powers of two as it is staged, rn_bf16(ldexpf(float(v), sc)), which is exact
 * for every element whose scaled value is a normal bf16; the others lie 2^-124 or more below the maximum and stay inside the bound
 * of nnc_cbmm_dc_f32, as that entry point's own caveat says.
 * m <= 16 (PATH = NNC_CBMM_STREAM): the plan is nnc_cbmm_dx_plan / nnc_cbmm_dc_plan field for field, the inputs are widened as they
 * are loaded and run the same float32 fmaf chain, so, bit for bit, nnc_cbmm_dx_h16 with float32 dx equals nnc_cbmm_dx_f32 on g
 * widened and the centres rounded to x_dtype and widened, and nnc_cbmm_dc_h16 equals nnc_cbmm_dc_f32 on x and g widened.
 * m > 16 (PATH = NNC_CBMM_MFMA): 128 x 128 tiles on v_mfma_f32_32x32x16_{bf16,f16}; the reduced dimension (ncols for dx, m for dc)
 * is cut into min(ceil(2 * 256 / tiles), floor(extent / 64), 16) splits of a multiple of 32.
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  Argument errors come back before any HIP call:
 * NNC_EINVAL for an x_dtype that is not NNC_DT_BF16 / NNC_DT_F16, a dx_dtype that is neither NNC_DT_F32 nor x_dtype, an odd address,
 * the errors of nnc_cbmm_dx_f32 / nnc_cbmm_dc_f32, a plan without a kernel instantiation; NNC_ENOSPACE for a short workspace (the dc
 * workspace is 8-byte aligned, the dx one 4-byte).  No host read; the same call gives the same bits.
 * The plans write NNC_CBDX_H16_PLAN_LEN / NNC_CBDC_H16_PLAN_LEN values: the NNC_CBDX_P_* / NNC_CBDC_P_* fields, then the dtype.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBDX_H16_P_DTYPE 12
#define NNC_CBDX_H16_PLAN_LEN 13
#define NNC_CBDC_H16_P_DTYPE 12
#define NNC_CBDC_H16_PLAN_LEN 13
int64_t nnc_cbmm_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes);
int nnc_cbmm_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr, int64_t *out);
int nnc_cbmm_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols, const float *centers_dev,
                    int32_t k, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream);
int64_t nnc_cbmm_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k);
int nnc_cbmm_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, uint64_t labels_addr, int64_t *out);
int nnc_cbmm_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int label_bytes, int64_t ncols, int32_t k,
                    void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBGRAD_H16_H */
