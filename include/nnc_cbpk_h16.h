/*
 * nnc_cbpk_h16.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that runs and trains the 2- and
 * 4-bit packed codebook layer on bf16 / fp16 activations.  The conventions, the error codes, NNC_DT_*, NNC_CBMM_* and the
 * NNC_CBPK_P_* / NNC_CBPKDX_P_* / NNC_CBPKDC_P_* plan fields are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBPK_H16_H
#define NNC_CBPK_H16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * nnc_cbpk_f32's layer and its backward pass on bf16 or fp16 activations (csrc/nnc_cbpk_h16.hip).  x_dtype is
 * NNC_DT_BF16 or NNC_DT_F16, the type of x and g.  packed, packed_bytes, bits, ncols: the form nnc_cbpk_pack wrote, as nnc_cbpk_f32
 * takes it.  W_h[i, o] = rn_dtype(centers_dev[label(i, o)]); a label >= k reads 0 and falls into no bin; a padding field past ncols
 * forms no product and is never binned.  centers_dev and bias_dev stay float32 (master values): the rounding to the dtype is treated
 * as the identity in the gradient.  A product of two bf16 or two fp16 values is exact in float32; every sum is float32.  x and g are
 * contiguous on any 2-byte aligned address.
 * nnc_cbpk_h16      y = x @ W_h + bias, then ReLU (NaN kept); y_dtype is NNC_DT_F32, or x_dtype: the float32 value rounded once.  The
 *                   call is nnc_cbpk_grouped with one group (group_rows = max(32, 32 * ceil(kdim / 32)), centers viewed as (1, k)): at
 *                   every m its bits; at m > 16 (PATH = NNC_CBMM_MFMA) the bits of nnc_cbmm_h16 on the unpacked labels; at m <= 16
 *                   with float32 y the bits of nnc_cbpk_f32 on x widened and the centres rounded to x_dtype and widened.
 * nnc_cbpk_dx_h16   dx = g @ W_h^T, g of x_dtype (m, ncols); dx_dtype is NNC_DT_F32, or x_dtype: the float32 value rounded once.
 *     m <= 16 (PATH = NNC_CBMM_STREAM): nnc_cbpk_dx_plan field for field and k_cbpkdx_stream with g widened as it is loaded and the
 *         table filled from the rounded centres; with float32 dx the bits of nnc_cbpk_dx_f32 on g widened and the centres rounded
 *         to x_dtype and widened.
 *     m > 16 (PATH = NNC_CBMM_MFMA): nnc_cbmm_dx_h16's tile and its plan at label_bytes = 1 in every shared field (tiles, splits of
 *         ncols, CPS a multiple of 32, workspace), the W^T image decoded from the packed row (one 8- or 4-byte load per thread and
 *         step, the 2^bits-entry per-bank table); a column at or past ncols is 0 in the image, whatever centers_dev[0] is.  dx
 *         equals nnc_cbmm_dx_h16 on the unpacked labels bit for bit, for every input.
 * nnc_cbpk_dc_h16   dc[k] as nnc_cbmm_dc_h16 on the unpacked uint8 labels, bit for bit, at every m: every dW[i, o] is the float32
 *                   value that call forms (the same main loop, the same splits of m, the same scaling) and is binned as
 *                   rint(dW * 2^S) with the same S (SPLITS and TERMS_LOG2 are nnc_cbmm_dc_h16_plan's at label_bytes = 1); the int64
 *                   sums are exact and order-independent.  float64[k] (out_f64 != 0) or float32[k]; a non-finite x or g, or
 *                   P > 127: all NaN; a zero maximum: dc = 0.  m <= 16: nnc_cbpk_dc_plan field for field, and the result is also
 *                   nnc_cbpk_dc_f32 on the widened inputs bit for bit.  Every lane adds into its own copy of the LDS bins (COPIES
 *                   = 64) on both paths.
 * m = 0 or ncols = 0: y is empty; kdim = 0: y = bias.  m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension:
 * dc = 0.  Argument errors come back before any HIP call: NNC_EINVAL for an x_dtype that is not NNC_DT_BF16 / NNC_DT_F16, the errors
 * of nnc_cbpk_f32 / nnc_cbpk_dx_f32 / nnc_cbpk_dc_f32, an output dtype that is neither NNC_DT_F32 nor x_dtype, an odd address, a
 * plan without a kernel instantiation; NNC_ENOSPACE for a short workspace (the dc workspace is 8-byte aligned, the others 4-byte).
 * No float atomics: split partials are float32 in the workspace and summed in split order.  No host read; the same call gives the
 * same bits.
 * The plans (host arithmetic; the splits depend on the shape alone, planned for 256 compute units, `cus` changes only the stream
 * grid) write NNC_CBPK_H16_PLAN_LEN / NNC_CBPKDX_H16_PLAN_LEN / NNC_CBPKDC_H16_PLAN_LEN values: the NNC_CBPK_P_* / NNC_CBPKDX_P_* /
 * NNC_CBPKDC_P_* fields (VB, MT and COLS are 0 on the MFMA path, COPIES there the copies of the per-bank table / of every bin), then
 * the dtype.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBPK_H16_P_DTYPE 14
#define NNC_CBPK_H16_PLAN_LEN 15
#define NNC_CBPKDX_H16_P_DTYPE 12
#define NNC_CBPKDX_H16_PLAN_LEN 13
#define NNC_CBPKDC_H16_P_DTYPE 12
#define NNC_CBPKDC_H16_PLAN_LEN 13
int64_t nnc_cbpk_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbpk_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out);
int nnc_cbpk_h16(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                 const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, void *y, int y_dtype, void *workspace,
                 int64_t workspace_bytes, void *stream);
int64_t nnc_cbpk_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbpk_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out);
int nnc_cbpk_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                    const float *centers_dev, int32_t k, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream);
int64_t nnc_cbpk_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k);
int nnc_cbpk_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out);
int nnc_cbpk_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                    int64_t ncols, int32_t k, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBPK_H16_H */
