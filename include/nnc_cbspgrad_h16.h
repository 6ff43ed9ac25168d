/*
 * nnc_cbspgrad_h16.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the backward pass
 * of the bitmap-sparse codebook layer on bf16 / fp16 activations.  The conventions, the error codes, NNC_DT_*, NNC_CBMM_* and the
 * NNC_CBSPDX_P_* / NNC_CBSPDC_P_* plan fields are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBSPGRAD_H16_H
#define NNC_CBSPGRAD_H16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbsp_h16 from the same packed form, the indices never unpacked and W never decoded
 * (csrc/nnc_cbspgrad_h16.hip).  x_dtype is NNC_DT_BF16 or NNC_DT_F16, the type of g (and x).  packed,
 * packed_bytes, label_bytes, zero_symbol, nnz: the form nnc_cbsp_pack wrote, as nnc_cbsp_dx_f32 / nnc_cbsp_dc_f32 take it.
 * W_h[i, o] = rn_dtype(centers_dev[label[i, o]]), label[i, o] the stored symbol, or zero_symbol at a skipped position: exactly the
 * forward's W_h.  An index >= k reads 0 in dx and falls into no bin in dc.  centers_dev stays float32 (master values): the rounding
 * to the dtype is treated as the identity in the gradient, so dc is the gradient with respect to the float32 centres.  A product of
 * two bf16 or two fp16 values is exact in float32; every sum is float32.  g and x are contiguous on any 2-byte aligned address.
 * nnc_cbsp_dx_h16   dx = g @ W_h^T, g of x_dtype (m, ncols); dx_dtype is NNC_DT_F32, or x_dtype: the float32 value rounded once to
 *                   nearest even.  The sums are float32 in an order fixed by the shape alone.  No float atomics: split partials are
 *                   float32 in the workspace and summed in split order.
 *     m <= 16 (PATH = NNC_CBMM_STREAM): nnc_cbsp_dx_f32's plan field for field and its kernels with g widened as it is loaded and
 *         the d table built from the rounded centres, d[s] = rn(c[s]) - rn(c_z); the rank-1 term rn(c_z) * sum_o g[r, o] is added in
 *         float32 before the rounding of a half dx.  With float32 dx the result equals nnc_cbsp_dx_f32 on g widened and the centres
 *         rounded to x_dtype and widened, bit for bit; a skipped weight forms no product when rn(c_z) == 0.
 *     m > 16 (PATH = NNC_CBMM_MFMA): nnc_cbmm_dx_h16's tile, table and plan in every shared field (tiles, splits of ncols, CPS a
 *         multiple of 32, LDS, workspace), with the W^T tile decoded from the bitmap and the symbols; dx equals nnc_cbmm_dx_h16 on
 *         the unpacked labels (nnc_cbsp_unpack) bit for bit, for every input.  The departure from nnc_cbsp_dx_f32: a skipped weight
 *         is an entry of W_h here (rn(c_z), or 0 for zero_symbol >= k), not absent, because a per-element mask cannot be applied
 *         inside an MFMA; an Inf or NaN in g at a column where row i is skipped therefore gives NaN (Inf * 0) in dx[r, i] as in the
 *         byte form, also when c_z == 0, where nnc_cbsp_dx_f32 forms no product.  No row sums and no rank-1 term on this path.
 * nnc_cbsp_dc_h16   dc[k] as nnc_cbmm_dc_h16 on the unpacked labels, bit for bit, at every m: every dW[i, o] is the float32 value that
 *                   call forms (the same kernels' main loops, the same splits of m) and is binned as rint(dW * 2^S) with the same S
 *                   (SPLITS, the bin copies and TERMS_LOG2 are nnc_cbmm_dc_h16_plan's for the shape); the int64 sums are exact and
 *                   order-independent.  A skipped (i, o) falls into bin zero_symbol (none if zero_symbol >= k), a stored index >= k
 *                   into none.  float64[k] (out_f64 != 0) or float32[k]; a non-finite x or g, or P > 127: all NaN; a zero maximum:
 *                   dc = 0.  m <= 16: nnc_cbsp_dc_plan field for field, and the result is also nnc_cbsp_dc_f32 on the widened inputs
 *                   bit for bit.  Scaling as nnc_cbmm_dc_h16: bf16 scaled in float32 on the stream path and as it is staged on the
 *                   MFMA path, fp16 unscaled on the MFMA path.
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  Argument errors come back before any HIP call:
 * NNC_EINVAL for an x_dtype that is not NNC_DT_BF16 / NNC_DT_F16, the errors of nnc_cbsp_dx_f32 / nnc_cbsp_dc_f32, a dx_dtype that is
 * neither NNC_DT_F32 nor x_dtype, an odd address, a plan without a kernel instantiation; NNC_ENOSPACE for a short workspace (the dc
 * workspace is 8-byte aligned, the dx one 4-byte).  No host read; the same call gives the same bits.
 * The plans (host arithmetic; the splits depend on the shape alone, planned for 256 compute units, `cus` changes only the stream
 * grid) write NNC_CBSPDX_H16_PLAN_LEN / NNC_CBSPDC_H16_PLAN_LEN values: the NNC_CBSPDX_P_* / NNC_CBSPDC_P_* fields (MT and SEGS are 0
 * on the MFMA path, COPIES there the copies of the per-bank table / of every bin), then the dtype.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBSPDX_H16_P_DTYPE 11
#define NNC_CBSPDX_H16_PLAN_LEN 12
#define NNC_CBSPDC_H16_P_DTYPE 11
#define NNC_CBSPDC_H16_PLAN_LEN 12
int64_t nnc_cbsp_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes);
int nnc_cbsp_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out);
int nnc_cbsp_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes, int64_t ncols,
                    int32_t zero_symbol, int64_t nnz, const float *centers_dev, int32_t k, void *dx, int dx_dtype, void *workspace,
                    int64_t workspace_bytes, void *stream);
int64_t nnc_cbsp_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k);
int nnc_cbsp_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out);
int nnc_cbsp_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes,
                    int64_t ncols, int32_t zero_symbol, int64_t nnz, int32_t k, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBSPGRAD_H16_H */
