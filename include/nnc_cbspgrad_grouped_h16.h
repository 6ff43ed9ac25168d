/*
 * nnc_cbspgrad_grouped_h16.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the backward
 * pass of the pruned group-wise codebook layer on bf16 / fp16 activations, from the bitmap-sparse form of its indices.  The
 * conventions, the error codes, NNC_DT_*, NNC_CBMM_*, the NNC_CBSPDX_P_* / NNC_CBSPDC_P_* plan fields and those of nnc_cbspgrad_h16.h
 * and nnc_cbgrad_grouped_h16.h are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBSPGRAD_GROUPED_H16_H
#define NNC_CBSPGRAD_GROUPED_H16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbsp_grouped_h16 from the same buffer, the indices never unpacked and neither W nor dW written
 * (csrc/nnc_cbspgrad_grouped_h16.hip).  x_dtype is NNC_DT_BF16 or NNC_DT_F16, the type of g (and x).  The form
 * is nnc_cbsp_grouped_pack's, as nnc_cbsp_grouped_dx_f32 / _dc_f32 take it (include/nnc_cbspgrad_grouped.h): G = ceil(kdim /
 * group_rows) groups (one where kdim = 0), group_rows a positive multiple of 32, a short last group; 1 <= k <= 256, uint8 symbols;
 * centers_dev float32[G][k] contiguous; zero_symbols_dev uint8[G] on the device, z_q the skipped symbol of group q, any byte.
 * W_h[i, o] = rn_dtype(centers_dev[q][label[i, o]]), q = i / group_rows, label[i, o] the stored symbol or z_q at a skipped position:
 * exactly the forward's W_h.  A label >= k reads 0 in dx and falls into no bin in dc.  centers_dev stays float32 (master values): the
 * rounding to the dtype counts as the identity in the gradient.  A product of two bf16 or two fp16 values is exact in float32; every
 * sum is float32 in an order fixed by the shape alone; no float atomics, no host read, the same call gives the same bits.  g and x
 * are contiguous on any 2-byte aligned address.
 *
 * nnc_cbsp_grouped_dx_h16   dx = g @ W_h^T, float32 or x_dtype (dx_dtype): the float32 value rounded once to nearest even.
 *     m > 16 (PATH = NNC_CBMM_MFMA): nnc_cbmm_grouped_dx_h16's tile, tables and plan (HELD tables of COPIES / HELD copies each, so the
 *         LDS is that kernel's), the W^T tile decoded from the bitmap and the symbols.  dx equals nnc_cbmm_grouped_dx_h16 on the
 *         unpacked labels (nnc_cbsp_grouped_unpack) bit for bit, for every input.  A skipped weight is an entry of W_h here
 *         (rn(c_{z_q}), or 0 for z_q >= k), not absent: an Inf in g at a skipped position gives NaN as in the byte form.  No row
 *         sums and no rank-1 term on this path.
 *     m <= 16 (PATH = NNC_CBMM_STREAM): nnc_cbsp_grouped_dx_f32's kernel with g widened as it is loaded and the d tables built from
 *         the rounded centres, d_q[s] = rn(c_q[s]) - rn(c_{z_q}); the rank-1 term rn(c_{z_q}) * sum_o g[r, o] is added in float32
 *         before the one rounding of a half dx.  With float32 dx the result equals nnc_cbsp_grouped_dx_f32 on g widened and the
 *         centres rounded to x_dtype and widened, bit for bit; a half dx is that float32 value rounded once.  The kernel writes
 *         float32 partials also with one column block, so the WORKSPACE is max(SPLITS, 1) * m * kdim floats (256-byte aligned
 *         size), then m floats of row sums.
 * nnc_cbsp_grouped_dc_h16   dc[q][j], float64[G][k] (out_f64 != 0) or float32[G][k]: nnc_cbmm_grouped_dc_h16 on the unpacked labels,
 *         bit for bit, at every m (the same main loops and splits of m, the same S; the int64 sums are exact and order-independent).
 *         A skipped position of group q falls into bin (q, z_q), into none if z_q >= k; a stored symbol >= k into none.  m <= 16: the
 *         result is also nnc_cbsp_grouped_dc_f32 on the widened inputs, bit for bit.  All NaN if x or g holds Inf / NaN; dc = 0 on a
 *         zero maximum.
 * With one group both calls equal nnc_cbsp_dx_h16 / nnc_cbsp_dc_h16 (label_bytes 1, zero_symbol z_0) bit for bit.
 *
 * The plans are nnc_cbsp_dx_h16_plan / nnc_cbsp_dc_h16_plan of (x_dtype, m, kdim, ncols, label_bytes 1, k, cus): every
 * NNC_CBSPDX_P_* / NNC_CBSPDC_P_* field and the dtype are theirs but the WORKSPACE (dx on the stream path: above; dc: 64 + 8 * G * k
 * bytes, 8-byte aligned).  Behind them come one reserved 0 and, at the offsets of NNC_CBGRAD_GROUPED_H16_P_*, GROUP_ROWS, GROUPS,
 * ROWS_PER_GROUP (stream: the index rows of a workgroup; else 0), MAX_GROUPS_PER_WORKGROUP and HELD (MFMA: 4, 2 or 1 at group_rows
 * 32, other, a multiple of 128; else 0): NNC_CBSP_GROUPED_GRAD_H16_PLAN_LEN = NNC_CBGRAD_GROUPED_H16_PLAN_LEN values.
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  Argument errors come back before any HIP call:
 * NNC_EINVAL for an x_dtype that is not NNC_DT_BF16 / NNC_DT_F16, a dx_dtype that is neither NNC_DT_F32 nor x_dtype, an odd address
 * of g, x or dx, the errors of nnc_cbsp_grouped_dx_f32 / _dc_f32; NNC_ENOSPACE for a short workspace (dx 4-byte, dc 8-byte aligned).
 * ---------------------------------------------------------------------------------- */
#define NNC_CBSP_GROUPED_GRAD_H16_P_RESERVED 12
#define NNC_CBSP_GROUPED_GRAD_H16_PLAN_LEN 18
int64_t nnc_cbsp_grouped_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols);
int nnc_cbsp_grouped_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbsp_grouped_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                            const void *zero_symbols_dev, int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, void *dx, int dx_dtype,
                            void *workspace, int64_t workspace_bytes, void *stream);
int64_t nnc_cbsp_grouped_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows);
int nnc_cbsp_grouped_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbsp_grouped_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                            const void *zero_symbols_dev, int64_t nnz, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace,
                            int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBSPGRAD_GROUPED_H16_H */
