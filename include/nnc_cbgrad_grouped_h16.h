/*
 * nnc_cbgrad_grouped_h16.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the backward
 * pass of the group-wise codebook layers on bf16 / fp16 activations: byte indices (nnc_cbmm_grouped_*_h16) and 2- / 4-bit packed
 * indices (nnc_cbpk_grouped_*_h16).  The conventions, the error codes, NNC_DT_*, NNC_CBMM_* and the plan fields are nnc.h's and
 * those of nnc_cbgrad_h16.h, nnc_cbgrad_grouped.h, nnc_cbpk_h16.h and nnc_cbpkgrad_grouped.h; include nnc.h, not this file.
 */
#ifndef NNC_CBGRAD_GROUPED_H16_H
#define NNC_CBGRAD_GROUPED_H16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbmm_grouped on bf16 / fp16 x from the same codebooks and indices (csrc/nnc_cbgrad_grouped_h16.hip,
 * DESIGN.md section 26).  x_dtype is NNC_DT_BF16 or NNC_DT_F16, the type of g (and x).
 * W_h[i, o] = rn_dtype(centers_dev[i / group_rows][labels[i * ncols + o]]), exactly the grouped forward's W_h; an index >= k reads 0
 * in dx and falls into no bin in dc.  The index side is nnc_cbmm_grouped's contract (centers_dev float32[G][k] contiguous, 1 <= k <=
 * 256, uint8 labels on any storage offset, group_rows a positive multiple of 32, a short last group, G = max(1, ceil(kdim /
 * group_rows))); the gradient side is nnc_cbmm_dx_h16's / nnc_cbmm_dc_h16's: centers stay float32 and their rounding counts as the
 * identity in the gradient, products are exact, sums float32 in an order fixed by the shape alone, no float atomics, no host read,
 * the same call gives the same bits; g and x contiguous on any 2-byte aligned address.
 * nnc_cbmm_grouped_dx_h16   dx[r, i] = sum_o g[r, o] * W_h[i, o], float32 or x_dtype (dx_dtype).  Row i of dx is, bit for bit, row i
 *                           of nnc_cbmm_dx_h16 on the same labels (label_bytes 1) with the one table of i's group.
 * nnc_cbmm_grouped_dc_h16   dc[q][j] = sum over (i, o) with i / group_rows = q and labels[i, o] = j of dW[i, o], dW = x^T g,
 *                           float64[G][k] (out_f64 != 0) or float32[G][k].  dW is formed, scaled and binned as nnc_cbmm_dc_h16
 *                           does, with that call's S (T is the whole layer's).  The result equals nnc_cbmm_dc_h16 on the 16-bit
 *                           labels q * k + labels[i, o] with G * k bins, bit for bit.  All NaN if x or g holds Inf / NaN or P > 127;
 *                           dc = 0 on a zero maximum.
 * The plans are nnc_cbmm_dx_h16_plan / nnc_cbmm_dc_h16_plan of (x_dtype, m, kdim, ncols, label_bytes 1, k, cus): every field of
 * theirs but the dc WORKSPACE (64 + 8 * G * k bytes, 8-byte aligned) is theirs, TERMS_LOG2 and LDS included.  m <= 16
 * (NNC_CBMM_STREAM): the float32 grouped kernels with the inputs widened as they are loaded, so with float32 output the results
 * equal nnc_cbmm_grouped_dx_f32 / _dc_f32 on the widened inputs (and the centres rounded to x_dtype), bit for bit.  m > 16
 * (NNC_CBMM_MFMA): k_cbdx_mfma / k_cbdc_mfma with the tables / bins of the up to four groups a 128-row tile lies in: the COPIES of
 * the dx table and of the dc bins are divided among HELD tables / sets (COPIES / HELD each), so the LDS does not grow.
 * Behind the NNC_CBDX_H16_* / NNC_CBDC_H16_* fields a plan writes GROUP_ROWS, GROUPS (ceil(kdim / group_rows)), ROWS_PER_GROUP
 * (stream: the label rows of a workgroup; else 0), MAX_GROUPS_PER_WORKGROUP and HELD (MFMA: 4, 2 or 1 at group_rows 32, other, a
 * multiple of 128; else 0): NNC_CBGRAD_GROUPED_H16_PLAN_LEN values.
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  Argument errors come back before any HIP call:
 * NNC_EINVAL for an x_dtype that is not NNC_DT_BF16 / NNC_DT_F16, a dx_dtype that is neither NNC_DT_F32 nor x_dtype, an odd address
 * of g, x or dx, the errors of nnc_cbmm_grouped_dx_f32 / _dc_f32; NNC_ENOSPACE for a short workspace.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBGRAD_GROUPED_H16_P_GROUP_ROWS 13
#define NNC_CBGRAD_GROUPED_H16_P_GROUPS 14
#define NNC_CBGRAD_GROUPED_H16_P_ROWS_PER_GROUP 15
#define NNC_CBGRAD_GROUPED_H16_P_MAX_GROUPS_PER_WORKGROUP 16
#define NNC_CBGRAD_GROUPED_H16_P_HELD 17
#define NNC_CBGRAD_GROUPED_H16_PLAN_LEN 18
int64_t nnc_cbmm_grouped_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols);
int nnc_cbmm_grouped_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, uint64_t labels_addr,
                                 int64_t *out);
int nnc_cbmm_grouped_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int64_t ncols, const float *centers_dev, int32_t k,
                            int64_t group_rows, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream);
int64_t nnc_cbmm_grouped_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows);
int nnc_cbmm_grouped_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, uint64_t labels_addr,
                                 int64_t *out);
int nnc_cbmm_grouped_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *labels, int64_t ncols, int32_t k,
                            int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbpk_grouped on bf16 / fp16 x from the same codebooks and the same packed buffer
 * (csrc/nnc_cbpkgrad_grouped_h16.hip).  The index side is nnc_cbpk_grouped_dx_f32's / _dc_f32's contract (bits 2
 * or 4, 1 <= k <= 2^bits, packed_bytes == nnc_cbpk_pack_bytes(kdim, ncols, bits), packed 16-byte aligned; a label >= k reads 0 in dx
 * and falls into no bin in dc; a padding field past ncols forms no product and is never binned, whatever centers[q][0] is); the
 * gradient side is that of the two entry points above.  Bit for bit, nnc_cbpk_grouped_dx_h16 / _dc_h16 equal
 * nnc_cbmm_grouped_dx_h16 / _dc_h16 on the unpacked labels, and with one group nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16.
 * The plans are nnc_cbpk_dx_h16_plan / nnc_cbpk_dc_h16_plan of (x_dtype, m, kdim, ncols, bits, k, cus).  Their own: the dc WORKSPACE
 * (64 + 8 * G * k bytes); LDS of dx (stream: one table per wave, as nnc_cbpk_grouped_dx_plan; MFMA: HELD whole tables of ENTRIES x
 * COPIES floats and their staging rows) and of dc on the MFMA path (HELD sets of k x 64 bins).  Behind the NNC_CBPKDX_H16_* /
 * NNC_CBPKDC_H16_* fields a plan writes the five group fields above, at the same offsets: NNC_CBGRAD_GROUPED_H16_PLAN_LEN values
 * (HELD on the stream path: 4 tables, one per wave, for dx; 1 set for dc).
 * Argument errors as above, with those of nnc_cbpk_grouped_dx_f32 / _dc_f32.
 * ---------------------------------------------------------------------------------- */
int64_t nnc_cbpk_grouped_dx_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbpk_grouped_dx_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbpk_grouped_dx_h16(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                            const float *centers_dev, int32_t k, int64_t group_rows, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes,
                            void *stream);
int64_t nnc_cbpk_grouped_dc_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows);
int nnc_cbpk_grouped_dc_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbpk_grouped_dc_h16(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                            int64_t ncols, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBGRAD_GROUPED_H16_H */
