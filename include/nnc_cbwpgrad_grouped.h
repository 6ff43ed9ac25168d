/*
 * nnc_cbwpgrad_grouped.h -- the part of the C ABI of libnnc_hip.so that trains the group-wise codebook layer of 17 .. 64 centres per
 * group from its 5- and 6-bit split-plane ("wide packed") indices (csrc/nnc_cbwpgrad_grouped.hip): the backward
 * pass of nnc_cbwp_grouped.  The form, its pack and the NNC_CBWPDX_P_* / NNC_CBWPDC_P_* plan fields are nnc_cbwp.h's and
 * nnc_cbwpgrad.h's, the group-wise contract nnc_cbwp_grouped.h's; this file includes both.
 */
#ifndef NNC_CBWPGRAD_GROUPED_H
#define NNC_CBWPGRAD_GROUPED_H

#include "nnc_cbwpgrad.h"
#include "nnc_cbwp_grouped.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * W[i, o] = centers_dev[i / group_rows][label (i, o)], centers_dev float32[G][k], G = max(1, ceil(kdim / group_rows)), group_rows a
 * positive multiple of 32 (a short last group; group_rows >= kdim is one group), bits 5 (17 <= k <= 32) or 6 (17 <= k <= 64); bits = 9,
 * k > 64 and k <= 16 are NNC_EINVAL as in nnc_cbwp_grouped.  packed, packed_bytes, bits, ncols: the buffer nnc_cbwp_pack wrote for the
 * whole (kdim, ncols) index matrix: a grouped layer has no pack of its own; it is never unpacked and dW is never written.  x_dtype
 * is NNC_DT_F32, NNC_DT_BF16 or NNC_DT_F16, the type of g (and x); with half g every centre is rounded to that type in the table.
 * nnc_cbwp_grouped_dx   dx[r, i] = sum_o g[r, o] * centers_dev[i / group_rows][label (i, o)], dx (m, kdim) of dx_dtype: NNC_DT_F32, or
 *     x_dtype (the float32 value rounded once).  The codebook changes along the output axis of dx.  The plan is nnc_cbwp_dx_plan's.
 *     m <= 16 (NNC_CBMM_STREAM): k_cbwpdx_stream_grouped.  Every wave owns a per-bank table of 2^bits entries x 32 copies and rewrites it
 *         from centres held one per lane when its index row crosses a group boundary; no staging row.  Index row i of dx is, bit for
 *         bit, row i of nnc_cbwp_dx with the one table of i's group.
 *     m > 16, float32 (NNC_CBMM_TILED): k_cbwpdx_tiled_grouped, the tables of the up to four groups a 128-row tile lies in.
 *     m > 16, bf16 / fp16 (NNC_CBMM_MFMA): k_cbwpdx_mfma_grouped; the per-bank copies of the table are divided over the tables of the
 *         tile's groups (COPIES = 32, 16 or 8 a table); dx equals nnc_cbmm_grouped_dx_h16 on the unpacked labels bit for bit.
 * nnc_cbwp_grouped_dc   dc[q][j] = sum over the (i, o) with i / group_rows = q and label j of (x^T g)[i, o], float64[G][k] (out_f64 != 0)
 *     or float32[G][k]: nnc_cbmm_grouped_dc_f32 (float32) / nnc_cbmm_grouped_dc_h16 (half) on the unpacked labels bit for bit at every m
 *     and dtype.  SPLITS, RPS and TERMS_LOG2 are nnc_cbwp_dc_plan's, so the byte form's at label_bytes 1 for the whole layer; the int64
 *     sums are exact and order-independent.  k_cbwpdc_stream_grouped (the bins are one group's, flushed into sums + q * k and cleared at
 *     a boundary), k_cbwpdc_tiled_grouped / k_cbwpdc_mfma_grouped (the 32 copies of a bin cut into HELD per-group sets, COPIES each;
 *     LDS unchanged).  A non-finite x or g, or 2^P > 2^127: all NaN; a zero maximum: dc = 0.
 * A label >= k reads 0 in dx and falls into no bin; the fields and plane bits past ncols form no product and are never binned.  m = 0
 * or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  No float atomics: split partials are float32 in the
 * workspace and are summed in split order.  No host read; the same call gives the same bits.  No load leaves the packed buffer.
 * Argument errors come back before any HIP call: NNC_EINVAL for those of nnc_cbwp_dx / nnc_cbwp_dc and of nnc_cbwp_grouped (bits, k,
 * group_rows), more than 2^30 bins (G * k), a plan without a kernel instantiation; NNC_ENOSPACE for a short workspace (the dc workspace,
 * 64 + 8 * G * k bytes, is 8-byte aligned, the dx one 4-byte).
 * The plans write the NNC_CBWPDX_P_* / NNC_CBWPDC_P_* fields (LDS and COPIES those of the grouped kernels, the dc WORKSPACE that of
 * G * k bins), then GROUP_ROWS, GROUPS (ceil(kdim / group_rows)), ROWS_PER_GROUP (stream: the packed rows of a workgroup; else 0),
 * MAX_GROUPS_PER_WORKGROUP (the most groups the rows of one workgroup lie in) and HELD (dx: the tables held in LDS, four on the stream
 * path, one per wave; dc: the per-group sets of bins), with the meaning nnc_cbpkgrad_grouped.h gives them.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBWPGRAD_GROUPED_P_GROUP_ROWS 15
#define NNC_CBWPGRAD_GROUPED_P_GROUPS 16
#define NNC_CBWPGRAD_GROUPED_P_ROWS_PER_GROUP 17
#define NNC_CBWPGRAD_GROUPED_P_MAX_GROUPS_PER_WORKGROUP 18
#define NNC_CBWPGRAD_GROUPED_P_HELD 19
#define NNC_CBWPGRAD_GROUPED_PLAN_LEN 20
int64_t nnc_cbwp_grouped_dx_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbwp_grouped_dx_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbwp_grouped_dx(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                        const float *centers_dev, int32_t k, int64_t group_rows, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes,
                        void *stream);
int64_t nnc_cbwp_grouped_dc_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows);
int nnc_cbwp_grouped_dc_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbwp_grouped_dc(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                        int64_t ncols, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBWPGRAD_GROUPED_H */
