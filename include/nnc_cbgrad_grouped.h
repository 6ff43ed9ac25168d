/*
 * nnc_cbgrad_grouped.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the backward
 * pass of the group-wise codebook layer.  The conventions, the error codes and the NNC_CBDX_P_* / NNC_CBDC_P_* plan fields are
 * nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBGRAD_GROUPED_H
#define NNC_CBGRAD_GROUPED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbmm_grouped (float32 x) from the same codebooks and indices (csrc/nnc_cbgrad_grouped.hip, DESIGN.md
 * section 19).  W[i, o] = centers_dev[i / group_rows][labels[i * ncols + o]]; the index side is nnc_cbmm_grouped's contract
 * (centers_dev float32[G][k] contiguous, 1 <= k <= 256, uint8 labels on any storage offset, group_rows a positive multiple of 32, a
 * short last group, group_rows >= kdim one group), the gradient side nnc_cbmm_dx_f32's / nnc_cbmm_dc_f32's (float32 throughout, no
 * float atomics, no host read, the result a function of the shape and the data only).  G = max(1, ceil(kdim / group_rows)).
 * nnc_cbmm_grouped_dx_f32   dx[r, i] = sum_o g[r, o] * centers_dev[i / group_rows][labels[i, o]]; an index >= k reads 0.  Row i of
 *                           dx is, bit for bit, row i of nnc_cbmm_dx_f32 on the same labels with the one table of i's group.
 * nnc_cbmm_grouped_dc_f32   dc[q][k] = sum over (i, o) with i / group_rows = q and labels[i, o] = k of dW[i, o], float64[G][k]
 *                           (out_f64 != 0) or float32[G][k].  dW is formed, scaled and binned as nnc_cbmm_dc_f32 does, with that
 *                           call's S: T is the whole layer's ceil(log2(kdim * ncols * splits)), and a group has fewer terms, so
 *                           the 2^63 bound holds a fortiori.  The result equals nnc_cbmm_dc_f32 on the 16-bit labels
 *                           q * k + labels[i, o] with G * k bins, bit for bit.  All NaN if x or g holds Inf / NaN or P > 127; an
 *                           index >= k falls into no bin.
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  Argument errors (those of nnc_cbmm_dx_f32 /
 * nnc_cbmm_dc_f32 at label_bytes 1, those nnc_cbmm_grouped makes of k and group_rows, G * k > 2^30) come back as NNC_EINVAL
 * (NNC_ENOSPACE for a short workspace) before any HIP call.
 * The plans are nnc_cbmm_dx_plan / nnc_cbmm_dc_plan of (m, kdim, ncols, label_bytes 1, k, cus): PATH, VB, MT, SPLITS, CPS / RPS,
 * ALIGNED, COL_TILES, ROW_TILES, TERMS_LOG2 and the dx WORKSPACE are theirs.  Their own: the dc WORKSPACE (64 + 8 * G * k bytes,
 * 8-byte aligned); on the tiled path COPIES and LDS of dx (the tables of the up to four groups a 128-row tile lies in) and COPIES
 * of dc (the copies of a bin in one of the per-group sets the LDS bins are cut into; LDS is unchanged).  Behind the NNC_CBDX_P_* /
 * NNC_CBDC_P_* fields a plan writes GROUP_ROWS, GROUPS (ceil(kdim / group_rows)), ROWS_PER_GROUP (stream: the label rows of a
 * workgroup; else 0) and MAX_GROUPS_PER_WORKGROUP (the most groups the rows of one workgroup lie in): NNC_CBGRAD_GROUPED_PLAN_LEN values.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBGRAD_GROUPED_P_GROUP_ROWS 12
#define NNC_CBGRAD_GROUPED_P_GROUPS 13
#define NNC_CBGRAD_GROUPED_P_ROWS_PER_GROUP 14
#define NNC_CBGRAD_GROUPED_P_MAX_GROUPS_PER_WORKGROUP 15
#define NNC_CBGRAD_GROUPED_PLAN_LEN 16
int64_t nnc_cbmm_grouped_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols);
int nnc_cbmm_grouped_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, uint64_t labels_addr, int64_t *out);
int nnc_cbmm_grouped_dx_f32(const float *g, int64_t m, int64_t kdim, const void *labels, int64_t ncols, const float *centers_dev, int32_t k,
                            int64_t group_rows, float *dx, void *workspace, int64_t workspace_bytes, void *stream);
int64_t nnc_cbmm_grouped_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows);
int nnc_cbmm_grouped_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, uint64_t labels_addr, int64_t *out);
int nnc_cbmm_grouped_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *labels, int64_t ncols, int32_t k, int64_t group_rows,
                            void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBGRAD_GROUPED_H */
