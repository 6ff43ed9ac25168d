/*
 * nnc_cbspgrad_grouped.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the backward
 * pass of the pruned group-wise codebook layer from the bitmap-sparse form of its indices.  The conventions, the error codes and the
 * NNC_CBSPDX_P_* / NNC_CBSPDC_P_* plan fields are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBSPGRAD_GROUPED_H
#define NNC_CBSPGRAD_GROUPED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbsp_grouped_f32 (float32 x and g) from the same buffer, the indices never unpacked and neither W nor dW
 * written (csrc/nnc_cbspgrad_grouped.hip).  The form is nnc_cbsp_grouped_pack's (include/nnc_cbsp_grouped.h):
 * G = ceil(kdim / group_rows) groups (one where kdim = 0: centers and dc always have a row), group_rows a positive multiple of 32, a
 * short last group, group_rows >= kdim one group; 1 <= k <= 256, uint8 symbols; centers_dev float32[G][k] contiguous;
 * zero_symbols_dev uint8[G] on the device, z_q the skipped symbol of group q, any byte (z_q >= k: c_{z_q} = 0).  With q = i /
 * group_rows, c_{z_q} = c_q[z_q], d_q[s] = float32(c_q[s] - c_{z_q}) for s < k and -c_{z_q} for s >= k, g = dL/dy float32[m][ncols]:
 *
 * nnc_cbsp_grouped_dx_f32   dx[r, i] = c_{z_q} * sum_o g[r, o] + sum over the stored (i, o) of g[r, o] * d_q[label]: the Jacobian of
 *                           nnc_cbsp_grouped_f32 with its conventions.  Where c_{z_q} == 0 exactly the rank-1 term is dropped for
 *                           the columns of group q (the test is c != 0, so a NaN centre counts); a skipped weight forms no
 *                           product, so an Inf in g at a column where row i is skipped gives no NaN in dx[., i] then.  The row sums
 *                           rs[r] = sum_o g[r, o] come from one pass ahead of the main kernel (nnc_cbsp_dx_f32's) and serve every
 *                           group; the last kernel adds dx[r, i] = c_{z_q} * rs[r] + dx[r, i].
 * nnc_cbsp_grouped_dc_f32   dc[q][j], float64[G][k] (out_f64 != 0) or float32[G][k]: nnc_cbmm_grouped_dc_f32 on the unpacked labels
 *                           (nnc_cbsp_grouped_unpack), bit for bit.  A skipped position of group q falls into bin (q, z_q), into none
 *                           if z_q >= k; a stored symbol >= k falls into none.  All NaN if x or g holds Inf / NaN; dc = 0 where
 *                           max |x| or max |g| is 0.
 *
 * Two identities, bit for bit on any float data, follow from the plans being the ungrouped ones:
 *   1. dx, group by group: a row of dx depends on its own bitmap words, symbols, table and z only, and in the rows of group q the
 *      grouped bit rule is nnc_cbsp_pack's for zero_symbol = z_q.  So the columns of dx that are the rows of group q equal those
 *      nnc_cbsp_dx_f32 gives on the same buffer at label_bytes 1 with zero_symbol = z_q and the one table centers_dev[q], at every m
 *      (the other columns of that call mean nothing).
 *   2. dc equals nnc_cbmm_grouped_dc_f32 on the unpacked labels: every dW is the same float32 value (the same scales, the same fmaf
 *      chain or tile, the same splits of m) and the shift S is the same (T is the whole layer's, from nnc_cbmm_dc_plan).
 * With one group both calls equal nnc_cbsp_dx_f32 / nnc_cbsp_dc_f32 bit for bit.
 *
 * The plans are nnc_cbsp_dx_plan / nnc_cbsp_dc_plan of (m, kdim, ncols, label_bytes 1, k, cus): every NNC_CBSPDX_P_* /
 * NNC_CBSPDC_P_* field is theirs, with two exceptions: the tiled dx LDS grows by (TABLES - 1) * (k + 1) words (the tables of the up
 * to four groups a 128-row tile lies in), and the dc WORKSPACE is 64 + 8 * G * k bytes (8-byte aligned).  The dx workspace is
 * nnc_cbsp_dx_f32's: the partials of a split call, 256-byte aligned, then m floats of row sums (4-byte aligned).  Behind those fields
 * a plan writes GROUP_ROWS, GROUPS (ceil(kdim / group_rows)), ROWS_PER_GROUP (stream: the index rows of a workgroup -- the plan's
 * name for them, not group_rows; else 0), MAX_GROUPS_PER_WORKGROUP (the most groups the index rows of one workgroup, or of one
 * 128-row tile, lie in) and, dx only, TABLES (tiled: 1, 2 or 4; else 0).
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  More than 2^30 bins (G * k), k > 256, a
 * group_rows that is no positive multiple of 32, NULL pointers, a misaligned workspace or packed buffer and a packed buffer smaller
 * than nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz) are NNC_EINVAL, a short workspace NNC_ENOSPACE, all before any HIP call.  No host
 * read, no float atomics; the same call gives the same bits.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBSPDX_GROUPED_P_GROUP_ROWS 11
#define NNC_CBSPDX_GROUPED_P_GROUPS 12
#define NNC_CBSPDX_GROUPED_P_ROWS_PER_GROUP 13
#define NNC_CBSPDX_GROUPED_P_MAX_GROUPS_PER_WORKGROUP 14
#define NNC_CBSPDX_GROUPED_P_TABLES 15
#define NNC_CBSPDX_GROUPED_PLAN_LEN 16
#define NNC_CBSPDC_GROUPED_P_GROUP_ROWS 11
#define NNC_CBSPDC_GROUPED_P_GROUPS 12
#define NNC_CBSPDC_GROUPED_P_ROWS_PER_GROUP 13
#define NNC_CBSPDC_GROUPED_P_MAX_GROUPS_PER_WORKGROUP 14
#define NNC_CBSPDC_GROUPED_PLAN_LEN 15
int64_t nnc_cbsp_grouped_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols);
int nnc_cbsp_grouped_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbsp_grouped_dx_f32(const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                            const void *zero_symbols_dev, int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, float *dx,
                            void *workspace, int64_t workspace_bytes, void *stream);
int64_t nnc_cbsp_grouped_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows);
int nnc_cbsp_grouped_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbsp_grouped_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                            const void *zero_symbols_dev, int64_t nnz, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace,
                            int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBSPGRAD_GROUPED_H */
