/*
 * nnc_cbsp_grouped.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the pruned
 * group-wise codebook layer run from the bitmap-sparse form of its indices.  The conventions, the error codes and the NNC_CBSP_P_*
 * plan fields are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBSP_GROUPED_H
#define NNC_CBSP_GROUPED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * One codebook per block of group_rows input rows (nnc_cbmm_grouped) on the bitmap-sparse form (nnc_cbsp_*), float32 x
 * (csrc/nnc_cbsp_grouped.hip).  G = ceil(kdim / group_rows); group_rows a positive multiple of 32 (a short
 * last group; group_rows >= kdim is one group); 1 <= k <= 256, uint8 labels only; centers_dev float32[G][k] contiguous;
 * zero_symbols_dev uint8[G] on the device, z_g the skipped symbol of group g.  Any byte is valid: z_g >= k means c_{z_g} = 0.
 *
 * The form is nnc_cbsp_pack's buffer at label_bytes 1 (the same offsets, the 256-byte alignment, the int64 counts, the pos < nnz
 * guards; nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz) stays the size query) with one difference, the bit rule: bit (i, o) is set iff
 * labels[i, o] != zero_symbols[i / group_rows].
 * nnc_cbsp_grouped_pack    as nnc_cbsp_pack: a buffer of nnc_cbsp_pack_bytes(kdim, ncols, 1, 0) takes the structure and *nnz_dev (a
 *                          device int64, may be NULL) the count of stored symbols; a buffer of the full size takes the symbols too.
 * nnc_cbsp_grouped_unpack  the inverse: labels_out[i, o] = the stored symbol, or zero_symbols[i / group_rows].
 *
 * The product:
 *     y[r, o] = t[r] + sum over stored (i, o) of x[r, i] * d_g(i)[label] (+ bias[o], then ReLU; NaN stays NaN)
 *     d_g[s] = float32(c_g[s] - c_{z_g}) for s < k, -c_{z_g} for s >= k;   t[r] = sum_g c_{z_g} * rs_g[r]
 * rs_g[r] is the sum of x[r, .] over the rows of group g, formed as nnc_cbsp_f32's row-sum pass forms a whole row (thread-strided by
 * 256 from the group's first row, then the fixed halving tree); t starts from the first group with c_{z_g} != 0 and adds the others
 * in group order.  A group with c_{z_g} == 0 exactly adds nothing to t and its skipped weights are absent (an Inf in x there meets
 * no 0); if no group has c_{z_g} != 0, t is not added at all.  The test is c != 0, so a NaN centre counts.  t comes from a pass of
 * its own (k_cbspg_rowterm) at every m.  No float atomics; the partials of a split call are summed in nnc_cbsp_f32's order; the
 * same call gives the same bits.  m = 0 or ncols = 0: nothing is written; kdim = 0: y = bias.
 *
 * Against nnc_cbsp_f32 with one group (group_rows >= kdim, zero_symbol = z_0): for m > 16 the result is the same bit for bit for any
 * c_z (both take the row sum from the same pass; c_z * rs, then + acc, are the same two roundings).  For m <= 16 it is the same bit
 * for bit when c_z == 0 exactly; with c_z != 0 nnc_cbsp_f32 sums the row inside its stream kernel in another order, and the two
 * agree only within the float bound of the product (2 * (kdim + 4) * 2^-24 * (|c_z| * sum|x| + sum |x| * |d|)).
 *
 * The plan is nnc_cbsp_plan(m, kdim, ncols, 1, k, cus): PATH, MT, COPIES, ENTRIES, SPLITS, RPS, LDS, COL_TILES and ROW_TILES are its
 * values.  ROWSUM is always NNC_CBSP_ROWSUM_PASS.  WORKSPACE: the partials of a split call (256-byte aligned), then t (m floats), then
 * one 32-bit word that says whether t applies.  Behind the NNC_CBSP_P_* fields the plan writes GROUP_ROWS, GROUPS and
 * MAX_GROUPS_PER_SPLIT (the most groups the rows of one split lie in): NNC_CBSP_GROUPED_PLAN_LEN values.
 * Argument errors (NNC_EINVAL; NNC_ENOSPACE for a short pack buffer or workspace) are returned before any HIP call.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBSP_GROUPED_P_GROUP_ROWS 11
#define NNC_CBSP_GROUPED_P_GROUPS 12
#define NNC_CBSP_GROUPED_P_MAX_GROUPS_PER_SPLIT 13
#define NNC_CBSP_GROUPED_PLAN_LEN 14
int nnc_cbsp_grouped_pack(const void *labels, int64_t kdim, int64_t ncols, int64_t group_rows, const void *zero_symbols_dev, void *packed,
                          int64_t packed_bytes, int64_t *nnz_dev, void *stream);
int nnc_cbsp_grouped_unpack(const void *packed, int64_t packed_bytes, int64_t kdim, int64_t ncols, int64_t group_rows, const void *zero_symbols_dev,
                            int64_t nnz, void *labels_out, void *stream);
int64_t nnc_cbsp_grouped_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols);
int nnc_cbsp_grouped_plan(int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbsp_grouped_f32(const float *x, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols, const void *zero_symbols_dev,
                         int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, const float *bias_dev, int32_t relu, float *y,
                         void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBSP_GROUPED_H */
