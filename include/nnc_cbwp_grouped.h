/*
 * nnc_cbwp_grouped.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that runs the group-wise
 * codebook layer from 5- and 6-bit split-plane ("wide packed") indices (csrc/nnc_cbwp_grouped.hip).
 * Inference only.  The form, its pack and unpack and the NNC_CBWP_P_* plan fields are nnc_cbwp.h's, which this file includes; the
 * conventions, the error codes, NNC_DT_* and NNC_CBMM_* are nnc.h's.
 */
#ifndef NNC_CBWP_GROUPED_H
#define NNC_CBWP_GROUPED_H

#include "nnc_cbwp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * y = x @ W + bias, then ReLU (NaN kept), W[i, o] = centers_dev[i / group_rows][label (i, o)]: one codebook per block of group_rows
 * input rows (a positive multiple of 32), the labels in the split-plane form of the whole row-major (kdim, ncols) index matrix as the
 * pack of nnc_cbwp.h writes it: a grouped layer has no form of its own.
 * bits, k      bits is 5 (17 <= k <= 32) or 6 (17 <= k <= 64), k the common size of the codebooks.  k <= 16 is NNC_EINVAL: the 2- and
 *              4-bit packed form serves it (the grouped packed call of nnc.h).  bits = 9 and k > 64 are NNC_EINVAL: the group-wise
 *              byte form holds uint8 labels, and 9 bits would be larger than it.
 * centers_dev  float32[G][k], G = ceil(kdim / group_rows) (one row where kdim = 0).  A label >= k reads 0 through the table's zero
 *              entries, with no compare.  With one group the result equals the ungrouped call of nnc_cbwp.h bit for bit.
 * x            x_dtype = NNC_DT_F32, NNC_DT_BF16 or NNC_DT_F16, (m, kdim) contiguous, aligned to its element size.  With half x every
 *              centre is rounded to x's type in the table, the products are exact in float32 and every sum is float32 in an order
 *              fixed by the shape and the CU count; y_dtype is NNC_DT_F32, or x_dtype: the float32 value rounded once.
 *     m <= 16 (PATH = NNC_CBMM_STREAM): k_cbwp_stream_grouped.  m > 16, float32 x (NNC_CBMM_TILED): k_cbwp_tiled_grouped.  Both follow
 *     the ungrouped plan of nnc_cbwp.h for the shape in PATH, VB, MT, COLS, the tiles, SPLITS, RPS and the workspace.
 *     m > 16, bf16 / fp16 x (NNC_CBMM_MFMA): k_cbwp_mfma_grouped on the grid of the group-wise byte form, RPS a multiple of 32; y equals
 *     that form's result on the unpacked labels bit for bit.
 *     Split-K partials are float32 in the workspace and are summed in split order: no float atomics, no host read.  m = 0 or
 *     ncols = 0: nothing is launched; kdim = 0: y = bias.
 * nnc_cbwp_grouped_workspace_bytes  the workspace the call needs (planned for 256 compute units; the splits never shrink with more).
 * nnc_cbwp_grouped_plan  host: NNC_CBWP_GROUPED_PLAN_LEN values: the NNC_CBWP_P_* fields (DTYPE the last of them; LDS and COPIES those
 *              of the grouped kernels), then GROUP_ROWS, GROUPS (G; 0 where kdim = 0), MAX_GROUPS_PER_SPLIT and TABLES, the tables
 *              held in LDS: 4 (one per wave, stream), 2 (tiled), 1 (MFMA).  A plan without a kernel instantiation is NNC_EINVAL.
 * Argument errors come back before any HIP call: NNC_EINVAL, or NNC_ENOSPACE for a short workspace.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBWP_GROUPED_P_GROUP_ROWS 15
#define NNC_CBWP_GROUPED_P_GROUPS 16
#define NNC_CBWP_GROUPED_P_MAX_GROUPS_PER_SPLIT 17
#define NNC_CBWP_GROUPED_P_TABLES 18
#define NNC_CBWP_GROUPED_PLAN_LEN 19
int64_t nnc_cbwp_grouped_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbwp_grouped_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbwp_grouped(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                     const float *centers_dev, int32_t k, int64_t group_rows, const float *bias_dev, int32_t relu, void *y, int y_dtype,
                     void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBWP_GROUPED_H */
