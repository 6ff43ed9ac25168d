/*
 * nnc_cbpkgrad_grouped.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that is the backward
 * pass of the group-wise codebook layer on 2- and 4-bit packed indices.  The conventions, the error codes and the NNC_CBPKDX_P_* /
 * NNC_CBPKDC_P_* plan fields are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBPKGRAD_GROUPED_H
#define NNC_CBPKGRAD_GROUPED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The backward pass of nnc_cbpk_grouped (float32 x) from the same codebooks and the same packed buffer of the whole index matrix
 * (csrc/nnc_cbpkgrad_grouped.hip).  W[i, o] = centers_dev[i / group_rows][label (i, o)]; the index side is
 * nnc_cbpk_grouped's contract (centers_dev float32[G][k] contiguous, 1 <= k <= 2^bits, bits 2 or 4, group_rows a positive multiple
 * of 32, a short last group, group_rows >= kdim one group, packed_bytes == nnc_cbpk_pack_bytes(kdim, ncols, bits), packed 16-byte
 * aligned), the gradient side nnc_cbpk_dx_f32's / nnc_cbpk_dc_f32's (float32 throughout, no float atomics, no host read, the same
 * call gives the same bits, the result a function of the shape and the data only).  G = max(1, ceil(kdim / group_rows)).
 * nnc_cbpk_grouped_dx_f32   dx[r, i] = sum_o g[r, o] * centers_dev[i / group_rows][label (i, o)]; a label >= k reads 0; a column
 *                           past ncols forms no product and g is never loaded there (the padding fields hold label 0 and do not
 *                           contribute, whatever centers[q][0] is).  Row i of dx is, bit for bit, row i of nnc_cbpk_dx_f32 on the
 *                           same packed buffer with the one table of i's group.
 * nnc_cbpk_grouped_dc_f32   dc[q][k] = sum over (i, o) with i / group_rows = q and label (i, o) = k of dW[i, o], float64[G][k]
 *                           (out_f64 != 0) or float32[G][k].  dW is formed, scaled and binned as nnc_cbmm_dc_f32 does, with that
 *                           call's S (T the whole layer's at label_bytes 1): the result equals nnc_cbmm_grouped_dc_f32 on the
 *                           unpacked labels, bit for bit.  All NaN if x or g holds Inf / NaN or P > 127; dc = 0 on a zero maximum;
 *                           a label >= k and a padding field fall into no bin.
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  Argument errors (those of nnc_cbpk_dx_f32 /
 * nnc_cbpk_dc_f32, m * kdim <= 2^44 among them, those nnc_cbpk_grouped makes of group_rows, G * k > 2^30, NULL pointers, a misaligned
 * workspace) come back as NNC_EINVAL (NNC_ENOSPACE for a short workspace) before any HIP call.
 * The plans are nnc_cbpk_dx_plan / nnc_cbpk_dc_plan of (m, kdim, ncols, bits, k, cus): PATH, VB, MT, COLS, ENTRIES, SPLITS, CPS /
 * RPS, COL_TILES, ROW_TILES, TERMS_LOG2 and the dx WORKSPACE are theirs.  Their own: the dc WORKSPACE (64 + 8 * G * k bytes, 8-byte
 * aligned); LDS of dx (stream: one table of ENTRIES x COPIES floats per wave and no staging row; tiled: the tables of the up to four
 * groups a 128-row tile lies in); on the tiled path COPIES of dc (the copies of a bin in one of the per-group sets the LDS bins are
 * cut into; LDS is unchanged).  Behind the NNC_CBPKDX_P_* / NNC_CBPKDC_P_* fields a plan writes GROUP_ROWS, GROUPS
 * (ceil(kdim / group_rows)), ROWS_PER_GROUP (stream: the packed rows of a workgroup; else 0), MAX_GROUPS_PER_WORKGROUP (the most
 * groups the rows of one workgroup lie in) and HELD (dx: the tables held in LDS, four on the stream path, one per wave; dc: the
 * per-group sets of bins): NNC_CBPKGRAD_GROUPED_PLAN_LEN values.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBPKGRAD_GROUPED_P_GROUP_ROWS 12
#define NNC_CBPKGRAD_GROUPED_P_GROUPS 13
#define NNC_CBPKGRAD_GROUPED_P_ROWS_PER_GROUP 14
#define NNC_CBPKGRAD_GROUPED_P_MAX_GROUPS_PER_WORKGROUP 15
#define NNC_CBPKGRAD_GROUPED_P_HELD 16
#define NNC_CBPKGRAD_GROUPED_PLAN_LEN 17
int64_t nnc_cbpk_grouped_dx_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbpk_grouped_dx_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbpk_grouped_dx_f32(const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                            const float *centers_dev, int32_t k, int64_t group_rows, float *dx, void *workspace, int64_t workspace_bytes,
                            void *stream);
int64_t nnc_cbpk_grouped_dc_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows);
int nnc_cbpk_grouped_dc_plan(int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbpk_grouped_dc_f32(const float *x, const float *g, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                            int64_t ncols, int32_t k, int64_t group_rows, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBPKGRAD_GROUPED_H */
