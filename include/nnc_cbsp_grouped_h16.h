/*
 * nnc_cbsp_grouped_h16.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that runs the pruned
 * group-wise codebook layer from the bitmap-sparse form of its indices on bf16 / fp16 activations.  The conventions, the error
 * codes, NNC_DT_*, NNC_CBMM_*, NNC_CBSP_ROWSUM_*, the NNC_CBSP_P_* and the NNC_CBSP_GROUPED_P_* plan fields are nnc.h's; include
 * nnc.h, not this file.
 */
#ifndef NNC_CBSP_GROUPED_H16_H
#define NNC_CBSP_GROUPED_H16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * nnc_cbsp_grouped_f32's layer on bf16 or fp16 activations (csrc/nnc_cbsp_grouped_h16.hip), forward and
 * inference only:
 *     y = x @ W_h + bias (then ReLU),   W_h[i, o] = rn_dtype(centers_dev[i / group_rows][label[i, o]]),   dtype = x_dtype
 * x_dtype is NNC_DT_BF16 or NNC_DT_F16.  packed, packed_bytes, zero_symbols_dev, nnz, k, group_rows: the form nnc_cbsp_grouped_pack
 * wrote, as nnc_cbsp_grouped_f32 takes it.  label[i, o] is the stored symbol, zero_symbols[i / group_rows] at a skipped position.  An
 * index >= k reads 0.  centers_dev float32[G][k] and bias_dev float32[ncols] (or NULL) stay float32 in memory: every centre is
 * rounded to dtype (to nearest even) when a kernel builds its LDS table, so an fp16 centre of 1e5 acts as Inf; the bias is added
 * in float32.  A product of two bf16 or two fp16 values is exact in float32; every sum is float32, in an order fixed by the shape and
 * the CU count alone: no float atomics, the same call gives the same bits.  ReLU keeps NaN.  y_dtype is NNC_DT_F32, or x_dtype: the
 * float32 value rounded once to nearest even.  x is contiguous (m, kdim) on any 2-byte aligned address.  m or ncols = 0 is a no-op;
 * kdim = 0 writes y = bias (or 0).
 * m <= 16 (PATH = NNC_CBMM_STREAM): nnc_cbsp_grouped_f32's kernels with x read as dtype and widened: c_{z_g} is rn(c) widened, the d
 *     table is d_g[s] = rn(c_g[s]) - rn(c_{z_g}), rs_g sums the widened x in k_cbspg_rowterm's order, t = sum_g rn(c_{z_g}) * rs_g.
 *     The plan is nnc_cbsp_grouped_plan's field for field and the arithmetic is nnc_cbsp_grouped_f32's, so the float32 result equals
 *     nnc_cbsp_grouped_f32 on x widened and the centres rounded to dtype and widened, bit for bit; a skipped weight stays absent when
 *     rn(c_{z_g}) == 0 (a centre that underflows to 0 in fp16 included).
 * m > 16 (PATH = NNC_CBMM_MFMA): k_cbspg_mfma, the 128 x 128 tile of nnc_cbmm_grouped on v_mfma_f32_32x32x16_{bf16,f16} with the W
 *     tile decoded from the bitmap and the symbols.  The plan is nnc_cbmm_grouped_plan's for x_dtype in every shared field (tiles,
 *     splits, RPS a multiple of 32, LDS, workspace; k_cbmm_reduce combines the splits), and y equals nnc_cbmm_grouped on the unpacked
 *     labels (nnc_cbsp_grouped_unpack) with the same dtypes, bit for bit, for every input.  The departure from nnc_cbsp_grouped_f32
 *     and from the m <= 16 path: a skipped weight is an entry of W_h here (rn(c_{z_g}), or 0 for z_g >= k), not absent, because a
 *     per-element mask cannot be applied inside an MFMA; there is no rank-1 term and no row-sum pass, and an Inf or NaN in x at a
 *     skipped position gives NaN (Inf * 0) as in the byte form, also when c_{z_g} == 0.
 * nnc_cbsp_grouped_h16_workspace_bytes: what the call needs (host arithmetic, plans for 256 CUs; the workspace is 4-byte aligned);
 *     0 for an x_dtype that is neither.
 * nnc_cbsp_grouped_h16_plan: host, NNC_CBSP_GROUPED_H16_PLAN_LEN values: the NNC_CBSP_P_* fields (ROWSUM is NNC_CBSP_ROWSUM_PASS on the
 *     stream path; MT is 0 and ROWSUM is NNC_CBSP_ROWSUM_NONE on the MFMA path), the NNC_CBSP_GROUPED_P_* fields, then
 *     NNC_CBSP_GROUPED_H16_P_DTYPE.
 * Argument errors come back before any HIP call: NNC_EINVAL for an x_dtype that is not NNC_DT_BF16 / NNC_DT_F16, a y_dtype that is
 * neither NNC_DT_F32 nor x_dtype, an odd x or half y address, the errors of nnc_cbsp_grouped_f32, a plan without a kernel
 * instantiation; NNC_ENOSPACE for a short workspace.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBSP_GROUPED_H16_P_DTYPE 14
#define NNC_CBSP_GROUPED_H16_PLAN_LEN 15
int64_t nnc_cbsp_grouped_h16_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols);
int nnc_cbsp_grouped_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int32_t k, int64_t group_rows, int32_t cus, int64_t *out);
int nnc_cbsp_grouped_h16(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int64_t ncols,
                         const void *zero_symbols_dev, int64_t nnz, const float *centers_dev, int32_t k, int64_t group_rows, const float *bias_dev,
                         int32_t relu, void *y, int y_dtype, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBSP_GROUPED_H16_H */
