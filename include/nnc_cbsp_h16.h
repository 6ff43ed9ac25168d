/*
 * nnc_cbsp_h16.h -- the part of the C ABI of libnnc_hip.so (include/nnc.h, which includes this file) that runs the bitmap-sparse
 * codebook layer on bf16 / fp16 activations.  The conventions, the error codes, NNC_DT_*, NNC_CBMM_*, NNC_CBSP_ROWSUM_* and the
 * NNC_CBSP_P_* plan fields are nnc.h's; include nnc.h, not this file.
 */
#ifndef NNC_CBSP_H16_H
#define NNC_CBSP_H16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * nnc_cbsp_f32's layer on bf16 or fp16 activations (csrc/nnc_cbsp_h16.hip), forward and inference only:
 *     y = x @ W_h + bias (then ReLU),   W_h[i, o] = rn_dtype(centers_dev[label[i, o]]),   dtype = x_dtype (NNC_DT_BF16 / NNC_DT_F16)
 * packed, packed_bytes, label_bytes, zero_symbol, nnz: the form nnc_cbsp_pack wrote, as nnc_cbsp_f32 takes it.  label[i, o] is the
 * stored symbol, zero_symbol at a skipped position.  An index >= k reads 0.  centers_dev float32[k] and bias_dev float32[ncols] (or
 * NULL) stay float32 in memory: every centre is rounded to dtype (to nearest even) when a kernel builds its LDS table, so an fp16
 * centre beyond 65504 acts as Inf; the bias is added in float32.  A product of two bf16 or two fp16 values is exact in float32; every
 * sum is float32, in an order fixed by the shape and the CU count alone: no float atomics, the same call gives the same bits.  ReLU
 * keeps NaN.  y_dtype is NNC_DT_F32, or x_dtype: the float32 value rounded once to nearest even.  x is contiguous (m, kdim) on any
 * 2-byte aligned address.  m or ncols = 0 is a no-op; kdim = 0 writes y = bias (or 0).
 * m <= 16 (PATH = NNC_CBMM_STREAM): k_cbsp_stream with x read as dtype and widened and the d table built from the rounded centres,
 *     d[s] = rn(c[s]) - rn(c_z).  The plan is nnc_cbsp_plan's field for field and the fmaf chain is nnc_cbsp_f32's, so the float32
 *     result equals nnc_cbsp_f32 on x widened and the centres rounded to dtype and widened, bit for bit; a skipped weight stays absent
 *     when rn(c_z) == 0.
 * m > 16 (PATH = NNC_CBMM_MFMA): k_cbsp_mfma, the 128 x 128 tile of nnc_cbmm_h16 on v_mfma_f32_32x32x16_{bf16,f16} with the W tile
 *     decoded from the bitmap and the symbols.  The plan is nnc_cbmm_h16_plan's in every shared field (tiles, splits, RPS a multiple
 *     of 32, LDS, workspace; k_cbmm_reduce combines the splits), and y equals nnc_cbmm_h16 on the unpacked labels (nnc_cbsp_unpack)
 *     bit for bit, for every input.  The departure from nnc_cbsp_f32: a skipped weight is an entry of W_h here (rn(c_z), or 0 for
 *     zero_symbol >= k), not absent, because a per-element mask cannot be applied inside an MFMA; an Inf or NaN in x at a skipped
 *     position therefore gives NaN (Inf * 0) as in the byte form, also when c_z == 0.
 * nnc_cbsp_h16_workspace_bytes: what the call needs (host arithmetic, plans for 256 CUs; the workspace is 4-byte aligned).
 * nnc_cbsp_h16_plan: host, NNC_CBSP_H16_PLAN_LEN values: the NNC_CBSP_P_* fields (MT is 0 and ROWSUM is NNC_CBSP_ROWSUM_NONE on the
 * MFMA path: it forms no row sums), then NNC_CBSP_H16_P_DTYPE.
 * Argument errors come back before any HIP call: NNC_EINVAL for an x_dtype that is not NNC_DT_BF16 / NNC_DT_F16, a y_dtype that is
 * neither NNC_DT_F32 nor x_dtype, an odd x or half y address, the errors of nnc_cbsp_f32, a plan without a kernel instantiation;
 * NNC_ENOSPACE for a short workspace.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBSP_H16_P_DTYPE 11
#define NNC_CBSP_H16_PLAN_LEN 12
int64_t nnc_cbsp_h16_workspace_bytes(int64_t m, int64_t kdim, int64_t ncols, int label_bytes);
int nnc_cbsp_h16_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int label_bytes, int32_t k, int32_t cus, int64_t *out);
int nnc_cbsp_h16(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int label_bytes, int64_t ncols,
                 int32_t zero_symbol, int64_t nnz, const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, void *y, int y_dtype,
                 void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBSP_H16_H */
