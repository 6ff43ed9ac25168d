/*
 * nnc_cbwpgrad.h -- the part of the C ABI of libnnc_hip.so that trains the quantized layer of 17 .. 512 centres from its 5-, 6- and
 * 9-bit split-plane ("wide packed") indices (csrc/nnc_cbwpgrad.hip): the backward pass of nnc_cbwp.  The form,
 * the conventions, the error codes, NNC_DT_* and NNC_CBMM_* are nnc_cbwp.h's and nnc.h's, which this file includes.
 */
#ifndef NNC_CBWPGRAD_H
#define NNC_CBWPGRAD_H

#include "nnc_cbwp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * packed, packed_bytes, bits, ncols: the buffer nnc_cbwp_pack wrote, as nnc_cbwp takes it; it is never unpacked and dW is never
 * written.  x_dtype is NNC_DT_F32, NNC_DT_BF16 or NNC_DT_F16, the type of g (and x).  W[i, o] = centers_dev[label (i, o)]; a label
 * >= k reads 0 in dx and falls into no bin in dc; the fields and plane bits past ncols form no product and are never binned (a
 * column at or past ncols is 0 in an image, not table[0]).  With bf16 / fp16 g every centre is rounded to that type, the products
 * are exact in float32 and every sum is float32; centers_dev stays float32 and dc is the gradient with respect to it.
 * nnc_cbwp_dx   dx = g @ W^T, g (m, ncols) of x_dtype, dx (m, kdim) of dx_dtype: NNC_DT_F32, or x_dtype (the float32 value rounded once).
 *     m <= 16 (PATH = NNC_CBMM_STREAM): k_cbwpdx_stream.  A lane owns COLS = 8 * VB / BASE consecutive columns and keeps COLS * MT
 *         <= 64 values of g; the table has ENTRIES = 2^bits entries in COPIES per-bank copies; one split per column block (CPS = 64
 *         * COLS), summed in block order.
 *     m > 16, float32 (NNC_CBMM_TILED): k_cbwpdx_tiled, the 128 x 128 tile over W^T; ncols is cut into min(ceil(512 / tiles),
 *         floor(ncols / 128), 16) splits of a multiple of 32 columns.
 *     m > 16, bf16 / fp16 (NNC_CBMM_MFMA): k_cbwpdx_mfma, nnc_cbmm_dx_h16's tile, tiles and splits (CPS a multiple of 32); dx equals
 *         nnc_cbmm_dx_h16 on the unpacked labels bit for bit.
 * nnc_cbwp_dc   dc[j] = sum over the (i, o) with label j of (x^T g)[i, o], float64[k] (out_f64 != 0) or float32[k]: the byte form's
 *         call (nnc_cbmm_dc_f32 for float32, nnc_cbmm_dc_h16 for half) on the unpacked labels bit for bit at every m and dtype.
 *         SPLITS, RPS and TERMS_LOG2 are those of nnc_cbmm_dc_plan / nnc_cbmm_dc_h16_plan for the shape at label_bytes = 1 (bits 5,
 *         6) or 2 (bits 9), every dW is formed as that call forms it and binned as rint(dW * 2^S) with the same S; the int64 sums
 *         are exact and order-independent.  k_cbwpdc_stream (m <= 16), k_cbwpdc_tiled (float32), k_cbwpdc_mfma (half); COPIES = 32,
 *         8 or 2 copies of every LDS bin (k <= 64, <= 256, above), a lane adding into copy lane mod COPIES.  A non-finite x or g,
 *         or 2^P > 2^127: all NaN; a zero maximum: dc = 0.
 * m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0.  No float atomics: split partials are float32 in
 * the workspace and are summed in split order.  No host read; the same call gives the same bits.  No load leaves the packed buffer.
 * Argument errors come back before any HIP call: NNC_EINVAL for the errors of nnc_cbwp (dtype, sizes, bits, k, the buffer), an odd
 * address of a half operand, a dx_dtype that is neither NNC_DT_F32 nor x_dtype, a NULL operand, a plan without a kernel
 * instantiation; NNC_ENOSPACE for a short workspace (the dc workspace is 8-byte aligned, the dx one 4-byte).
 * The plans are host arithmetic; the splits depend on the shape alone (planned for 256 compute units), `cus` changes only the grid
 * of the stream path.  VB, MT and COLS are 0 off the stream path.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBWPDX_P_PATH 0
#define NNC_CBWPDX_P_VB 1
#define NNC_CBWPDX_P_MT 2
#define NNC_CBWPDX_P_COLS 3
#define NNC_CBWPDX_P_BASE 4
#define NNC_CBWPDX_P_PLANES 5
#define NNC_CBWPDX_P_COPIES 6      /* per-bank copies of the table (1 on the float32 tile) */
#define NNC_CBWPDX_P_ENTRIES 7
#define NNC_CBWPDX_P_SPLITS 8      /* splits of ncols */
#define NNC_CBWPDX_P_CPS 9         /* columns per split */
#define NNC_CBWPDX_P_LDS 10
#define NNC_CBWPDX_P_COL_TILES 11
#define NNC_CBWPDX_P_ROW_TILES 12
#define NNC_CBWPDX_P_WORKSPACE 13
#define NNC_CBWPDX_P_DTYPE 14
#define NNC_CBWPDX_PLAN_LEN 15
#define NNC_CBWPDC_P_PATH 0
#define NNC_CBWPDC_P_VB 1
#define NNC_CBWPDC_P_MT 2
#define NNC_CBWPDC_P_COLS 3
#define NNC_CBWPDC_P_BASE 4
#define NNC_CBWPDC_P_PLANES 5
#define NNC_CBWPDC_P_COPIES 6      /* copies of every LDS bin */
#define NNC_CBWPDC_P_SPLITS 7      /* splits of m */
#define NNC_CBWPDC_P_RPS 8         /* rows of m per split */
#define NNC_CBWPDC_P_LDS 9
#define NNC_CBWPDC_P_COL_TILES 10
#define NNC_CBWPDC_P_ROW_TILES 11
#define NNC_CBWPDC_P_TERMS_LOG2 12
#define NNC_CBWPDC_P_WORKSPACE 13
#define NNC_CBWPDC_P_DTYPE 14
#define NNC_CBWPDC_PLAN_LEN 15
int64_t nnc_cbwp_dx_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbwp_dx_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out);
int nnc_cbwp_dx(const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
                const float *centers_dev, int32_t k, void *dx, int dx_dtype, void *workspace, int64_t workspace_bytes, void *stream);
int64_t nnc_cbwp_dc_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k);
int nnc_cbwp_dc_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out);
int nnc_cbwp_dc(const void *x, const void *g, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits,
                int64_t ncols, int32_t k, void *dc, int32_t out_f64, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBWPGRAD_H */
