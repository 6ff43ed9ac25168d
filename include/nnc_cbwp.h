/*
 * nnc_cbwp.h -- the part of the C ABI of libnnc_hip.so that runs the quantized layer of 17 .. 512 centres from 5-, 6- and 9-bit
 * split-plane ("wide packed") indices (csrc/nnc_cbwp.hip).  Inference only.  The conventions, the error codes,
 * NNC_DT_* and NNC_CBMM_* are nnc.h's, which this file includes.
 */
#ifndef NNC_CBWP_H
#define NNC_CBWP_H

#include "nnc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The form of a (kdim, ncols) index matrix at `bits` = 5, 6 or 9: a base field of 4 (bits 5, 6) or 8 (bits 9) bits per label and
 * bits - base one-bit planes.  One buffer of kdim rows; row i holds its base part, 16 * ceil(ncols * base / 128) bytes, label
 * (i, o)'s low `base` bits at bit o * base of the part (low bits first, the row of nnc_cbpk_pack at base = 4, a byte per label at
 * base = 8), then plane 0 and (bits 6) plane 1, 16 * ceil(ncols / 128) bytes each, bit o of plane p = bit base + p of label (i, o).
 * Every part starts on a 16-byte boundary; the fields and bits past ncols are 0.  label = field | plane0 << base | plane1 <<
 * (base + 1).  No label straddles a dword and every load of 1 .. 16 bytes of a part is naturally aligned.
 *
 * nnc_cbwp_pack_bytes  the bytes of the buffer (host arithmetic); 0 for a width other than 5, 6, 9, a negative or too large size.
 * nnc_cbwp_pack        labels (label_bytes 1 or 2 per index, any address that is a multiple of label_bytes, device) -> packed (16-byte
 *                      aligned, packed_bytes = nnc_cbwp_pack_bytes).  One pass, a thread per dword written.  bad_count_dev (or NULL):
 *                      one device uint32 that receives the number of labels >= 2^bits (they are stored masked).
 * nnc_cbwp_unpack      the labels again, 1 or (required at bits = 9) 2 bytes each.
 * nnc_cbwp             y = x @ W + bias, then ReLU (NaN kept), W[i, o] = centers_dev[label (i, o)], a label >= k reading 0.  x is
 *                      float32, bf16 or fp16 (x_dtype, NNC_DT_*), (m, kdim) contiguous; centers_dev float32[k], 1 <= k <= 2^bits;
 *                      bias_dev float32[ncols] or NULL.  With half x every centre is rounded to x's type, the products are exact in
 *                      float32 and every sum is float32; y_dtype is NNC_DT_F32, or x_dtype: the float32 value rounded once.
 *     m <= 16 (PATH = NNC_CBMM_STREAM): k_cbwp_stream; a lane owns COLS = 8 * VB / BASE consecutive columns of a row.
 *     m > 16, float32 x (NNC_CBMM_TILED): k_cbwp_tiled, the 128 x 128 tile; bf16 / fp16 x (NNC_CBMM_MFMA): k_cbwp_mfma.
 *     Split-K partials are float32 in the workspace and are summed in split order: no float atomics, the same call gives the same
 *     bits.  m = 0 or ncols = 0: y is empty; kdim = 0: y = bias.
 * nnc_cbwp_workspace_bytes  the workspace nnc_cbwp needs (planned for 256 compute units; the splits never shrink with more).
 * nnc_cbwp_plan        host: the NNC_CBWP_PLAN_LEN decisions nnc_cbwp takes on a device of `cus` compute units.  A plan without a
 *                      kernel instantiation is NNC_EINVAL.
 * Argument errors come back before any HIP call: NNC_EINVAL, or NNC_ENOSPACE for a short workspace.
 * ---------------------------------------------------------------------------------- */
#define NNC_CBWP_P_PATH 0
#define NNC_CBWP_P_VB 1
#define NNC_CBWP_P_MT 2
#define NNC_CBWP_P_COLS 3
#define NNC_CBWP_P_BASE 4
#define NNC_CBWP_P_PLANES 5
#define NNC_CBWP_P_COPIES 6
#define NNC_CBWP_P_ENTRIES 7
#define NNC_CBWP_P_SPLITS 8
#define NNC_CBWP_P_RPS 9
#define NNC_CBWP_P_LDS 10
#define NNC_CBWP_P_COL_TILES 11
#define NNC_CBWP_P_ROW_TILES 12
#define NNC_CBWP_P_WORKSPACE 13
#define NNC_CBWP_P_DTYPE 14
#define NNC_CBWP_PLAN_LEN 15
int64_t nnc_cbwp_pack_bytes(int64_t kdim, int64_t ncols, int bits);
int nnc_cbwp_pack(const void *labels, int label_bytes, int64_t kdim, int64_t ncols, int bits, void *packed, int64_t packed_bytes,
                  uint32_t *bad_count_dev, void *stream);
int nnc_cbwp_unpack(const void *packed, int64_t packed_bytes, int bits, int64_t kdim, int64_t ncols, void *labels_out, int label_bytes_out,
                    void *stream);
int64_t nnc_cbwp_workspace_bytes(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits);
int nnc_cbwp_plan(int x_dtype, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k, int32_t cus, int64_t *out);
int nnc_cbwp(const void *x, int x_dtype, int64_t m, int64_t kdim, const void *packed, int64_t packed_bytes, int bits, int64_t ncols,
             const float *centers_dev, int32_t k, const float *bias_dev, int32_t relu, void *y, int y_dtype, void *workspace,
             int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNC_CBWP_H */
