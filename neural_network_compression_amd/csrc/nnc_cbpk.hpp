// nnc_cbpk.hpp -- what the 2- and 4-bit packed codebook matmul (nnc_cbpk.hip) shares with its backward pass (nnc_cbpkgrad.hip):
// the layout arithmetic and the limits of the packed form, the argument checks, the constants of the per-bank lookup table and
// the aligned row load of the stream kernels.
#pragma once
#include "nnc_cbmm.hpp"

#define PK_COPIES 32              // per-bank copies of the table
#define PK_CSHIFT 5
#define PK_ACC 64                 // accumulators per lane: columns per lane per row x rows of x

// ------------------------------------------------------------------ the layout (host)
static inline bool pk_bits_ok(int bits) { return bits == 2 || bits == 4; }
static inline long long pk_row_bytes(long long ncols, int bits) { return 16 * cdiv(ncols * bits, 128); }
static inline bool pk_size_ok(int64_t kdim, int64_t ncols) { return kdim <= (1LL << 40) && ncols <= (1LL << 40) && (ncols == 0 || kdim <= (1LL << 44) / cdiv(ncols, 2)); }

// ------------------------------------------------------------------ argument checks (host)
static int pk_check_form(const char *fn, int64_t kdim, int64_t ncols, int bits)
{
    if (kdim < 0 || ncols < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    if (!pk_bits_ok(bits)) return fail(NNC_EINVAL, std::string(fn) + ": bits must be 2 or 4");
    if (!pk_size_ok(kdim, ncols)) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

static int pk_check_buffer(const char *fn, const void *packed, int64_t packed_bytes, int64_t kdim, int64_t ncols, int bits)
{
    if (packed_bytes != kdim * pk_row_bytes(ncols, bits)) return fail(NNC_EINVAL, std::string(fn) + ": packed_bytes is not nnc_cbpk_pack_bytes(kdim, ncols, bits)");
    if (packed_bytes > 0 && !packed) return fail(NNC_EINVAL, std::string(fn) + ": packed is NULL");
    if (reinterpret_cast<uintptr_t>(packed) % 16) return fail(NNC_EINVAL, std::string(fn) + ": packed must be 16-byte aligned");
    return NNC_OK;
}

static int pk_check(const char *fn, int64_t m, int64_t kdim, int64_t ncols, int bits, int32_t k)
{
    if (m < 0) return fail(NNC_EINVAL, std::string(fn) + ": negative size");
    const int rc = pk_check_form(fn, kdim, ncols, bits);
    if (rc != NNC_OK) return rc;
    if (k < 1 || k > (1 << bits)) return fail(NNC_EINVAL, std::string(fn) + ": k outside 1..2^bits");
    if (m > (1LL << 40)) return fail(NNC_EINVAL, std::string(fn) + ": size too large");
    return NNC_OK;
}

// ------------------------------------------------------------------ a lane's VB bytes of a packed row (aligned: VB divides 16)
template <int VB>
__device__ __forceinline__ void pk_load(const unsigned char *p, uint32_t *w)
{
    if constexpr (VB == 1) w[0] = *p;
    else if constexpr (VB == 2) w[0] = *reinterpret_cast<const uint16_t *>(p);
    else load_chunk<VB>(p, w);
}
