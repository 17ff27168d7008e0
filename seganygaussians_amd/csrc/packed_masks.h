// packed_masks.h -- the bit-packed SAM masks that the contrastive loss, the mask scales, the mask sets, the CLIP tiles and the vote
// graph share: M x H x ceil(W / 64) 64-bit words, bit x & 63 of word x >> 6 = pixel x of the row, padding bits 0 (cl_pack_kernel
// of contrastive_loss.h writes them).  The layout, the bilinear taps with which masks are resampled, and the host files' checks.
#pragma once

#include "../../include/mi_contrastive.h"   // MI_CONTRASTIVE_LOSS_MAX_MASKS
#include "host.h"

namespace mirast {

// ---- layout: words per row, words of M masks, tiles of `rows` rows x one word that cover an image ----------------------------------
__host__ __device__ constexpr int pm_row_words(int W) { return (W + 63) / 64; }
__host__ __device__ constexpr size_t pm_words(int M, int H, int W) { return (size_t)M * H * pm_row_words(W); }
__host__ __device__ constexpr size_t pm_tiles(int H, int W, int rows) { return (size_t)((H + rows - 1) / rows) * pm_row_words(W); }

// the valid-pixel bits of word q of a W-pixel row
__device__ inline uint64_t pm_valid_bits(int W, int q)
{
    const int n = W - 64 * q;
    return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

template <typename Int>   // bit x of a row
__device__ inline uint64_t pm_bit(const uint64_t* __restrict__ row, Int x) { return (row[x >> 6] >> (x & 63)) & 1ull; }

// ---- the two taps of upsample_bilinear2d (align_corners=False), f32, as PyTorch's CPU build computes them (UpSampleKernel.cpp) ----
// That build rounds scale * (dst + 0.5) - 0.5 and the height pass t0 w0 + t1 w1 once each (contracted); the fmaf calls reproduce
// that, so the resampled values are its values bit for bit (a separate rounding is 1 ulp of src -- up to 3e-5 of a weight at
// 1080p -- away on ~1 % of pixels).
__device__ inline void pm_source_taps(float scale, int dst, int in_size, int& i0, int& i1, float& l0, float& l1)
{
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);   // area_pixel_compute_source_index
    src = src < 0.f ? 0.f : src;
    const int idx = min((int)floorf(src), in_size - 1);  // guard_index_and_lambda
    const float lam = fminf(fmaxf(src - (float)idx, 0.f), 1.f);
    i0 = idx;
    i1 = idx + (idx < in_size - 1 ? 1 : 0);
    l1 = lam;
    l0 = 1.f - lam;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
constexpr int PM_MAX_MASKS = MI_CONTRASTIVE_LOSS_MAX_MASKS;   // the mask-count limit of every call that takes packed masks
constexpr bool pm_pixels_ok(int H, int W) { return (size_t)H * (size_t)W < ((size_t)1 << 24); }   // every pixel count is exact in f32

inline int pm_check_dims(const char* who, int M, int H, int W, const char* dims = "H, W")
{
    static_assert(PM_MAX_MASKS == 1024, "the text says 1024");
    if (M < 1 || M > PM_MAX_MASKS || H < 1 || W < 1)
        return fail(MI_RAST_ERR_INVALID, std::string(who) + ": need 1 <= M <= 1024 masks and " + dims + " >= 1");
    return MI_RAST_OK;
}

template <typename T>   // do the n_in words read and the n_out words written share memory?
inline bool pm_overlap(const T* in, size_t n_in, const T* out, size_t n_out) { return out < in + n_in && in < out + n_out; }

}  // namespace mirast
