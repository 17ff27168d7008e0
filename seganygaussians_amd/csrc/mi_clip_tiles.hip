// mi_clip_tiles.hip -- C-ABI implementation of include/mi_clip_tiles.h.
#include "host.h"
#include "../../include/mi_clip_tiles.h"

#include "clip_tiles.h"   // masked crops resized and normalised for the CLIP network, and the mask index map

using namespace mirast;

namespace {
int ct_check(int M, int H, int W)
{
    if (int rc = pm_check_dims("clip tiles", M, H, W)) return rc;
    return pm_pixels_ok(H, W) ? MI_RAST_OK : fail(MI_RAST_ERR_INVALID, "clip tiles: need H * W < 2^24 pixels");
}

template <bool AA, typename OutT>
void ct_launch(int M, int H, int W, const uint64_t* packed, const uint8_t* image, const int* rects, int layout, float bg,
               const CtNorm& nrm, int Sh, int Sw, void* tiles, hipStream_t stream)
{
    hipLaunchKernelGGL((ct_tiles_kernel<AA, OutT>), dim3((unsigned)((Sh + CT_BAND - 1) / CT_BAND), (unsigned)M), dim3(CT_THREADS), 0,
                       stream, H, W, pm_row_words(W), packed, image, rects, layout, bg, nrm, Sh, Sw, (OutT*)tiles);
}
}  // namespace

extern "C" {

int mi_mask_clip_tiles(int M, int H, int W, const unsigned long long* packed, const unsigned char* image, const int* rects, int layout,
                       float background, int antialias, const float* mean, const float* std, int Sh, int Sw, int half, void* tiles,
                       void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ct_check(M, H, W)) return rc;
    if (Sh < 1 || Sw < 1 || Sh > MI_CLIP_TILES_MAX_SIZE || Sw > MI_CLIP_TILES_MAX_SIZE)
        return fail(MI_RAST_ERR_INVALID, "clip tiles: need 1 <= Sh, Sw <= 512 (MI_CLIP_TILES_MAX_SIZE)");
    if (layout != MI_CLIP_TILES_CROP && layout != MI_CLIP_TILES_PAD_SQUARE)
        return fail(MI_RAST_ERR_INVALID, "clip tiles: layout must be MI_CLIP_TILES_CROP or MI_CLIP_TILES_PAD_SQUARE");
    if (!packed || !image || !rects || !mean || !std || !tiles) return fail(MI_RAST_ERR_INVALID, "clip tiles: null pointer");
    if (!(background == background)) return fail(MI_RAST_ERR_INVALID, "clip tiles: background is NaN");
    CtNorm nrm;
    for (int c = 0; c < 3; c++) {
        nrm.mean[c] = mean[c];
        nrm.std[c] = std[c];
        if (!(mean[c] == mean[c]) || !(std[c] == std[c]) || std[c] == 0.f)
            return fail(MI_RAST_ERR_INVALID, "clip tiles: need mean and std without NaN and std != 0");
    }
    const uint64_t* p = (const uint64_t*)packed;
    if (antialias) {
        if (half)
            ct_launch<true, __half>(M, H, W, p, image, rects, layout, background, nrm, Sh, Sw, tiles, stream);
        else
            ct_launch<true, float>(M, H, W, p, image, rects, layout, background, nrm, Sh, Sw, tiles, stream);
    } else {
        if (half)
            ct_launch<false, __half>(M, H, W, p, image, rects, layout, background, nrm, Sh, Sw, tiles, stream);
        else
            ct_launch<false, float>(M, H, W, p, image, rects, layout, background, nrm, Sh, Sw, tiles, stream);
    }
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_mask_index_map(int M, int H, int W, const unsigned long long* packed, int offset, int* out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ct_check(M, H, W)) return rc;
    if (offset < 0 || offset > 0x7fffffff - PM_MAX_MASKS)
        return fail(MI_RAST_ERR_INVALID, "mask index map: need 0 <= offset <= 2^31 - 1 - 1024");
    if (!packed || !out) return fail(MI_RAST_ERR_INVALID, "clip tiles: null pointer");
    const size_t NW = pm_words(1, H, W);   // one wave per word of the image
    constexpr int wpb = CT_THREADS / 64;
    hipLaunchKernelGGL(ct_index_map_kernel, dim3((unsigned)((NW + wpb - 1) / wpb)), dim3(CT_THREADS), 0, stream, M, H, W, pm_row_words(W),
                       (const uint64_t*)packed, offset, out);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
