// mi_mask_scales.hip -- C-ABI implementation of include/mi_mask_scales.h.
#include "host.h"
#include "../../include/mi_mask_scales.h"

#include "mask_scales.h"   // SAM-mask 3-D scales: erosion and per-mask point spread

using namespace mirast;

namespace {
int ms_check(int M, int H, int W, const char* what)
{
    if (int rc = pm_check_dims("mask scales", M, H, W, what)) return rc;
    return pm_words(M, H, W) < ((size_t)1 << 31) ? MI_RAST_OK : fail(MI_RAST_ERR_INVALID, "mask scales: more than 2^31 mask words");
}
}  // namespace

extern "C" {

size_t mi_mask_scales_workspace_bytes(int M, int H, int W)
{
    if (M < 1 || H < 1 || W < 1) return 0;
    return (size_t)M * pm_tiles(H, W, MS_TILE_ROWS) * MS_STATS * sizeof(double);
}

int mi_mask_erode_min_sum(int M, int h, int w, const unsigned long long* packed_in, int H, int W, float min_sum,
                          unsigned long long* packed_out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ms_check(M, h, w, "h, w")) return rc;
    if (int rc = ms_check(M, H, W, "H, W")) return rc;
    if (!packed_in || !packed_out) return fail(MI_RAST_ERR_INVALID, "mask scales: null pointer");
    if (!(min_sum == min_sum)) return fail(MI_RAST_ERR_INVALID, "mask scales: min_sum is NaN");
    const int Wqi = pm_row_words(w), Wq = pm_row_words(W);
    const size_t words = pm_words(M, H, W);
    if (pm_overlap(packed_in, pm_words(M, h, w), packed_out, words))
        return fail(MI_RAST_ERR_INVALID, "mask scales: the eroded masks must not overlap the input masks");
    if (h == H && w == W) {
        // the window holds an integer 0 .. 9: count >= min_sum is count >= ceil(min_sum); 10 is "never"
        const int k = min_sum <= 0.f ? 0 : min_sum > 9.f ? 10 : (int)ceilf(min_sum);
        hipLaunchKernelGGL(ms_erode_same_kernel, dim3((unsigned)((words + MS_THREADS - 1) / MS_THREADS)), dim3(MS_THREADS), 0, stream,
                           M, H, W, Wq, (const uint64_t*)packed_in, k, (uint64_t*)packed_out);
    } else {
        // area_pixel_compute_scale (align_corners=False, no scale factor): (float)in / out
        const float scale_h = (float)h / (float)H, scale_w = (float)w / (float)W;
        constexpr int wpb = MS_THREADS / 64;
        hipLaunchKernelGGL(ms_erode_resample_kernel, dim3((unsigned)((words + wpb - 1) / wpb)), dim3(MS_THREADS), 0, stream,
                           M, h, w, Wqi, (const uint64_t*)packed_in, H, W, Wq, scale_h, scale_w, min_sum, (uint64_t*)packed_out);
    }
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_mask_erode(int M, int h, int w, const unsigned long long* packed_in, int H, int W, unsigned long long* packed_out, void* stream)
{
    return mi_mask_erode_min_sum(M, h, w, packed_in, H, W, 5.f, packed_out, stream);
}

int mi_mask_resize(int M, int h, int w, const unsigned long long* packed_in, int H, int W, float threshold,
                   unsigned long long* packed_out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ms_check(M, h, w, "h, w")) return rc;
    if (int rc = ms_check(M, H, W, "H, W")) return rc;
    if (!pm_pixels_ok(h, w) || !pm_pixels_ok(H, W)) return fail(MI_RAST_ERR_INVALID, "mask resize: need h * w and H * W < 2^24 pixels");
    if (!packed_in || !packed_out) return fail(MI_RAST_ERR_INVALID, "mask scales: null pointer");
    if (!(threshold == threshold)) return fail(MI_RAST_ERR_INVALID, "mask resize: threshold is NaN");
    const size_t words = pm_words(M, H, W);
    if (pm_overlap(packed_in, pm_words(M, h, w), packed_out, words))
        return fail(MI_RAST_ERR_INVALID, "mask resize: the resized masks must not overlap the input masks");
    const float scale_h = (float)h / (float)H, scale_w = (float)w / (float)W;   // as in mi_mask_erode_min_sum
    constexpr int wpb = MS_THREADS / 64;
    hipLaunchKernelGGL(ms_resize_kernel, dim3((unsigned)((words + wpb - 1) / wpb)), dim3(MS_THREADS), 0, stream, M, h, w, pm_row_words(w),
                       (const uint64_t*)packed_in, H, W, pm_row_words(W), scale_h, scale_w, threshold, (uint64_t*)packed_out);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_mask_scales(int M, int H, int W, const unsigned long long* eroded, const float* depth, double fx, double fy, void* workspace,
                   size_t workspace_bytes, float* scales, long long* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ms_check(M, H, W, "H, W")) return rc;
    if (!eroded || !depth || !workspace || !scales || !counts) return fail(MI_RAST_ERR_INVALID, "mask scales: null pointer");
    if (!(fx > 0.0) || !(fy > 0.0)) return fail(MI_RAST_ERR_INVALID, "mask scales: need focal lengths fx, fy > 0");
    if (workspace_bytes < mi_mask_scales_workspace_bytes(M, H, W))
        return fail(MI_RAST_ERR_INVALID, "mask scales: workspace smaller than mi_mask_scales_workspace_bytes(M, H, W)");
    const size_t T = pm_tiles(H, W, MS_TILE_ROWS);
    if (T >= ((size_t)1 << 31)) return fail(MI_RAST_ERR_INVALID, "mask scales: image too large");
    hipLaunchKernelGGL(ms_moments_kernel, dim3((unsigned)T), dim3(64), 0, stream, M, H, W, pm_row_words(W), (const uint64_t*)eroded, depth,
                       fx, fy, (int)T, (double*)workspace);
    hipLaunchKernelGGL(ms_finalize_kernel, dim3((unsigned)M), dim3(MS_THREADS), 0, stream, (int)T, (const double*)workspace, scales, counts);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
