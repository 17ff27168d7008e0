// mi_mask_sets.hip -- C-ABI implementation of include/mi_mask_sets.h.
#include "host.h"
#include "../../include/mi_mask_sets.h"

#include "mask_sets.h"   // set operations on packed SAM masks: overlaps, boxes, NMS decision, score images

using namespace mirast;

namespace {
int mset_check(int M, int H, int W)
{
    if (int rc = pm_check_dims("mask sets", M, H, W)) return rc;
    return pm_pixels_ok(H, W) ? MI_RAST_OK : fail(MI_RAST_ERR_INVALID, "mask sets: need H * W < 2^24 pixels (every count is then exact in f32)");
}

template <int MODE>
void mset_launch_images(int M, int H, int W, int K, const uint64_t* packed, const float* scores, float* out, hipStream_t stream)
{
    const int Wq = pm_row_words(W);
    const size_t NW = (size_t)H * Wq;
    const dim3 grid((unsigned)((NW + MSET_SI_WORDS - 1) / MSET_SI_WORDS)), block(MSET_SI_THREADS);
    if (K == 1)
        hipLaunchKernelGGL((mset_score_images_kernel<1, MODE>), grid, block, 0, stream, M, H, W, Wq, K, packed, scores, out);
    else if (K <= 4)
        hipLaunchKernelGGL((mset_score_images_kernel<4, MODE>), grid, block, 0, stream, M, H, W, Wq, K, packed, scores, out);
    else if (K <= 16)
        hipLaunchKernelGGL((mset_score_images_kernel<16, MODE>), grid, block, 0, stream, M, H, W, Wq, K, packed, scores, out);
    else
        hipLaunchKernelGGL((mset_score_images_kernel<64, MODE>), grid, block, 0, stream, M, H, W, Wq, K, packed, scores, out);
}
}  // namespace

extern "C" {

int mi_mask_overlaps(int M, int H, int W, const unsigned long long* packed, const long long* order, int* inter, long long* areas,
                     void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = mset_check(M, H, W)) return rc;
    if (!packed || !inter) return fail(MI_RAST_ERR_INVALID, "mask sets: null pointer");
    const size_t NW = (size_t)H * pm_row_words(W);
    const int T = (M + MSET_OV_TILE - 1) / MSET_OV_TILE, tiles = mset_upper_tiles(T);
    // slices of the words, whole chunks each, so that tiles x slices gives every CU the three workgroups its registers admit at
    // small M (the kernel is bound by its vector popcounts, so it wants the waves); more slices would only add atomics
    const size_t chunks = (NW + MSET_OV_CHUNK - 1) / MSET_OV_CHUNK;
    size_t slices = (size_t)(768 + tiles - 1) / tiles;
    if (slices > chunks) slices = chunks;
    const size_t per = (chunks + slices - 1) / slices * MSET_OV_CHUNK;
    slices = (NW + per - 1) / per;
    HIP_TRY(hipMemsetAsync(inter, 0, (size_t)M * M * sizeof(int), stream));
    hipLaunchKernelGGL(mset_overlap_kernel, dim3((unsigned)tiles, (unsigned)slices), dim3(MSET_OV_THREADS), 0, stream, M, NW, per,
                       (const uint64_t*)packed, order, inter);
    hipLaunchKernelGGL(mset_overlap_finish_kernel, dim3((unsigned)(((size_t)M * M + 255) / 256)), dim3(256), 0, stream, M, inter, areas);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_mask_boxes(int M, int H, int W, const unsigned long long* packed, float* boxes, long long* areas, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = mset_check(M, H, W)) return rc;
    if (!packed || !boxes) return fail(MI_RAST_ERR_INVALID, "mask sets: null pointer");
    hipLaunchKernelGGL(mset_boxes_kernel, dim3((unsigned)M), dim3(MSET_BOX_THREADS), 0, stream, H, pm_row_words(W),
                       (const uint64_t*)packed, boxes, areas);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_mask_nms_keep(int M, const int* inter, const long long* areas, const float* scores, float iou_thr, float score_thr,
                     float inner_max, unsigned char* keep, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 1 || M > MSET_NMS_MAX) return fail(MI_RAST_ERR_INVALID, "mask nms: need 1 <= M <= 1024 masks");
    if (!inter || !areas || !scores || !keep) return fail(MI_RAST_ERR_INVALID, "mask nms: null pointer");
    if (iou_thr != iou_thr || score_thr != score_thr || inner_max != inner_max)
        return fail(MI_RAST_ERR_INVALID, "mask nms: a threshold is NaN");
    hipLaunchKernelGGL(mset_nms_kernel, dim3(1), dim3((unsigned)((M + 63) / 64 * 64)), 0, stream, M, inter, areas, scores, iou_thr,
                       score_thr, inner_max, keep);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_mask_score_images(int M, int H, int W, int K, const unsigned long long* packed, const float* scores, int mode, float* out,
                         void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = mset_check(M, H, W)) return rc;
    if (K < 1 || K > MI_MASK_SCORE_MAX_COLUMNS) return fail(MI_RAST_ERR_INVALID, "mask score images: need 1 <= K <= 64 score columns");
    if (mode != MI_MASK_SCORE_SUM && mode != MI_MASK_SCORE_MEAN && mode != MI_MASK_SCORE_MAX)
        return fail(MI_RAST_ERR_INVALID, "mask score images: mode must be MI_MASK_SCORE_SUM, _MEAN or _MAX");
    if (!packed || !scores || !out) return fail(MI_RAST_ERR_INVALID, "mask score images: null pointer");
    static_assert(MSET_SI_SUM == MI_MASK_SCORE_SUM && MSET_SI_MEAN == MI_MASK_SCORE_MEAN && MSET_SI_MAX == MI_MASK_SCORE_MAX, "modes");
    const uint64_t* p = (const uint64_t*)packed;
    if (mode == MI_MASK_SCORE_SUM)
        mset_launch_images<MSET_SI_SUM>(M, H, W, K, p, scores, out, stream);
    else if (mode == MI_MASK_SCORE_MEAN)
        mset_launch_images<MSET_SI_MEAN>(M, H, W, K, p, scores, out, stream);
    else
        mset_launch_images<MSET_SI_MAX>(M, H, W, K, p, scores, out, stream);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
