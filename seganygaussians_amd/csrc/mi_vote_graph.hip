// mi_vote_graph.hip -- C-ABI implementation of include/mi_vote_graph.h.
#include "host.h"
#include "../../include/mi_vote_graph.h"

#include "packed_masks.h"  // the layout of the eroded masks
#include "vote_graph.h"    // language-segmentation vote graph: mask features, anchor bits, relevancy

using namespace mirast;

namespace {
bool vg_mask_sizes_ok(int M, int C, int h, int w)
{
    return M >= 1 && M <= PM_MAX_MASKS && C >= 1 && C <= MI_SEGMENT_MAX_CHANNELS && h >= 1 && w >= 1 &&
           (size_t)C * h * w < ((size_t)1 << 31) && pm_words(M, h, w) < ((size_t)1 << 31);
}
}  // namespace

extern "C" {

size_t mi_vote_mask_features_workspace_bytes(int M, int C, int h, int w)
{
    if (!vg_mask_sizes_ok(M, C, h, w)) return 0;
    Carver cv;
    cv.take((size_t)C * h * w * sizeof(float));
    cv.take((size_t)M * pm_tiles(h, w, VG_TILE_ROWS) * sizeof(double));
    cv.take((size_t)M * pm_tiles(h, w, VG_TILE_ROWS) * C * sizeof(double));
    return cv.off;
}

int mi_vote_mask_features(int M, int C, int H, int W, const float* rendered, int h, int w, const unsigned long long* eroded,
                          const float* gates, void* workspace, size_t workspace_bytes, float* features, long long* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!vg_mask_sizes_ok(M, C, h, w) || H < 1 || W < 1 || (size_t)C * H * W >= ((size_t)1 << 31))
        return fail(MI_RAST_ERR_INVALID, "vote graph: need 1 <= M <= 1024 masks, 1 <= C <= 256 channels and images of 1 .. 2^31 - 1 values");
    if (!rendered || !eroded || !gates || !workspace || !features) return fail(MI_RAST_ERR_INVALID, "vote graph: null pointer");
    if (workspace_bytes < mi_vote_mask_features_workspace_bytes(M, C, h, w))
        return fail(MI_RAST_ERR_INVALID, "vote graph: workspace smaller than mi_vote_mask_features_workspace_bytes(M, C, h, w)");
    if ((uintptr_t)workspace % 8) return fail(MI_RAST_ERR_INVALID, "vote graph: the workspace must be 8-byte aligned");
    const size_t T = pm_tiles(h, w, VG_TILE_ROWS);
    Carver cv;
    char* base = (char*)workspace;
    float* fs = (float*)(base + cv.take((size_t)C * h * w * sizeof(float)));
    double* tile_counts = (double*)(base + cv.take((size_t)M * T * sizeof(double)));
    double* tile_sums = (double*)(base + cv.take((size_t)M * T * C * sizeof(double)));
    const size_t n = (size_t)C * h * w;
    hipLaunchKernelGGL(vg_resample_kernel, dim3((unsigned)((n + VG_THREADS - 1) / VG_THREADS)), dim3(VG_THREADS), 0, stream, C, H, W,
                       rendered, h, w, (double)H / (double)h, (double)W / (double)w, fs);
    hipLaunchKernelGGL(vg_mask_sums_kernel, dim3((unsigned)T, (unsigned)((M + VG_MASK_GROUP - 1) / VG_MASK_GROUP)), dim3(64), 0, stream, M, C, h, w, pm_row_words(w), (const uint64_t*)eroded,
                       (const float*)fs, gates, (int)T, tile_counts, tile_sums);
    hipLaunchKernelGGL(vg_mask_finalize_kernel, dim3((unsigned)M), dim3(VG_THREADS), 0, stream, C, (int)T, (const double*)tile_counts,
                       (const double*)tile_sums, gates, features, counts);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_vote_anchor_bits(int M, int A, int C, const float* mask_features, const float* gates, const float* anchors, float threshold,
                        int* bits, int* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 1 || M > MI_CLUSTER_MAX_POINTS || A < 1 || A > MI_VOTE_MAX_ANCHORS || C < 1 || C > MI_SEGMENT_MAX_CHANNELS)
        return fail(MI_RAST_ERR_INVALID, "vote graph: need 1 <= M <= 2^20 rows, 1 <= A <= 32768 anchors and 1 <= C <= 256 channels");
    if (!mask_features || !gates || !anchors || !bits) return fail(MI_RAST_ERR_INVALID, "vote graph: null pointer");
    if (!(threshold == threshold)) return fail(MI_RAST_ERR_INVALID, "vote graph: the threshold is NaN");
    const int words = (A + 31) / 32;
    constexpr int rows = 32 * VG_THREADS / 64;   // a wave per 32 masks
    const dim3 grid((unsigned)((M + rows - 1) / rows), (unsigned)words);
    const int wide = C % 4 == 0 && ((uintptr_t)mask_features | (uintptr_t)gates | (uintptr_t)anchors) % 16 == 0;
    hipLaunchKernelGGL(vg_anchor_bits_kernel, grid, dim3(VG_THREADS), 0, stream, M, A, C, mask_features, gates, anchors, threshold, words,
                       wide, bits);
    if (counts)
        hipLaunchKernelGGL(vg_popcount_kernel, dim3((unsigned)((M + VG_THREADS / 64 - 1) / (VG_THREADS / 64))), dim3(VG_THREADS), 0, stream,
                           M, words, (const int*)bits, counts);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_vote_relevancy(int N, int D, int P, int Q, const void* embeds, int embeds_f16, const float* pos, const float* neg, int normalize,
                      float* out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    static_assert(64 * VG_CR_SLOTS == MI_VOTE_MAX_EMBED_DIM, "a wave holds a whole row");
    if (N < 1 || D < 1 || D > MI_VOTE_MAX_EMBED_DIM || (size_t)N * D >= ((size_t)1 << 40))
        return fail(MI_RAST_ERR_INVALID, "vote graph: need N >= 1 rows and 1 <= D <= 1024");
    if (P < 1 || P > MI_VOTE_MAX_PROMPTS || Q < 1 || Q > MI_VOTE_MAX_PROMPTS)
        return fail(MI_RAST_ERR_INVALID, "vote graph: need 1 <= P, Q <= 16 prompt embeddings");
    if (!embeds || !pos || !neg || !out) return fail(MI_RAST_ERR_INVALID, "vote graph: null pointer");
    constexpr int rows = VG_CR_ROWS * VG_THREADS / 64;
    const dim3 grid((unsigned)(((size_t)N + rows - 1) / rows));
    if (embeds_f16)
        hipLaunchKernelGGL((vg_relevancy_kernel<_Float16>), grid, dim3(VG_THREADS), 0, stream, N, D, P, Q, (const _Float16*)embeds, pos, neg,
                           normalize ? 1 : 0, out);
    else
        hipLaunchKernelGGL((vg_relevancy_kernel<float>), grid, dim3(VG_THREADS), 0, stream, N, D, P, Q, (const float*)embeds, pos, neg,
                           normalize ? 1 : 0, out);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
