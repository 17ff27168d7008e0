// mi_segment.hip -- C-ABI implementation of include/mi_segment.h.
#include "host.h"
#include "../../include/mi_segment.h"

#include "segment.h"       // segmentation queries: scores, selection, cluster assignment

using namespace mirast;

namespace {
int seg_check(int layout, int N, int C, int Q, int max_q, const char* what, const void* features, const void* queries, int pre)
{
    if (layout != MI_SEGMENT_IMAGE && layout != MI_SEGMENT_POINTS) return fail(MI_RAST_ERR_INVALID, "segment: layout must be MI_SEGMENT_IMAGE or MI_SEGMENT_POINTS");
    if (N < 1 || C < 1 || C > MI_SEGMENT_MAX_CHANNELS) return fail(MI_RAST_ERR_INVALID, "segment: need N >= 1 and 1 <= C <= 256");
    if (Q < 1 || Q > max_q) return fail(MI_RAST_ERR_INVALID, std::string("segment: need 1 <= ") + what);
    if (pre != MI_SEGMENT_PRE_NONE && pre != MI_SEGMENT_PRE_L2 && pre != MI_SEGMENT_PRE_EPS)
        return fail(MI_RAST_ERR_INVALID, "segment: pre must be MI_SEGMENT_PRE_NONE, _L2 or _EPS");
    if (!features || !queries) return fail(MI_RAST_ERR_INVALID, "segment: null pointer");
    return MI_RAST_OK;
}

template <int QT>
void seg_launch_stream(int layout, const SegArgs& a, hipStream_t stream)
{
    const uintptr_t addr = (uintptr_t)a.feat;
    if (layout == MI_SEGMENT_IMAGE) {
        const int vec = (a.N % 4 == 0 && addr % 16 == 0) ? 4 : (a.N % 2 == 0 && addr % 8 == 0) ? 2 : 1;
        const dim3 grid((unsigned)((a.N / vec + SEG_THREADS - 1) / SEG_THREADS));
        if (vec == 4) hipLaunchKernelGGL((seg_image_kernel<4, QT>), grid, dim3(SEG_THREADS), 0, stream, a);
        else if (vec == 2) hipLaunchKernelGGL((seg_image_kernel<2, QT>), grid, dim3(SEG_THREADS), 0, stream, a);
        else hipLaunchKernelGGL((seg_image_kernel<1, QT>), grid, dim3(SEG_THREADS), 0, stream, a);
    } else {
        constexpr int rows = SEG_POINT_ITERS * SEG_THREADS / SEG_POINT_LANES;
        const int wide = (a.C % 4 == 0 && addr % 16 == 0) ? 1 : 0;
        hipLaunchKernelGGL((seg_points_kernel<QT>), dim3((unsigned)((a.N + rows - 1) / rows)), dim3(SEG_THREADS), 0, stream, a, wide);
    }
}

// scores, select and assign with K <= 16: one kernel, the queries padded to 1, 4 or 16 columns
int seg_stream(int layout, const SegArgs& a, hipStream_t stream)
{
    if (a.Q == 1) seg_launch_stream<1>(layout, a, stream);
    else if (a.Q <= 4) seg_launch_stream<4>(layout, a, stream);
    else seg_launch_stream<16>(layout, a, stream);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

template <int NS>
void seg_launch_mfma(int layout, const SegArgs& a, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.N + SEG_GEMM_ROWS - 1) / SEG_GEMM_ROWS));
    if (layout == MI_SEGMENT_IMAGE) hipLaunchKernelGGL((seg_assign_mfma_kernel<NS, true>), grid, dim3(SEG_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((seg_assign_mfma_kernel<NS, false>), grid, dim3(SEG_THREADS), 0, stream, a);
}
}  // namespace

extern "C" {

int mi_segment_scores(int layout, int N, int C, int Q, const float* features, const float* queries, const float* gates, int pre, int post,
                      float* scores, void* stream_)
{
    if (int rc = seg_check(layout, N, C, Q, MI_SEGMENT_MAX_QUERIES, "Q <= 16 queries", features, queries, pre)) return rc;
    if (!scores) return fail(MI_RAST_ERR_INVALID, "segment: null output");
    SegArgs a{features, queries, gates, N, C, Q, pre, post ? 1 : 0, SEG_SCORES, 0, 0.f, scores, nullptr, nullptr};
    return seg_stream(layout, a, (hipStream_t)stream_);
}

int mi_segment_select(int layout, int N, int C, int Q, const float* features, const float* queries, const float* gates, int pre,
                      int half_shift, float threshold, unsigned char* mask, float* score, void* stream_)
{
    if (int rc = seg_check(layout, N, C, Q, MI_SEGMENT_MAX_QUERIES, "Q <= 16 queries", features, queries, pre)) return rc;
    if (!mask || !score) return fail(MI_RAST_ERR_INVALID, "segment: null output");
    if (!(threshold == threshold)) return fail(MI_RAST_ERR_INVALID, "segment: the threshold is NaN");
    SegArgs a{features, queries, gates, N, C, Q, pre, 1, SEG_SELECT, half_shift ? 1 : 0, threshold, score, mask, nullptr};
    return seg_stream(layout, a, (hipStream_t)stream_);
}

int mi_segment_assign(int layout, int N, int C, int K, const float* features, const float* centers, const float* gates, int pre,
                      int* labels, float* best, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = seg_check(layout, N, C, K, MI_SEGMENT_MAX_CENTERS, "K <= 4096 centres", features, centers, pre)) return rc;
    if (!labels || !best) return fail(MI_RAST_ERR_INVALID, "segment: null output");
    SegArgs a{features, centers, gates, N, C, K, pre, 1, SEG_ASSIGN, 0, 0.f, best, nullptr, labels};
    if (K <= MI_SEGMENT_MAX_QUERIES) return seg_stream(layout, a, stream);
    switch (seg_assign_steps(C)) {
        case 16: seg_launch_mfma<16>(layout, a, stream); break;
        case 32: seg_launch_mfma<32>(layout, a, stream); break;
        case 64: seg_launch_mfma<64>(layout, a, stream); break;
        default: seg_launch_mfma<128>(layout, a, stream); break;
    }
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_segment_assign_block(int C)
{
    if (C < 1 || C > MI_SEGMENT_MAX_CHANNELS) return 0;
    return seg_assign_block(seg_assign_steps(C));
}

}  // extern "C"
