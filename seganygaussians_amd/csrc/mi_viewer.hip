// mi_viewer.hip -- C-ABI implementation of include/mi_viewer.h.
#include "host.h"
#include "../../include/mi_viewer.h"

#include "viewer.h"        // feature moments for the PCA basis, the fused display frame

using namespace mirast;

namespace {
size_t view_mom_gram_bytes(int n, int C) { return (size_t)view_mom_groups(n, C) * view_mom_pairs(C) * 1024 * sizeof(double); }
size_t view_mom_sum_bytes(int n, int C) { return (size_t)view_mom_groups(n, C) * 32 * view_mom_blocks(C) * sizeof(double); }

template <int VEC, int QT>
void view_launch_frame(const ViewFrameArgs& a, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.N / VEC + VIEW_THREADS - 1) / VIEW_THREADS));
    if (a.modes & MI_VIEW_PCA) hipLaunchKernelGGL((view_frame_kernel<VEC, QT, true>), grid, dim3(VIEW_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((view_frame_kernel<VEC, QT, false>), grid, dim3(VIEW_THREADS), 0, stream, a);
}

template <int VEC>
void view_launch_frame_q(const ViewFrameArgs& a, hipStream_t stream)
{
    if (a.Q == 0) view_launch_frame<VEC, 0>(a, stream);
    else if (a.Q == 1) view_launch_frame<VEC, 1>(a, stream);
    else if (a.Q <= 4) view_launch_frame<VEC, 4>(a, stream);
    else view_launch_frame<VEC, 16>(a, stream);
}
}  // namespace

extern "C" {

size_t mi_view_moments_workspace_bytes(int n, int C)
{
    if (n < 1 || C < 1 || C > MI_SEGMENT_MAX_CHANNELS) return 0;
    return view_mom_gram_bytes(n, C) + view_mom_sum_bytes(n, C);
}

int mi_view_moments_block(void) { return VIEW_MOM_B; }

int mi_view_moments(int layout, int N, int C, const float* features, const long long* index, int n, int pre, void* workspace,
                    size_t workspace_bytes, double* mean, double* cov, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (layout != MI_SEGMENT_IMAGE && layout != MI_SEGMENT_POINTS) return fail(MI_RAST_ERR_INVALID, "view moments: layout must be MI_SEGMENT_IMAGE or MI_SEGMENT_POINTS");
    if (N < 1 || C < 1 || C > MI_SEGMENT_MAX_CHANNELS) return fail(MI_RAST_ERR_INVALID, "view moments: need N >= 1 and 1 <= C <= 256");
    if (n < 1 || (!index && n > N)) return fail(MI_RAST_ERR_INVALID, "view moments: need n >= 1 rows, and n <= N without an index");
    if (pre != MI_SEGMENT_PRE_NONE && pre != MI_SEGMENT_PRE_L2 && pre != MI_SEGMENT_PRE_EPS)
        return fail(MI_RAST_ERR_INVALID, "view moments: pre must be MI_SEGMENT_PRE_NONE, _L2 or _EPS");
    if (!features || !mean || !cov) return fail(MI_RAST_ERR_INVALID, "view moments: null pointer");
    if (!workspace || workspace_bytes < mi_view_moments_workspace_bytes(n, C) || (uintptr_t)workspace % 8)
        return fail(MI_RAST_ERR_INVALID, "view moments: the workspace is null, misaligned or smaller than mi_view_moments_workspace_bytes");
    const int G = view_mom_groups(n, C), per_group = 4 * view_mom_pairs_per_wave(C);
    ViewMomArgs a{features, index, N, n, C, layout, pre, (double*)workspace, (double*)((char*)workspace + view_mom_gram_bytes(n, C))};
    const dim3 grid((unsigned)G, (unsigned)((view_mom_pairs(C) + per_group - 1) / per_group));
    if (view_mom_pairs_per_wave(C) == 1) hipLaunchKernelGGL((view_moments_kernel<1>), grid, dim3(VIEW_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((view_moments_kernel<3>), grid, dim3(VIEW_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    constexpr int outs = VIEW_THREADS / VIEW_RED_SLICES;
    hipLaunchKernelGGL(view_moments_reduce_kernel, dim3((unsigned)((C * C + outs - 1) / outs)), dim3(VIEW_THREADS), 0, stream, a, G,
                       mean, cov);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_view_frame(int N, int C, const float* features, const float* rgb, const float* cluster_rgb, const float* proj, int Q,
                  const float* queries, const float* gates, float threshold, int modes, int preview, float* frame, unsigned char* mask,
                  float* score, void* stream_)
{
    if (N < 1 || C < 1 || C > MI_SEGMENT_MAX_CHANNELS) return fail(MI_RAST_ERR_INVALID, "view frame: need N >= 1 and 1 <= C <= 256");
    if (Q < 0 || Q > MI_SEGMENT_MAX_QUERIES) return fail(MI_RAST_ERR_INVALID, "view frame: need 0 <= Q <= 16 queries");
    if (modes < 1 || modes > (MI_VIEW_RGB | MI_VIEW_PCA | MI_VIEW_CLUSTER | MI_VIEW_SIMILARITY))
        return fail(MI_RAST_ERR_INVALID, "view frame: modes must be a non-empty OR of MI_VIEW_RGB, _PCA, _CLUSTER, _SIMILARITY");
    if (!features || !rgb || !frame) return fail(MI_RAST_ERR_INVALID, "view frame: null pointer");
    if ((modes & MI_VIEW_PCA) && !proj) return fail(MI_RAST_ERR_INVALID, "view frame: MI_VIEW_PCA needs the basis");
    if (Q > 0 && (!queries || !mask || !score)) return fail(MI_RAST_ERR_INVALID, "view frame: queries need mask and score outputs");
    if (Q > 0 && !(threshold == threshold)) return fail(MI_RAST_ERR_INVALID, "view frame: the threshold is NaN");
    ViewFrameArgs a{features, rgb, cluster_rgb, proj, Q > 0 ? queries : nullptr, gates, N, C, Q, modes, preview ? 1 : 0, threshold,
                    frame, mask, score};
    const uintptr_t addr = (uintptr_t)features | (uintptr_t)rgb | (uintptr_t)cluster_rgb | (uintptr_t)frame;
    hipStream_t stream = (hipStream_t)stream_;
    if (N % 4 == 0 && addr % 16 == 0) view_launch_frame_q<4>(a, stream);
    else if (N % 2 == 0 && addr % 8 == 0) view_launch_frame_q<2>(a, stream);
    else view_launch_frame_q<1>(a, stream);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
