// seg_row.h -- the row arithmetic of the segmentation queries (include/mi_segment.h), shared by the kernels
// of segment.h and by the fused viewer frame of viewer.h: inline device functions only, the way wave.h is shared.  One pass over a
// feature row accumulates n1 = sum f^2, n2 = sum (f g)^2 and d_k = sum (f g) q_k as fmaf chains; seg_row_scale() turns (n1, n2)
// into the factor that makes s_k = d_k * scale the gated, normalised similarity of the header; seg_select() is the GUI's decision
// on those s_k.  The build uses -ffp-contract=off, so two kernels that walk a row in the same order through these functions give
// the same bits.
#pragma once

#include "../../include/mi_segment.h"
#include <hip/hip_runtime.h>

namespace mirast {

// s_k = d_k * scale: a = u / f of the header's `pre`, then F.normalize of v = a (f g) when post is set
__device__ inline float seg_row_scale(float n1, float n2, int pre, int post)
{
    float a = 1.f;
    if (pre == MI_SEGMENT_PRE_L2) a = 1.f / fmaxf(sqrtf(n1), 1e-12f);
    else if (pre == MI_SEGMENT_PRE_EPS) a = 1.f / (sqrtf(n1) + 1e-6f);
    if (post) a = a / fmaxf(a * sqrtf(n2), 1e-12f);
    return a;
}

template <int QT>
__device__ inline void seg_accumulate(float f, float g, const float* __restrict__ qc, float& n1, float& n2, float (&d)[QT])
{
    const float t = f * g;
    n1 = fmaf(f, f, n1);
    n2 = fmaf(t, t, n2);
#pragma unroll
    for (int k = 0; k < QT; k++) d[k] = fmaf(t, qc[k], d[k]);
}

// select: t_k = (s_k + 1) / 2 with half_shift, else s_k; any = some t_k > threshold, top = max_k (t_k > threshold ? t_k : 0)
template <int QT>
__device__ inline void seg_select(const float (&d)[QT], float scale, int Q, int half_shift, float threshold, bool& any, float& top)
{
    any = false;
    top = -INFINITY;
#pragma unroll
    for (int k = 0; k < QT; k++)
        if (k < Q) {
            float t = d[k] * scale;
            if (half_shift) t = (t + 1.f) * 0.5f;
            const bool b = t > threshold;
            any = any || b;
            top = fmaxf(top, b ? t : 0.f);
        }
}

}  // namespace mirast
