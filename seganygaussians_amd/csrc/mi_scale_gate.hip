// mi_scale_gate.hip -- C-ABI implementation of include/mi_scale_gate.h, scale conditioning.  Every entry point
// checks its arguments, launches ONE kernel on the caller's stream and returns: nothing is allocated, copied or waited for.
#include "host.h"
#include "../../include/mi_scale_gate.h"

#include "scale_gate.h"   // the quantile table, the uniform transform, the gates and their backward

using namespace mirast;

namespace {

constexpr int SG_MAX_N = (1 << 30) - 1;     // row numbers and their strides stay ints

static_assert(SG_MAX_QUANTILES == MI_SCALE_MAX_QUANTILES && SG_MAX_CHANNELS == MI_SCALE_MAX_CHANNELS, "limits");
static_assert(SG_MODE_NONE == MI_SCALE_GATE_NONE && SG_MODE_LEARNED == MI_SCALE_GATE_LEARNED && SG_MODE_FIXED == MI_SCALE_GATE_FIXED, "modes");

int check_sizes(int n, int nq)
{
    if (n < 1 || n > SG_MAX_N) return fail(MI_RAST_ERR_INVALID, "scale gate: need 1 <= n < 2^30 scales");
    if (nq < 1 || nq > MI_SCALE_MAX_QUANTILES) return fail(MI_RAST_ERR_INVALID, "scale gate: need 1 <= nq <= 1024 quantiles");
    return MI_RAST_OK;
}

int check_channels(int channels)
{
    if (channels < 1 || channels > MI_SCALE_MAX_CHANNELS) return fail(MI_RAST_ERR_INVALID, "scale gate: need 1 <= channels <= 256");
    return MI_RAST_OK;
}

}  // namespace

extern "C" {

int mi_scale_quantile_fit(int n, const float* sorted, int nq, const double* references, double* quantiles, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_sizes(n, nq)) return rc;
    if (!sorted || !references || !quantiles) return fail(MI_RAST_ERR_INVALID, "scale gate: null pointer");
    const Range r[3] = {{(const char*)quantiles, (size_t)nq * sizeof(double), true}, {(const char*)sorted, (size_t)n * sizeof(float), false},
                        {(const char*)references, (size_t)nq * sizeof(double), false}};
    if (outputs_overlap(r, 3)) return fail(MI_RAST_ERR_INVALID, "scale gate: an output overlaps another tensor of the call");
    hipLaunchKernelGGL(scale_quantile_fit_kernel, dim3(1), dim3(SG_MAX_QUANTILES), 0, stream, n, sorted, nq, references, quantiles);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_scale_gate_forward(int n, const float* scales, int nq, const double* quantiles, const double* references, int mode, int channels,
                          const float* weight, const float* bias, int scale_aware_dim, float* u, float* gates, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_sizes(n, nq)) return rc;
    if (mode != MI_SCALE_GATE_NONE && mode != MI_SCALE_GATE_LEARNED && mode != MI_SCALE_GATE_FIXED)
        return fail(MI_RAST_ERR_INVALID, "scale gate: unknown gate mode");
    if (!scales || !quantiles || !references) return fail(MI_RAST_ERR_INVALID, "scale gate: null pointer");
    Range r[7] = {{(const char*)u, u ? (size_t)n * sizeof(float) : 0, true}, {(const char*)scales, (size_t)n * sizeof(float), false},
                  {(const char*)quantiles, (size_t)nq * sizeof(double), false}, {(const char*)references, (size_t)nq * sizeof(double), false}};
    int ranges = 4;
    if (mode == MI_SCALE_GATE_NONE) {
        if (!u) return fail(MI_RAST_ERR_INVALID, "scale gate: null pointer");
        channels = 1, scale_aware_dim = 0, weight = bias = nullptr, gates = nullptr;
    } else {
        if (int rc = check_channels(channels)) return rc;
        if (!gates) return fail(MI_RAST_ERR_INVALID, "scale gate: null pointer");
        r[ranges++] = {(const char*)gates, (size_t)n * channels * sizeof(float), true};
        if (mode == MI_SCALE_GATE_LEARNED) {
            if (!weight || !bias) return fail(MI_RAST_ERR_INVALID, "scale gate: null pointer");
            r[ranges++] = {(const char*)weight, (size_t)channels * sizeof(float), false};
            r[ranges++] = {(const char*)bias, (size_t)channels * sizeof(float), false};
        } else if (scale_aware_dim < 1 || scale_aware_dim >= channels)
            return fail(MI_RAST_ERR_INVALID, "scale gate: need 1 <= scale_aware_dim < channels");
    }
    if (outputs_overlap(r, ranges)) return fail(MI_RAST_ERR_INVALID, "scale gate: an output overlaps another tensor of the call");
    const dim3 grid((unsigned)((n + SG_THREADS - 1) / SG_THREADS));
    if (n <= SG_DIRECT_MAX)
        hipLaunchKernelGGL(scale_gate_forward_kernel<false>, grid, dim3(SG_THREADS), 0, stream, n, scales, nq, quantiles, references, mode, channels,
                           weight, bias, scale_aware_dim, u, gates);
    else
        hipLaunchKernelGGL(scale_gate_forward_kernel<true>, grid, dim3(SG_THREADS), 0, stream, n, scales, nq, quantiles, references, mode, channels,
                           weight, bias, scale_aware_dim, u, gates);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_scale_gate_backward(int n, int channels, const float* u, const float* weight, const float* bias, const float* d_gates, float* d_weight,
                           float* d_bias, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_sizes(n, 1)) return rc;
    if (int rc = check_channels(channels)) return rc;
    if (!u || !weight || !bias || !d_gates || !d_weight || !d_bias) return fail(MI_RAST_ERR_INVALID, "scale gate: null pointer");
    const size_t row = (size_t)channels * sizeof(float);
    const Range r[6] = {{(const char*)d_weight, row, true}, {(const char*)d_bias, row, true}, {(const char*)u, (size_t)n * sizeof(float), false},
                        {(const char*)weight, row, false}, {(const char*)bias, row, false}, {(const char*)d_gates, (size_t)n * row, false}};
    if (outputs_overlap(r, 6)) return fail(MI_RAST_ERR_INVALID, "scale gate: an output overlaps another tensor of the call");
    hipLaunchKernelGGL(scale_gate_backward_kernel, dim3((unsigned)channels), dim3(SG_THREADS), 0, stream, n, channels, u, weight, bias, d_gates,
                       d_weight, d_bias);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
