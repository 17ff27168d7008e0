/* mi_scale_gate.h -- C-ABI of scale conditioning, in libmi_rast.so.  Error codes and mi_rast_last_error() are those of mi_rast.h.
 */
#ifndef MI_SCALE_GATE_H
#define MI_SCALE_GATE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Scale conditioning: quantile transform and scale gates (csrc/mi_scale_gate.hip) ----
 *
 * The two steps every stage that takes a 3-D scale goes through (train_contrastive_feature.py:42-62, 228, 240-245): q_trans,
 * scikit-learn's QuantileTransformer with the uniform output, and scale_gate, Linear(1, C) + Sigmoid, or the fixed 1 / 0 gates.
 *
 * fit      : sorted [n] is the fit data in ascending order with the NaNs last; references [nq] is np.linspace(0, 1, nq).  Writes
 *            quantiles [nq] = np.maximum.accumulate(np.nanpercentile(data, references * 100)) as numpy computes it on float32
 *            data, bit for bit (all NaN when the data are).  One launch of one workgroup.
 * forward  : u[i] = the transformer's uniform output for scales[i], bit for bit (NaN for NaN; 1 and 0 at and beyond the ends of
 *            the table), and with a gate mode gates [n][channels] in the same launch:
 *              MI_SCALE_GATE_LEARNED  sigmoid(fl(fl(weight[c] * u) + bias[c])), accurate expf;
 *              MI_SCALE_GATE_FIXED    1 where c < channels - scale_aware_dim + trunc(fl(fl(1 - u) * scale_aware_dim)), else 0; a
 *                                     NaN row for a NaN scale.
 *            MI_SCALE_GATE_NONE writes u alone (channels, weight, bias, scale_aware_dim, gates are not looked at); with a gate
 *            mode u may be NULL.  weight and bias are read in the LEARNED mode only.  One launch.
 * backward : d_weight[c] = sum_i d_gates[i][c] * sigmoid'(z) * u[i] and d_bias[c] the same without u[i], z = weight[c] * u[i] +
 *            bias[c], evaluated and accumulated in binary64 in a fixed order: no atomics, the same bits every run.  One launch.
 *
 * 1 <= n < 2^30, 1 <= nq <= MI_SCALE_MAX_QUANTILES, 1 <= channels <= MI_SCALE_MAX_CHANNELS, 1 <= scale_aware_dim < channels.
 * Device pointers, contiguous, naturally aligned; outputs must not overlap anything else of the call; `stream` is a hipStream_t.
 * Nothing is allocated, copied to the host or waited for.  Returns 0 or an MI_RAST_ERR_* code.
 */
#define MI_SCALE_MAX_QUANTILES 1024
#define MI_SCALE_MAX_CHANNELS 256

enum { MI_SCALE_GATE_NONE = 0, MI_SCALE_GATE_LEARNED, MI_SCALE_GATE_FIXED };

int mi_scale_quantile_fit(int n, const float* sorted /* [n] */, int nq, const double* references /* [nq] */,
                          double* quantiles /* [nq] */, void* stream);

int mi_scale_gate_forward(int n, const float* scales /* [n] */, int nq, const double* quantiles, const double* references,
                          int mode, int channels, const float* weight /* [channels] */, const float* bias /* [channels] */,
                          int scale_aware_dim, float* u /* [n] or NULL */, float* gates /* [n][channels] */, void* stream);

int mi_scale_gate_backward(int n, int channels, const float* u /* [n] */, const float* weight, const float* bias,
                           const float* d_gates /* [n][channels] */, float* d_weight /* [channels] */, float* d_bias /* [channels] */,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
