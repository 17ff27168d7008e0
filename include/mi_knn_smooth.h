/* mi_knn_smooth.h -- C-ABI of the fused KNN feature smoothing, in libmi_rast.so.
 *
 * Replaces the PyTorch expression of FeatureGaussianModel.get_smoothed_point_features
 * (scene/gaussian_model_ff.py:338-364: normalize -> gather selected neighbour columns -> mean) fused with the
 * renderer's re-normalisation of its result (gaussian_renderer/__init__.py:362-363), and its autograd backward.
 * All pointers are device pointers (fp32 / int32), row-major; `stream` is a hipStream_t.  C must be 32 or 64,
 * K <= 32.  sel_mask: bit s set <=> neighbour column s takes part (the reference draws int(K*dropout) columns with
 * torch.randperm; all K columns when dropout is outside (0, 1)).  Returns 0 or an MI_RAST_ERR_* code
 * (mi_rast_last_error() holds the text). */
#ifndef MI_KNN_SMOOTH_H
#define MI_KNN_SMOOTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int mi_knn_smooth_forward(int P, int C, int K, const int* knn_idx /* [P,K] */, uint32_t sel_mask,
                          const float* features /* [P,C] */, float* out /* [P,C] */, int normalize_out, void* stream);

/* inv_offsets[P+1] / inv_entries[P*K]: the inverse neighbour lists -- entries (i << 5 | column) with
 * knn_idx[i][column] == j, grouped by j -- built once per neighbour map by the caller.
 * dmean: scratch [P,C].  dL_dfeatures is overwritten (not accumulated). */
int mi_knn_smooth_backward(int P, int C, int K, const int* knn_idx, const int* inv_offsets,
                           const uint32_t* inv_entries, uint32_t sel_mask, const float* features,
                           const float* dL_dout, float* dmean, float* dL_dfeatures, int normalize_out, void* stream);

/* Multi-resolution smoothing with per-Gaussian level weights: FeatureGaussianModel.get_multi_resolution_smoothed_point_features
 * (scene/gaussian_model_ff.py:366-400) fused with the same re-normalisation, and its backward for features AND weights:
 *     mean_l[i] = (1/k_l) * sum over level l's columns s of  n[knn_idx[i][s]],   n[j] = F[j] / max(|F[j]|, 1e-12)
 *     ret[i]    = sum_l weights[i][l] * mean_l[i];   out[i] = normalize_out ? ret[i] / (|ret[i]| + 1e-9) : ret[i]
 * knn_idx [P, Ktot] holds GLOBAL indices, the L levels' maps side by side: level l owns level_k[l] columns, Ktot = sum of
 * level_k (the reference's per-level maps index into the subset xyz[point_mask]; the caller composes them with the subset's
 * members once per map).  1 <= L <= 4, every level_k[l] >= 1 (a host array, read during the call), Ktot <= 32, C 32 or 64,
 * P < 2^27.  weights: [P, L]; one row [1, L] shared by all Gaussians when weights_broadcast != 0; NULL = all ones. */
int mi_knn_smooth_multi_forward(int P, int C, int L, const int* level_k /* host [L] */, const int* knn_idx /* [P,Ktot] */,
                                const float* weights, int weights_broadcast, const float* features /* [P,C] */,
                                float* out /* [P,C] */, int normalize_out, void* stream);

/* inv_offsets[P+1] / inv_entries[P*Ktot]: the inverse lists of knn_idx, as for mi_knn_smooth_backward; a list may be of any
 * length (a level whose subset has k_l members puts all P rows into k_l lists) and is summed in its stored order, with a compensated sum.
 * dret: scratch [P,C].  dL_dfeatures is overwritten (not accumulated).  dL_dweights: [P, L] (ALSO when weights_broadcast: the
 * caller sums the rows), overwritten; NULL = not wanted. */
int mi_knn_smooth_multi_backward(int P, int C, int L, const int* level_k, const int* knn_idx, const int* inv_offsets,
                                 const uint32_t* inv_entries, const float* weights, int weights_broadcast,
                                 const float* features, const float* dL_dout, float* dret, float* dL_dfeatures,
                                 float* dL_dweights, int normalize_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
