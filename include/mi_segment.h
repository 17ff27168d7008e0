/* mi_segment.h -- C-ABI of the scale-gated segmentation queries (csrc/mi_segment.hip), in libmi_rast.so.
 *
 * What a user does with trained affinity features: gate and normalise every feature row, compare it with a few query features or
 * with cluster centres, threshold or take the arg-max (saga_gui.py:590-599, 633-659, 673-679, 524-543; prompt_segmenting.ipynb).
 * One definition for the three operations.  For a feature row f in R^C, optional gates g in R^C and a row normalisation `pre`:
 *
 *     u = f                          MI_SEGMENT_PRE_NONE   (saga_gui.py:674)
 *     u = f / max(|f|, 1e-12)        MI_SEGMENT_PRE_L2     (F.normalize; cluster_in_3D :526)
 *     u = f / (|f| + 1e-6)           MI_SEGMENT_PRE_EPS    (the GUI's image path, :592)
 *     v = u * g                      (v = u when gates is NULL)
 *     w = v / max(|v|, 1e-12)        F.normalize (:528, :599, :675); w = v with post == 0 (the PCA image, :593)
 *     s_k = <w, q_k>                 q_k as given, never normalised here
 *
 * The kernels form a = u / f (a scalar per row), |f * g| and <f * g, q_k> in one pass over the row and combine them at its end:
 * s_k = <f * g, q_k> * a / max(a |f * g|, 1e-12), the same value in exact arithmetic.  A zero row gives s_k = 0.  Inputs must be
 * finite and the sums of squares of a row must neither overflow nor underflow binary32 (|f| = 0 or 1e-18 < |f| < 1e18);
 * non-finite inputs are outside the contract.
 *
 * Layouts: MI_SEGMENT_IMAGE -- features [C][N] (a (C, H, W) render, N = H W); MI_SEGMENT_POINTS -- features [N][C].
 * 1 <= C <= 256, 1 <= N < 2^31; offsets inside the kernels are 64-bit.  queries / centers are [Q][C] / [K][C], gates [C] or NULL.
 * All pointers are device pointers, contiguous and 4-byte aligned (16-byte aligned features take the wide loads); outputs must
 * not overlap inputs; `stream` is a hipStream_t.  No atomics, no workspace, nothing allocated; the functions are re-entrant and
 * their results bit-identical from run to run.  Returns 0 or an MI_RAST_ERR_* code (mi_rast_last_error() holds the text).
 *
 * scores : scores [Q][N] f32, 1 <= Q <= 16.  One launch.  Algorithmic bytes: 4 N C read + 4 N Q written
 *          (265 MB + 8 MB at 1080p, C = 32, Q = 1).
 * select : t_k = (s_k + 1) / 2 with half_shift, else s_k; b_k = t_k > threshold; mask[n] = any_k b_k (one byte, 0 / 1) and
 *          score[n] = max_k (b_k ? t_k : 0), post-normalised (post = 1), 1 <= Q <= 16.  One launch, (Q, N) is never written.
 *          Algorithmic bytes: 4 N C read + 5 N written.
 * assign : label[n] = the lowest k with s_k = max_k s_k (int32), best[n] = that maximum, post-normalised, 1 <= K <= 4096.  One
 *          launch, (N, K) is never formed.  K <= 16 runs the kernel of scores / select (the same row arithmetic, so the labels are
 *          the arg-max of scores' output bit for bit); larger K runs on the f32 matrix pipe with the centres staged through LDS
 *          in blocks of mi_segment_assign_block(C) centres: 2 N K C flops.  Algorithmic bytes: 4 N C read + 8 N written (the
 *          centres, 4 K C, are re-read from L2 by every workgroup).
 */
#ifndef MI_SEGMENT_H
#define MI_SEGMENT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SEGMENT_IMAGE 0
#define MI_SEGMENT_POINTS 1

#define MI_SEGMENT_PRE_NONE 0
#define MI_SEGMENT_PRE_L2 1
#define MI_SEGMENT_PRE_EPS 2

#define MI_SEGMENT_MAX_CHANNELS 256
#define MI_SEGMENT_MAX_QUERIES 16
#define MI_SEGMENT_MAX_CENTERS 4096

int mi_segment_scores(int layout, int N, int C, int Q, const float* features, const float* queries /* [Q,C] */,
                      const float* gates /* [C] or NULL */, int pre, int post, float* scores /* [Q,N] */, void* stream);

int mi_segment_select(int layout, int N, int C, int Q, const float* features, const float* queries /* [Q,C] */,
                      const float* gates /* [C] or NULL */, int pre, int half_shift, float threshold, unsigned char* mask /* [N] */,
                      float* score /* [N] */, void* stream);

int mi_segment_assign(int layout, int N, int C, int K, const float* features, const float* centers /* [K,C] */,
                      const float* gates /* [C] or NULL */, int pre, int* labels /* [N] */, float* best /* [N] */, void* stream);

/* centres per LDS block of the K > 16 path of mi_segment_assign at C channels (a multiple of 32); 0 for C out of range */
int mi_segment_assign_block(int C);

#ifdef __cplusplus
}
#endif
#endif
