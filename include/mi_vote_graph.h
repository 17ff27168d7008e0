/* mi_vote_graph.h -- C-ABI of the language-segmentation vote graph, in libmi_rast.so.  Error codes and mi_rast_last_error() are those
 * of mi_rast.h; the channel limit is mi_segment.h's MI_SEGMENT_MAX_CHANNELS, the bit rows are mi_cluster.h's.
 */
#ifndef MI_VOTE_GRAPH_H
#define MI_VOTE_GRAPH_H

#include <stddef.h>

#include "mi_cluster.h"
#include "mi_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Language-segmentation vote graph (csrc/mi_vote_graph.hip) --------------------------------------------
 *
 * The notebook's "Language-driven Segmentation" between the feature render and the Jaccard clustering above, and the CLIP relevancy
 * that scores its clusters.  g_m in R^C are the scale gates of mask m, f_p the bilinear sample (align_corners=False, no
 * antialiasing) of the (C, H, W) render at working pixel p of (h, w), a_a a raw anchor feature.
 *
 * mask_features : eroded [M][h][ceil(w/64)] are the masks at the working resolution (mi_mask_erode_min_sum, mi_mask_scales.h), n_m
 *                 their pixel counts.  s_m = sum_{p in m} (g_m * f_p) / max(|g_m * f_p|, 1e-12) / (n_m + 1e-9);
 *                 features[m] = s_m / max(|s_m|, 1e-12), counts[m] = n_m (may be NULL).  Evaluated as g_m * sum_p f_p w_mp with the
 *                 scalar w_mp = 1 / max(|g_m * f_p|, 1e-12): f_p is rounded once to f32 from an f64 interpolation, everything
 *                 after it is f64 until the final rounding.  Three launches, no atomics: per-tile (16 rows x 64 pixels) partials in
 *                 the workspace, added in tile order -- the same inputs give the same bits.  Workspace: 4 C h w (the resampled
 *                 render) + 8 M T (C + 1), T = ceil(h/16) ceil(w/64).  No (M, C, h, w) or (M, h, w) float tensor exists.
 *                 Algorithmic bytes: 4 C H W + 8 M h ceil(w/64) read, 4 M C written.
 * anchor_bits   : v_ma = ((g_m * phi_m) . a_a) / max(sqrt(g_m^2 . a_a^2), 1e-12) in f32 (two multiply-accumulate chains on the exact
 *                 f32 matrix instruction, one root, one division); bit a of row m = v_ma > threshold, strict, false for NaN
 *                 (a non-finite anchor gives 0 bits in its column and touches no other).  bits [M][words] int32,
 *                 words = ceil(A/32), bit k of word j = anchor 32 j + k, bits past A zero (the MI_CLUSTER_JACCARD row layout);
 *                 counts[m] = the row's set bits (may be NULL: one launch instead of two).  (M, A) values are never stored.
 *                 Algorithmic bytes: 4 C (A + 2 M) read, 4 M words written.
 * relevancy     : out[n][p] = 1 / (1 + exp(10 (max_q e_n . neg_q - e_n . pos_p))) = min_q softmax(10 [e_n . pos_p, e_n . neg_q])[0];
 *                 e_n = row n of embeds (f32, or f16 with embeds_f16) converted to f32, divided by max(|row|, 1e-12) with normalize.
 *                 One launch, each row read once; sums in f64 in a fixed order.  Algorithmic bytes: (2 or 4) N D read, 4 N P written.
 *
 * All pointers are device pointers, contiguous; outputs must not overlap inputs; `stream` is a hipStream_t.  Nothing is allocated;
 * re-entrant; bit-identical from run to run.  Returns 0 or an MI_RAST_ERR_* code.
 */
#define MI_VOTE_MAX_ANCHORS 32768   /* 32 MI_CLUSTER_MAX_WORDS */
#define MI_VOTE_MAX_EMBED_DIM 1024
#define MI_VOTE_MAX_PROMPTS 16

/* 0 for arguments out of range */
size_t mi_vote_mask_features_workspace_bytes(int M, int C, int h, int w);

int mi_vote_mask_features(int M, int C, int H, int W, const float* rendered /* [C,H,W] */, int h, int w,
                          const unsigned long long* eroded /* [M,h,ceil(w/64)] */, const float* gates /* [M,C] */, void* workspace,
                          size_t workspace_bytes, float* features /* [M,C] */, long long* counts /* [M] or NULL */, void* stream);

int mi_vote_anchor_bits(int M, int A, int C, const float* mask_features /* [M,C] */, const float* gates /* [M,C] */,
                        const float* anchors /* [A,C] */, float threshold, int* bits /* [M,ceil(A/32)] */, int* counts /* [M] or NULL */,
                        void* stream);

int mi_vote_relevancy(int N, int D, int P, int Q, const void* embeds /* [N,D] */, int embeds_f16, const float* pos /* [P,D] */,
                      const float* neg /* [Q,D] */, int normalize, float* out /* [N,P] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
