/* mi_segment.h -- C-ABI of the scale-gated segmentation queries, in libmi_rast.so.
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

/* ---- Clustering: exact HDBSCAN* (csrc/mi_cluster.hip) ----------------------------------------------------
 *
 * Where the centres of `assign` come from (saga_gui.py:518-543, the notebook's "Cluster in 3D / 2D" and its Jaccard cell).  Core
 * distances and the minimum spanning tree of the mutual-reachability graph run on the device, the tree work on the host.
 *
 * Pair distance of rows i, j:
 *   MI_CLUSTER_EUCLIDEAN  rows f32 [n][C], 1 <= C <= 256: d = sqrt(sum_c (x_ic - x_jc)^2) in binary32, summed in channel order
 *                         (difference form, one fused multiply-add per channel, a correctly rounded root).  d(i,j) and d(j,i) are the
 *                         same bits, d(i,i) = 0.
 *   MI_CLUSTER_JACCARD    rows uint32 [n][Wd], 1 <= Wd <= 1024, packed bit sets, bits past the logical width zero:
 *                         I = popcount(a & b) as an integer, d = float32(1 - I / (|a| + |b| - I + 1e-6)) evaluated in binary64 and
 *                         rounded once.
 * core_i   = the core_k-th smallest of d(i,j) over ALL j, j = i included (scikit-learn's min_samples; a caller who wants "self not
 *            counted" passes min_samples + 1).  1 <= core_k <= min(n, MI_CLUSTER_MAX_CORE_K).
 * w(i,j)   = max(core_i, core_j, d(i,j)), i != j.
 * the tree = a minimum spanning tree of the complete graph under w: n - 1 edges (a, b, w) with a < b; n = 1 gives none.  Boruvka
 *            rounds under the strict total order (w, min(i,j), max(i,j)) on undirected edges, which every row and every component
 *            uses alike; integer atomicMin keys only.  One 4-byte host read per round (the stream is synchronised there), about
 *            log2(n) rounds at most.
 * labels   = single-linkage tree over the edges sorted by (w, a, b), condensed with min_cluster_size, excess-of-mass selection,
 *            cluster_selection_epsilon (a selected cluster born below epsilon gives way to its lowest ancestor born above it; of two
 *            selected clusters one above the other the upper one stays), allow_single_cluster; noise is -1, clusters are numbered
 *            0 .. K-1 by ascending smallest member.  n < min_cluster_size gives all -1.
 *
 * rows, core, edge_*, workspace are device pointers (rows 4-byte, the workspace 8-byte aligned); the labels call takes HOST pointers
 * and makes no HIP call.  Nothing is allocated; the workspace (one size for both device calls, linear in n: no n x n buffer exists
 * in any path) is scratch and carries nothing from call to call.  Re-entrant; results are bit-identical from run to run, the order
 * of the edges included.  Non-finite inputs are outside the contract.  Returns 0 or an MI_RAST_ERR_* code.
 */
#define MI_CLUSTER_EUCLIDEAN 0
#define MI_CLUSTER_JACCARD 1
#define MI_CLUSTER_MAX_POINTS (1 << 20)
#define MI_CLUSTER_MAX_CHANNELS 256
#define MI_CLUSTER_MAX_WORDS 1024
#define MI_CLUSTER_MAX_CORE_K 64

/* bytes of workspace for both device calls; 0 for arguments out of range */
size_t mi_cluster_workspace_bytes(int metric, int n, int width, int core_k);

int mi_cluster_core_distances(int metric, int n, int width, const void* rows, int core_k, float* core /* [n] */, void* workspace,
                              size_t workspace_bytes, void* stream);

int mi_cluster_mst(int metric, int n, int width, const void* rows, const float* core /* [n] */, int* edge_a /* [n-1] */,
                   int* edge_b /* [n-1] */, float* edge_w /* [n-1] */, void* workspace, size_t workspace_bytes, void* stream);

/* Boruvka rounds of the calling thread's last successful tree call */
int mi_cluster_mst_rounds(void);

/* host pointers; refuses what is not a spanning tree of n points (n_edges != n - 1, an index out of range, a cycle) */
int mi_cluster_labels_host(int n, int n_edges, const int* edge_a, const int* edge_b, const float* edge_w, int min_cluster_size,
                           double epsilon, int allow_single_cluster, int* labels /* [n] */, int* n_clusters);

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

/* ---- The viewer frame (csrc/mi_viewer.hip) ----------------------------------------------------------------
 *
 * What the GUI shows (saga_gui.py:547-569, 590-599, 645-659, 701-724): the PCA basis of the features and the display buffer of a
 * frame.  u = f / (|f| + 1e-6) and the gated, normalised w of the segmentation section above (MI_SEGMENT_PRE_EPS, post = 1).
 *
 * moments : the n rows index[0 .. n) of the features (index NULL: rows 0 .. n, n <= N), normalised by `pre`:
 *           mean = sum u / n, cov = sum u u^T / n - mean mean^T (the 1/n form of :551), both binary64, cov [C][C] symmetric bit for
 *           bit.  The Gram matrix runs on the exact f32 matrix instruction in chains of mi_view_moments_block() rows; each chain
 *           is then added into binary64 sums kept per workgroup, sum u is added in binary64 directly, and a second launch adds the
 *           workgroups' partial sums in a fixed order.  No atomics: the same inputs give the same bits.  Two launches.
 *           index holds int64 row numbers in [0, N), repeats allowed; the CALLER guarantees the range (the kernels do not check
 *           it).  1 <= n < 2^31.  Workspace: mi_view_moments_workspace_bytes(n, C) bytes, 8-byte aligned, scratch.
 *           Algorithmic bytes: 4 n C read (once for C <= 64; ceil(C / 32) (ceil(C / 32) + 1) / 24 times above, rounded up).
 * frame   : one launch over a (C, H, W) feature render, N = H W, features [C][N], rgb and cluster_rgb [3][N]:
 *             t_k = (<w, q_k> + 1) / 2, b_k = t_k > threshold, any = or_k b_k, score = max_k (b_k ? t_k : 0)  -- bit for bit
 *                   what the select call above gives with MI_SEGMENT_PRE_EPS and half_shift (the same inline row arithmetic);
 *             p_j = <u, proj[:, j]>, j < 3 (the ungated chain of the scores call with post = 0);
 *             rgb_score = rgb * any when preview is set and Q > 0, else rgb;
 *             frame[n][:] = (the enabled components, added in this order) / their count, in binary32:
 *               MI_VIEW_RGB         rgb_score
 *               MI_VIEW_PCA         min(max(p * 0.5 + 0.5, 0), 1)
 *               MI_VIEW_CLUSTER     cluster_rgb, or rgb_score when it is NULL
 *               MI_VIEW_SIMILARITY  jet(score), or rgb_score when Q = 0; jet is the 9-knot piecewise-linear map of :272-292 on
 *                                   the positions k / 8, constant outside [0, 1]
 *           modes is a non-empty OR of the four bits.  Q = 0 (queries NULL): mask and score are not written and may be NULL.
 *           proj [C][3] is required with MI_VIEW_PCA.  frame [N][3] interleaved; mask [N] one byte, 0 / 1; score [N].  The features
 *           are read once (not at all when neither MI_VIEW_PCA nor queries ask for them; rgb only where a component shows it).
 *           No workspace.  Algorithmic bytes: 4 N (C + 3 or 6) read, 12 N written, + 5 N with queries.
 *
 * Device pointers, contiguous, 4-byte aligned unless stated; outputs must not overlap inputs; `stream` is a hipStream_t.  Nothing
 * is allocated; re-entrant; bit-identical from run to run.  Returns 0 or an MI_RAST_ERR_* code.
 */
#define MI_VIEW_RGB 1
#define MI_VIEW_PCA 2
#define MI_VIEW_CLUSTER 4
#define MI_VIEW_SIMILARITY 8

/* 0 for arguments out of range */
size_t mi_view_moments_workspace_bytes(int n, int C);

/* rows per f32 accumulator chain of the Gram matrix */
int mi_view_moments_block(void);

int mi_view_moments(int layout, int N, int C, const float* features, const long long* index /* [n] or NULL */, int n, int pre,
                    void* workspace, size_t workspace_bytes, double* mean /* [C] */, double* cov /* [C,C] */, void* stream);

int mi_view_frame(int N, int C, const float* features /* [C,N] */, const float* rgb /* [3,N] */,
                  const float* cluster_rgb /* [3,N] or NULL */, const float* proj /* [C,3] or NULL */, int Q,
                  const float* queries /* [Q,C] or NULL */, const float* gates /* [C] or NULL */, float threshold, int modes,
                  int preview, float* frame /* [N,3] */, unsigned char* mask /* [N] or NULL */, float* score /* [N] or NULL */,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
