/* mi_viewer.h -- C-ABI of the viewer frame, in libmi_rast.so.  Error codes and mi_rast_last_error() are those of mi_rast.h; the row
 * arithmetic (u, w, `pre`, the layouts, the select call) and its constants are mi_segment.h's.
 */
#ifndef MI_VIEWER_H
#define MI_VIEWER_H

#include <stddef.h>

#include "mi_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

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
