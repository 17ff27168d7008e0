/* mi_cluster.h -- C-ABI of the clustering, in libmi_rast.so.  Error codes and mi_rast_last_error() are those of mi_rast.h; `assign`
 * below is mi_segment.h's mi_segment_assign.
 */
#ifndef MI_CLUSTER_H
#define MI_CLUSTER_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif
