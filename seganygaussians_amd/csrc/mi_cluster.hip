// mi_cluster.hip -- C-ABI implementation of include/mi_cluster.h.
#include "host.h"
#include "../../include/mi_cluster.h"

#include "cluster.h"        // HDBSCAN* on the device: core distances, Boruvka rounds
#include "cluster_tree.h"   // its host half: from the spanning tree to labels

using namespace mirast;

namespace {

thread_local int g_last_rounds = 0;

struct ClusterLayout {
    size_t cnt, comp, parent, row_w, row_j, comp_w, comp_pair, tmp_a, tmp_b, tmp_w, merged, total;
};

// 11 arrays of n words (comp_pair has two) and one counter, each on a 256-byte boundary: total <= 44 n + 12 * 256
ClusterLayout cluster_layout(int n)
{
    ClusterLayout l;
    Carver c;
    const size_t words = (size_t)n * 4;
    l.cnt = c.take(words);
    l.comp = c.take(words);
    l.parent = c.take(words);
    l.row_w = c.take(words);
    l.row_j = c.take(words);
    l.comp_w = c.take(words);
    l.comp_pair = c.take(2 * words);
    l.tmp_a = c.take(words);
    l.tmp_b = c.take(words);
    l.tmp_w = c.take(words);
    l.merged = c.take(sizeof(int));
    l.total = c.off;
    return l;
}

bool shape_ok(int metric, int n, int width)
{
    if (metric != MI_CLUSTER_EUCLIDEAN && metric != MI_CLUSTER_JACCARD) return false;
    if (n < 1 || n > MI_CLUSTER_MAX_POINTS || width < 1) return false;
    return width <= (metric == MI_CLUSTER_EUCLIDEAN ? MI_CLUSTER_MAX_CHANNELS : MI_CLUSTER_MAX_WORDS);
}

int cluster_check(int metric, int n, int width, const void* rows, const void* workspace, size_t workspace_bytes)
{
    if (metric != MI_CLUSTER_EUCLIDEAN && metric != MI_CLUSTER_JACCARD)
        return fail(MI_RAST_ERR_INVALID, "cluster: metric must be MI_CLUSTER_EUCLIDEAN or MI_CLUSTER_JACCARD");
    if (!shape_ok(metric, n, width))
        return fail(MI_RAST_ERR_INVALID, "cluster: need 1 <= n <= 2^20 rows and a width of 1..256 channels (euclidean) or 1..1024 words (jaccard)");
    if (!rows || !workspace) return fail(MI_RAST_ERR_INVALID, "cluster: null pointer");
    if ((uintptr_t)rows % 4 || (uintptr_t)workspace % 8) return fail(MI_RAST_ERR_INVALID, "cluster: rows must be 4-byte and the workspace 8-byte aligned");
    if (workspace_bytes < cluster_layout(n).total) return fail(MI_RAST_ERR_INVALID, "cluster: workspace smaller than the workspace-bytes query says");
    return MI_RAST_OK;
}

dim3 flat_grid(int n) { return dim3((unsigned)((n + CL_THREADS - 1) / CL_THREADS)); }
dim3 pair_grid(int n) { return dim3((unsigned)((n + CL_ROWS - 1) / CL_ROWS)); }

template <class M, int CH>
void launch_core(const ClArgs& a, hipStream_t stream)
{
    if (a.core_k <= 16) hipLaunchKernelGGL((cl_core_kernel<M, CH, 16>), pair_grid(a.n), dim3(CL_THREADS), 0, stream, a);
    else if (a.core_k <= 32) hipLaunchKernelGGL((cl_core_kernel<M, CH, 32>), pair_grid(a.n), dim3(CL_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((cl_core_kernel<M, CH, CL_MAX_K>), pair_grid(a.n), dim3(CL_THREADS), 0, stream, a);
}

void launch_row_min(int metric, const ClArgs& a, hipStream_t stream)
{
    if (metric == MI_CLUSTER_JACCARD) hipLaunchKernelGGL((cl_row_min_kernel<ClJaccard, 32>), pair_grid(a.n), dim3(CL_THREADS), 0, stream, a);
    else if (a.width <= 32) hipLaunchKernelGGL((cl_row_min_kernel<ClEuclid, 32>), pair_grid(a.n), dim3(CL_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((cl_row_min_kernel<ClEuclid, 64>), pair_grid(a.n), dim3(CL_THREADS), 0, stream, a);
}

}  // namespace

extern "C" {

size_t mi_cluster_workspace_bytes(int metric, int n, int width, int core_k)
{
    if (!shape_ok(metric, n, width) || core_k < 1 || core_k > MI_CLUSTER_MAX_CORE_K || core_k > n) return 0;
    return cluster_layout(n).total;
}

int mi_cluster_core_distances(int metric, int n, int width, const void* rows, int core_k, float* core, void* workspace,
                              size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = cluster_check(metric, n, width, rows, workspace, workspace_bytes)) return rc;
    if (core_k < 1 || core_k > MI_CLUSTER_MAX_CORE_K || core_k > n) return fail(MI_RAST_ERR_INVALID, "cluster: need 1 <= core_k <= min(n, 64)");
    if (!core) return fail(MI_RAST_ERR_INVALID, "cluster: null output");
    const ClusterLayout l = cluster_layout(n);
    char* ws = (char*)workspace;
    ClArgs a{};
    a.rows = (const uint32_t*)rows;
    a.n = n;
    a.width = width;
    a.cnt = (const int*)(ws + l.cnt);
    a.core_k = core_k;
    a.core_out = core;
    if (metric == MI_CLUSTER_JACCARD) {
        hipLaunchKernelGGL(cl_popcount_kernel, flat_grid(n), dim3(CL_THREADS), 0, stream, a.rows, n, width, (int*)(ws + l.cnt));
        launch_core<ClJaccard, 32>(a, stream);
    } else if (width <= 32) {
        launch_core<ClEuclid, 32>(a, stream);
    } else {
        launch_core<ClEuclid, 64>(a, stream);
    }
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_cluster_mst(int metric, int n, int width, const void* rows, const float* core, int* edge_a, int* edge_b, float* edge_w,
                   void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = cluster_check(metric, n, width, rows, workspace, workspace_bytes)) return rc;
    if (!core) return fail(MI_RAST_ERR_INVALID, "cluster: null pointer");
    if (n > 1 && (!edge_a || !edge_b || !edge_w)) return fail(MI_RAST_ERR_INVALID, "cluster: null output");
    g_last_rounds = 0;
    if (n == 1) return MI_RAST_OK;
    const ClusterLayout l = cluster_layout(n);
    char* ws = (char*)workspace;
    int* comp = (int*)(ws + l.comp);
    int* parent = (int*)(ws + l.parent);
    unsigned long long* comp_pair = (unsigned long long*)(ws + l.comp_pair);
    int *tmp_a = (int*)(ws + l.tmp_a), *tmp_b = (int*)(ws + l.tmp_b), *merged = (int*)(ws + l.merged);
    float* tmp_w = (float*)(ws + l.tmp_w);
    ClArgs a{};
    a.rows = (const uint32_t*)rows;
    a.n = n;
    a.width = width;
    a.cnt = (const int*)(ws + l.cnt);
    a.core = core;
    a.comp = comp;
    a.row_w = (unsigned*)(ws + l.row_w);
    a.row_j = (int*)(ws + l.row_j);
    a.comp_w = (unsigned*)(ws + l.comp_w);
    const dim3 grid = flat_grid(n), block(CL_THREADS);
    if (metric == MI_CLUSTER_JACCARD) hipLaunchKernelGGL(cl_popcount_kernel, grid, block, 0, stream, a.rows, n, width, (int*)(ws + l.cnt));
    hipLaunchKernelGGL(cl_components_init_kernel, grid, block, 0, stream, n, comp, parent);
    int components = n, rounds = 0;
    while (components > 1) {
        hipLaunchKernelGGL(cl_round_init_kernel, grid, block, 0, stream, n, a.comp_w, comp_pair, merged);
        launch_row_min(metric, a, stream);
        hipLaunchKernelGGL(cl_pair_min_kernel, grid, block, 0, stream, n, comp, a.row_w, a.row_j, a.comp_w, comp_pair);
        hipLaunchKernelGGL(cl_hook_kernel, grid, block, 0, stream, n, comp, a.comp_w, comp_pair, parent, tmp_a, tmp_b, tmp_w, merged);
        for (int reach = 1; reach < components; reach *= 2)   // a chain of hooks is shorter than the number of components
            hipLaunchKernelGGL(cl_jump_kernel, grid, block, 0, stream, n, parent);
        hipLaunchKernelGGL(cl_relabel_kernel, grid, block, 0, stream, n, comp, parent);
        HIP_TRY(hipGetLastError());
        int merged_host = 0;   // the one host read of a round
        HIP_TRY(hipMemcpyAsync(&merged_host, merged, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        rounds++;
        // every component of a complete graph has an outgoing edge, and at most half of them stay roots
        if (merged_host < (components + 1) / 2 || merged_host >= components)
            return fail(MI_RAST_ERR_HIP, "cluster: a Boruvka round merged an impossible number of components (non-finite input?)");
        components -= merged_host;
    }
    hipLaunchKernelGGL(cl_emit_kernel, grid, block, 0, stream, n, comp, tmp_a, tmp_b, tmp_w, edge_a, edge_b, edge_w);
    HIP_TRY(hipGetLastError());
    g_last_rounds = rounds;
    return MI_RAST_OK;
}

int mi_cluster_mst_rounds(void) { return g_last_rounds; }

int mi_cluster_labels_host(int n, int n_edges, const int* edge_a, const int* edge_b, const float* edge_w, int min_cluster_size,
                           double epsilon, int allow_single_cluster, int* labels, int* n_clusters)
{
    if (n < 1 || n > MI_CLUSTER_MAX_POINTS) return fail(MI_RAST_ERR_INVALID, "cluster: need 1 <= n <= 2^20 points");
    if (min_cluster_size < 2) return fail(MI_RAST_ERR_INVALID, "cluster: need min_cluster_size >= 2");
    if (!(epsilon >= 0.0)) return fail(MI_RAST_ERR_INVALID, "cluster: need cluster_selection_epsilon >= 0");
    if (!labels || !n_clusters || (n_edges > 0 && (!edge_a || !edge_b || !edge_w))) return fail(MI_RAST_ERR_INVALID, "cluster: null pointer");
    switch (cluster_labels_from_mst(n, n_edges, edge_a, edge_b, edge_w, min_cluster_size, epsilon, allow_single_cluster != 0, labels, n_clusters)) {
        case CL_TREE_OK: return MI_RAST_OK;
        case CL_TREE_BAD_COUNT: return fail(MI_RAST_ERR_INVALID, "cluster: a spanning tree of n points has n - 1 edges");
        case CL_TREE_BAD_INDEX: return fail(MI_RAST_ERR_INVALID, "cluster: edge index out of range");
        case CL_TREE_BAD_WEIGHT: return fail(MI_RAST_ERR_INVALID, "cluster: edge weights must be finite and >= 0");
        default: return fail(MI_RAST_ERR_INVALID, "cluster: the edges contain a cycle");
    }
}

}  // extern "C"
