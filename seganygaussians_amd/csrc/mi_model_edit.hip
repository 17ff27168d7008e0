// mi_model_edit.hip -- C-ABI implementation of include/mi_model_edit.h, the model cut.
#include "host.h"
#include "../../include/mi_model_edit.h"

#include "model_edit.h"   // current rows, selection, the row map; the scan and the gather are row_compact.h's

using namespace mirast;

namespace {

constexpr int ME_MAX_P = (1 << 30) - 1;     // as densify: row numbers and 2 P stay ints
constexpr int ME_MAX_TIMES = 1 << 24;       // segment_times + 1 must be exact in binary32

struct EditLayout {
    size_t flags, current_counts, current_offsets, selected_counts, selected_offsets, totals, src_of, total;
    int nblocks;
};

EditLayout edit_layout(int P0)
{
    EditLayout l;
    Carver c;
    l.nblocks = (P0 + RC_THREADS - 1) / RC_THREADS;
    l.flags = c.take((size_t)P0);
    l.current_counts = c.take((size_t)l.nblocks * sizeof(int));
    l.current_offsets = c.take((size_t)l.nblocks * sizeof(int));
    l.selected_counts = c.take((size_t)l.nblocks * sizeof(int));
    l.selected_offsets = c.take((size_t)l.nblocks * sizeof(int));
    l.totals = c.take(MT_N * sizeof(int));
    l.src_of = c.take((size_t)P0 * sizeof(int));
    l.total = c.off;
    return l;
}

int edit_check_ws(int P0, const void* workspace, size_t workspace_bytes)
{
    if (P0 < 1 || P0 > ME_MAX_P) return fail(MI_RAST_ERR_INVALID, "model edit: need 1 <= P0 < 2^30 rows");
    if (!workspace) return fail(MI_RAST_ERR_INVALID, "model edit: null pointer");
    if (workspace_bytes < edit_layout(P0).total) return fail(MI_RAST_ERR_INVALID, "model edit: workspace smaller than mi_edit_workspace_bytes(P0)");
    return MI_RAST_OK;
}

}  // namespace

extern "C" {

size_t mi_edit_workspace_bytes(int P0)
{
    if (P0 < 1 || P0 > ME_MAX_P) return 0;
    return edit_layout(P0).total;
}

int mi_edit_plan(int P0, const float* level, int segment_times, int n_rows, const unsigned char* mask, void* workspace, size_t workspace_bytes,
                 void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = edit_check_ws(P0, workspace, workspace_bytes)) return rc;
    if (!level || !mask) return fail(MI_RAST_ERR_INVALID, "model edit: null pointer");
    if (segment_times < 0 || segment_times >= ME_MAX_TIMES) return fail(MI_RAST_ERR_INVALID, "model edit: need 0 <= segment_times < 2^24");
    if (n_rows < 1 || n_rows > P0) return fail(MI_RAST_ERR_INVALID, "model edit: need 1 <= n_rows <= P0");
    const EditLayout l = edit_layout(P0);
    const Range r[3] = {{(const char*)workspace, l.total, true}, {(const char*)level, (size_t)P0 * sizeof(float), false},
                        {(const char*)mask, (size_t)n_rows, false}};
    if (outputs_overlap(r, 3)) return fail(MI_RAST_ERR_INVALID, "model edit: the workspace overlaps another tensor of the call");
    char* ws = (char*)workspace;
    int* totals = (int*)(ws + l.totals);
    const float current_level = (float)(segment_times + 1);
    hipLaunchKernelGGL(edit_current_kernel, dim3(l.nblocks), dim3(RC_THREADS), 0, stream, P0, level, current_level, (int*)(ws + l.current_counts));
    hipLaunchKernelGGL(block_scan_kernel<1>, dim3(1), dim3(RC_THREADS), 0, stream, l.nblocks, (const int*)(ws + l.current_counts),
                       (int*)(ws + l.current_offsets), totals + MT_CURRENT);
    hipLaunchKernelGGL(edit_select_kernel, dim3(l.nblocks), dim3(RC_THREADS), 0, stream, P0, level, current_level, n_rows, mask,
                       (const int*)(ws + l.current_offsets), (unsigned char*)(ws + l.flags), (int*)(ws + l.selected_counts));
    hipLaunchKernelGGL(block_scan_kernel<1>, dim3(1), dim3(RC_THREADS), 0, stream, l.nblocks, (const int*)(ws + l.selected_counts),
                       (int*)(ws + l.selected_offsets), totals + MT_SELECTED);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_edit_counts(int P0, const void* workspace, size_t workspace_bytes, int* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = edit_check_ws(P0, workspace, workspace_bytes)) return rc;
    if (!counts) return fail(MI_RAST_ERR_INVALID, "model edit: null pointer");
    static_assert(MT_CURRENT == MI_EDIT_CURRENT && MT_SELECTED == MI_EDIT_SELECTED && MI_EDIT_KEPT == MT_N && MI_EDIT_NCOUNTS == MT_N + 1, "counts");
    HIP_TRY(hipMemcpyAsync(counts, (const char*)workspace + edit_layout(P0).totals, MT_N * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    counts[MI_EDIT_KEPT] = edit_kept(counts[MI_EDIT_CURRENT], counts[MI_EDIT_SELECTED]);
    return MI_RAST_OK;
}

int mi_edit_apply(int P0, int n_rows, const int* counts, float* level, int n_tensors, const float* const* src, float* const* dst, const int* cols,
                  void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = edit_check_ws(P0, workspace, workspace_bytes)) return rc;
    if (!counts || !src || !dst || !cols) return fail(MI_RAST_ERR_INVALID, "model edit: null table");
    static_assert(RC_MAX_TENSORS == MI_EDIT_MAX_TENSORS, "tensors per call");
    if (n_tensors < 1 || n_tensors > RC_MAX_TENSORS) return fail(MI_RAST_ERR_INVALID, "model edit: need 1 <= n_tensors <= 32");
    if (n_rows < 1 || n_rows > P0) return fail(MI_RAST_ERR_INVALID, "model edit: need 1 <= n_rows <= P0");
    const int kept = counts[MI_EDIT_KEPT];
    if (counts[MI_EDIT_CURRENT] != n_rows || counts[MI_EDIT_SELECTED] < 0 || counts[MI_EDIT_SELECTED] > n_rows ||
        kept != edit_kept(counts[MI_EDIT_CURRENT], counts[MI_EDIT_SELECTED]))
        return fail(MI_RAST_ERR_INVALID, "model edit: counts are not those of a plan whose current rows are the n_rows of the tensors");
    const EditLayout l = edit_layout(P0);
    GatherTable T = {};
    Range r[2 * RC_MAX_TENSORS + 2];
    size_t longest = 0;
    int live = 0;
    for (int k = 0; k < n_tensors; k++) {
        if (cols[k] < 0 || cols[k] > MI_EDIT_MAX_COLS) return fail(MI_RAST_ERR_INVALID, "model edit: need 0 <= cols <= 4096");
        if (cols[k] == 0) continue;     // f_rest at SH degree 0: nothing to gather
        if (!src[k] || !dst[k]) return fail(MI_RAST_ERR_INVALID, "model edit: null pointer");
        T.t[live] = {src[k], dst[k], cols[k], 0};
        r[2 * live] = {(const char*)src[k], (size_t)n_rows * cols[k] * sizeof(float), false};
        r[2 * live + 1] = {(const char*)dst[k], (size_t)kept * cols[k] * sizeof(float), true};
        if ((size_t)kept * cols[k] > longest) longest = (size_t)kept * cols[k];
        live++;
    }
    r[2 * live] = {(const char*)workspace, l.total, true};
    r[2 * live + 1] = {(const char*)level, level ? (size_t)P0 * sizeof(float) : 0, true};
    if (outputs_overlap(r, 2 * live + 2)) return fail(MI_RAST_ERR_INVALID, "model edit: an output overlaps another tensor of the call");
    char* ws = (char*)workspace;
    int* src_of = (int*)(ws + l.src_of);
    hipLaunchKernelGGL(edit_map_kernel, dim3(l.nblocks), dim3(RC_THREADS), 0, stream, P0, (const unsigned char*)(ws + l.flags),
                       (const int*)(ws + l.current_offsets), (const int*)(ws + l.selected_offsets), (const int*)(ws + l.totals), kept, level, src_of);
    if (live > 0)
        hipLaunchKernelGGL(row_gather_kernel<false>, dim3(gather_grid_x(longest), (unsigned)live), dim3(RC_THREADS), 0, stream, T, n_rows, kept, kept,
                           (const int*)src_of);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
