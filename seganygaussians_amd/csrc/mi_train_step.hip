// mi_train_step.hip -- C-ABI implementation of include/mi_train_step.h.
#include "host.h"
#include "../../include/mi_train_step.h"

#include "train_step.h"   // Adam over all groups, densification statistics, densify and prune

#include <cmath>

using namespace mirast;

namespace {

constexpr int DN_MAX_P = (1 << 30) - 1;   // src_of has 2 P int32 entries, and 2 P rows must be an int

struct DensifyLayout {
    size_t flags, block_counts, block_offsets, totals, src_of, rank_of, total;
    int nblocks;
};

DensifyLayout densify_layout(int P)
{
    DensifyLayout l;
    Carver c;
    l.nblocks = (P + TS_THREADS - 1) / TS_THREADS;
    l.flags = c.take((size_t)P);
    l.block_counts = c.take((size_t)l.nblocks * DC_N * sizeof(int));
    l.block_offsets = c.take((size_t)l.nblocks * DC_N * sizeof(int));
    l.totals = c.take(DC_N * sizeof(int));
    l.src_of = c.take(2 * (size_t)P * sizeof(int));
    l.rank_of = c.take((size_t)P * sizeof(int));
    l.total = c.off;
    return l;
}

int densify_check_ws(int P, const void* workspace, size_t workspace_bytes)
{
    if (P < 1 || P > DN_MAX_P) return fail(MI_RAST_ERR_INVALID, "densify: need 1 <= P < 2^30 rows");
    if (!workspace) return fail(MI_RAST_ERR_INVALID, "densify: null pointer");
    if (workspace_bytes < densify_layout(P).total) return fail(MI_RAST_ERR_INVALID, "densify: workspace smaller than mi_train_densify_workspace_bytes(P)");
    return MI_RAST_OK;
}

}  // namespace

extern "C" {

int mi_train_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const size_t* counts, const double* step_sizes, double inv_sqrt_bc2, double beta1, double beta2, double eps, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    static_assert(ADAM_MAX_TENSORS == MI_TRAIN_ADAM_MAX_TENSORS, "tensors per call");
    if (n_tensors < 1 || n_tensors > ADAM_MAX_TENSORS) return fail(MI_RAST_ERR_INVALID, "adam: need 1 <= n_tensors <= 16 per call");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !counts || !step_sizes) return fail(MI_RAST_ERR_INVALID, "adam: null table");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(MI_RAST_ERR_INVALID, "adam: need 0 <= beta < 1");
    if (!(eps >= 0.0) || !(inv_sqrt_bc2 > 0.0) || !std::isfinite(inv_sqrt_bc2)) return fail(MI_RAST_ERR_INVALID, "adam: need eps >= 0 and a finite 1 / sqrt(1 - beta2^t) > 0");
    AdamTable T = {};
    Range r[4 * ADAM_MAX_TENSORS];
    unsigned long long tiles = 0;
    T.n = n_tensors;
    for (int k = 0; k < n_tensors; k++) {
        AdamEntry& e = T.t[k];
        e.p = params[k], e.g = grads[k], e.m = exp_avg[k], e.v = exp_avg_sq[k];
        e.n = counts[k];
        e.step_size = (float)step_sizes[k];
        T.tile_begin[k] = (unsigned)tiles;
        const size_t bytes = e.n * sizeof(float);
        r[4 * k + 0] = {(const char*)e.p, bytes, true};
        r[4 * k + 1] = {(const char*)e.m, bytes, true};
        r[4 * k + 2] = {(const char*)e.v, bytes, true};
        r[4 * k + 3] = {(const char*)e.g, bytes, false};
        if (e.n == 0) continue;
        if (!e.p || !e.g || !e.m || !e.v) return fail(MI_RAST_ERR_INVALID, "adam: null pointer in a tensor with elements");
        if (e.n >= (1ull << 40)) return fail(MI_RAST_ERR_INVALID, "adam: 2^40 elements or more in one tensor");
        if (!std::isfinite(step_sizes[k])) return fail(MI_RAST_ERR_INVALID, "adam: a step size is not finite");
        const uintptr_t a = (uintptr_t)e.p;
        if (a % 4 || (uintptr_t)e.g % 4 || (uintptr_t)e.m % 4 || (uintptr_t)e.v % 4) return fail(MI_RAST_ERR_INVALID, "adam: a pointer is not 4-byte aligned");
        if (a % 16 == (uintptr_t)e.g % 16 && a % 16 == (uintptr_t)e.m % 16 && a % 16 == (uintptr_t)e.v % 16) {
            unsigned long long head = ((16 - a % 16) % 16) / 4;
            if (head > e.n) head = e.n;
            e.head = (unsigned)head;
            const unsigned long long nvec = (e.n - head) / 4;
            tiles += nvec ? (nvec + ADAM_TILE_VEC - 1) / ADAM_TILE_VEC : 1;
        } else {
            e.head = ADAM_SCALAR;
            tiles += (e.n + ADAM_TILE - 1) / ADAM_TILE;
        }
        if (tiles >= (1ull << 31)) return fail(MI_RAST_ERR_INVALID, "adam: too many elements in one call");
    }
    T.tile_begin[n_tensors] = (unsigned)tiles;
    if (outputs_overlap(r, 4 * n_tensors)) return fail(MI_RAST_ERR_INVALID, "adam: a parameter or moment overlaps another tensor of the call");
    if (tiles == 0) return MI_RAST_OK;
    AdamScalars s;
    s.inv_sqrt_bc2 = (float)inv_sqrt_bc2;
    s.omb1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.omb2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
    const unsigned grid = (unsigned)(tiles < (unsigned long long)ADAM_MAX_GRID ? tiles : ADAM_MAX_GRID);
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(TS_THREADS), 0, stream, T, s);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_train_densify_stats(int P, const int* radii, const float* viewspace_grad, float* xyz_gradient_accum, float* denom, float* max_radii2D,
                           void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return fail(MI_RAST_ERR_INVALID, "densify stats: P is negative");
    if (P == 0) return MI_RAST_OK;
    if (!radii || !viewspace_grad || !xyz_gradient_accum || !denom) return fail(MI_RAST_ERR_INVALID, "densify stats: null pointer");
    const size_t row = (size_t)P * sizeof(float);
    const Range r[5] = {{(const char*)xyz_gradient_accum, row, true}, {(const char*)denom, row, true}, {(const char*)max_radii2D, max_radii2D ? row : 0, true},
                        {(const char*)radii, row, false}, {(const char*)viewspace_grad, 3 * row, false}};
    if (outputs_overlap(r, 5)) return fail(MI_RAST_ERR_INVALID, "densify stats: an output overlaps another tensor of the call");
    hipLaunchKernelGGL(densify_stats_kernel, dim3((P + TS_THREADS - 1) / TS_THREADS), dim3(TS_THREADS), 0, stream, P, radii, viewspace_grad,
                       xyz_gradient_accum, denom, max_radii2D);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

size_t mi_train_densify_workspace_bytes(int P)
{
    if (P < 1 || P > DN_MAX_P) return 0;
    return densify_layout(P).total;
}

int mi_train_densify_plan(int P, const float* xyz_gradient_accum, const float* denom, const float* scaling, const float* opacity,
                          double max_grad, double min_opacity, double extent, double percent_dense, int use_screen_size,
                          void* workspace, size_t workspace_bytes, long long* split_rows, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = densify_check_ws(P, workspace, workspace_bytes)) return rc;
    if (!xyz_gradient_accum || !denom || !scaling || !opacity || !split_rows) return fail(MI_RAST_ERR_INVALID, "densify: null pointer");
    if (!(max_grad > 0.0)) return fail(MI_RAST_ERR_INVALID, "densify: max_grad must be > 0 (at 0 the reference selects its own zero-padded clone rows)");
    if (!(min_opacity == min_opacity) || !(extent == extent) || !(percent_dense == percent_dense)) return fail(MI_RAST_ERR_INVALID, "densify: a threshold is NaN");
    const DensifyLayout l = densify_layout(P);
    const size_t row = (size_t)P * sizeof(float);
    const Range r[6] = {{(const char*)workspace, l.total, true}, {(const char*)split_rows, (size_t)P * sizeof(long long), true},
                        {(const char*)xyz_gradient_accum, row, false}, {(const char*)denom, row, false}, {(const char*)scaling, 3 * row, false},
                        {(const char*)opacity, row, false}};
    if (outputs_overlap(r, 6)) return fail(MI_RAST_ERR_INVALID, "densify: the workspace or split_rows overlaps another tensor of the call");
    DensifyThresholds th;
    th.max_grad = (float)max_grad;
    th.dense = (float)(percent_dense * extent);
    th.min_opacity = (float)min_opacity;
    th.world = (float)(0.1 * extent);
    th.use_screen = use_screen_size ? 1 : 0;
    char* ws = (char*)workspace;
    unsigned char* flags = (unsigned char*)(ws + l.flags);
    int* block_counts = (int*)(ws + l.block_counts);
    int* block_offsets = (int*)(ws + l.block_offsets);
    int* totals = (int*)(ws + l.totals);
    hipLaunchKernelGGL(densify_plan_kernel, dim3(l.nblocks), dim3(TS_THREADS), 0, stream, P, xyz_gradient_accum, denom, scaling, opacity, th, flags,
                       block_counts);
    hipLaunchKernelGGL(block_scan_kernel<DC_N>, dim3(1), dim3(TS_THREADS), 0, stream, l.nblocks, (const int*)block_counts, block_offsets, totals);
    hipLaunchKernelGGL(densify_map_kernel, dim3(l.nblocks), dim3(TS_THREADS), 0, stream, P, (const unsigned char*)flags, (const int*)block_offsets,
                       (const int*)totals, (int*)(ws + l.src_of), (int*)(ws + l.rank_of), split_rows);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_train_densify_counts(int P, const void* workspace, size_t workspace_bytes, int* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = densify_check_ws(P, workspace, workspace_bytes)) return rc;
    if (!counts) return fail(MI_RAST_ERR_INVALID, "densify: null pointer");
    HIP_TRY(hipMemcpyAsync(counts, (const char*)workspace + densify_layout(P).totals, DC_N * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return MI_RAST_OK;
}

int mi_train_densify_apply(int P, const int* counts, int n_tensors, const float* const* src, float* const* dst, const int* cols, const int* kinds,
                           const float* samples, const void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = densify_check_ws(P, workspace, workspace_bytes)) return rc;
    if (!counts || !src || !dst || !cols || !kinds) return fail(MI_RAST_ERR_INVALID, "densify: null table");
    static_assert(DN_MAX_TENSORS == MI_TRAIN_DENSIFY_MAX_TENSORS, "tensors per call");
    if (n_tensors < 3 || n_tensors > DN_MAX_TENSORS) return fail(MI_RAST_ERR_INVALID, "densify: need 3 <= n_tensors <= 32");
    const long long n_split = counts[DC_SPLITS], n_orig = counts[DC_KEEP_ORIG], n_clone = counts[DC_KEEP_CLONE], n_child = counts[DC_KEEP_CHILD];
    if (counts[DC_CLONES] < 0 || n_split < 0 || n_orig < 0 || n_clone < 0 || n_child < 0 || counts[DC_CLONES] + n_split > P || n_orig + n_split > P ||
        n_clone > counts[DC_CLONES] || n_child > n_split)
        return fail(MI_RAST_ERR_INVALID, "densify: counts are not those of a plan over P rows");
    const long long new_rows = n_orig + n_clone + 2 * n_child;
    if (n_split > 0 && !samples) return fail(MI_RAST_ERR_INVALID, "densify: split rows need samples");
    const DensifyLayout l = densify_layout(P);
    GatherTable T = {};
    Range r[2 * DN_MAX_TENSORS + 2];
    int at[5] = {-1, -1, -1, -1, -1}, seen[5] = {0, 0, 0, 0, 0};
    size_t longest = 0;
    for (int k = 0; k < n_tensors; k++) {
        if (cols[k] < 1 || cols[k] > 4096) return fail(MI_RAST_ERR_INVALID, "densify: need 1 <= cols <= 4096");
        if (kinds[k] < DK_COPY || kinds[k] > DK_ROTATION) return fail(MI_RAST_ERR_INVALID, "densify: unknown tensor kind");
        if (!src[k] || (new_rows > 0 && !dst[k])) return fail(MI_RAST_ERR_INVALID, "densify: null pointer");
        if ((kinds[k] == DK_XYZ || kinds[k] == DK_SCALING) && cols[k] != 3) return fail(MI_RAST_ERR_INVALID, "densify: xyz and scaling have 3 columns");
        if (kinds[k] == DK_ROTATION && cols[k] != 4) return fail(MI_RAST_ERR_INVALID, "densify: rotation has 4 columns");
        at[kinds[k]] = k;
        seen[kinds[k]]++;
        T.t[k] = {src[k], dst[k], cols[k], kinds[k] == DK_MOMENT};
        r[2 * k] = {(const char*)src[k], (size_t)P * cols[k] * sizeof(float), false};
        r[2 * k + 1] = {(const char*)dst[k], (size_t)new_rows * cols[k] * sizeof(float), true};
        if ((size_t)new_rows * cols[k] > longest) longest = (size_t)new_rows * cols[k];
    }
    if (seen[DK_XYZ] != 1 || seen[DK_SCALING] != 1 || seen[DK_ROTATION] != 1)
        return fail(MI_RAST_ERR_INVALID, "densify: need exactly one xyz, one scaling and one rotation tensor");
    r[2 * n_tensors] = {(const char*)workspace, l.total, false};
    r[2 * n_tensors + 1] = {(const char*)samples, (size_t)(2 * n_split) * 3 * sizeof(float), false};
    if (outputs_overlap(r, 2 * n_tensors + 2)) return fail(MI_RAST_ERR_INVALID, "densify: an output overlaps another tensor of the call");
    if (new_rows == 0) return MI_RAST_OK;
    const char* ws = (const char*)workspace;
    const int* src_of = (const int*)(ws + l.src_of);
    hipLaunchKernelGGL(row_gather_kernel<true>, dim3(gather_grid_x(longest), (unsigned)n_tensors), dim3(TS_THREADS), 0, stream, T, P, (int)new_rows, (int)n_orig, src_of);
    if (n_child > 0)
        hipLaunchKernelGGL(densify_children_kernel, dim3((unsigned)((n_child + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, stream, P, (int)n_split,
                           (int)n_child, (int)(n_orig + n_clone), src_of, (const int*)(ws + l.rank_of), src[at[DK_XYZ]], src[at[DK_SCALING]],
                           src[at[DK_ROTATION]], samples, dst[at[DK_XYZ]], dst[at[DK_SCALING]]);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
