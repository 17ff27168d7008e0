/* mi_train_step.h -- C-ABI of the training step of the RGB loop, in libmi_rast.so.  The general conventions, the error codes and
 * mi_rast_last_error() are those of mi_rast.h.
 */
#ifndef MI_TRAIN_STEP_H
#define MI_TRAIN_STEP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the training step of the RGB loop (train_scene.py:126-138; csrc/mi_train_step.hip) ----
 * What follows loss.backward(): the Adam update of every parameter group, the densification statistics, and
 * scene/gaussian_model.py:566-578 (densify_and_prune, N = 2).  An extension: the reference does all of this in Python.
 * Device pointers everywhere except the small host tables named so below; nothing is allocated, nothing is kept between
 * calls; every result is bit-identical from run to run.  Arguments are checked before any HIP call. */

/* One Adam step of up to 16 tensors in ONE launch.  Host tables of n_tensors entries: params, grads, exp_avg, exp_avg_sq
 * (device pointers, binary32, 4-byte aligned), counts (elements; a tensor of 0 elements is skipped), step_sizes
 * (lr / (1 - beta1^t) per tensor).  inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t).  Per element, in binary32, each operation rounded:
 *     m += (g - m) (1 - beta1);   v = beta2 v + (1 - beta2) g g;   p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps)
 * (1 - beta) is formed in double and rounded once.  No weight decay, no amsgrad.  16-byte accesses where p, g, m and v share
 * their offset modulo 16, single floats before and after that body (and throughout where they do not). */
#define MI_TRAIN_ADAM_MAX_TENSORS 16
int mi_train_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const size_t* counts, const double* step_sizes, double inv_sqrt_bc2,
                       double beta1, double beta2, double eps, void* stream);

/* Per row with radii > 0:  xyz_gradient_accum += sqrt(gx^2 + gy^2) of viewspace_grad (P x 3), denom += 1,
 * max_radii2D = max(max_radii2D, (float)radii) (max_radii2D may be NULL).  Other rows are not touched. */
int mi_train_densify_stats(int P, const int* radii, const float* viewspace_grad, float* xyz_gradient_accum, float* denom,
                           float* max_radii2D, void* stream);

/* Densify and prune in three calls: plan (classes, counts and the row map, three launches, no host read), counts (THE one
 * host read: 5 ints), apply (gathers every tensor into the caller's new tensors).
 *   g = accum / denom (NaN -> 0);  big = max_k exp(s_k) > percent_dense extent;  clone: g >= max_grad and not big;
 *   split: g >= max_grad and big.  New rows: originals not split, clones, first children, second children, each in row order;
 *   of these, rows with sigmoid(o) < min_opacity are deleted, and with use_screen_size also rows with
 *   max_k exp(s_k) > 0.1 extent (children: their new s).  The reference has zeroed max_radii2D before it tests it against
 *   max_screen_size, so that test never deletes a row and is not made.  Thresholds are rounded to binary32 once.
 * counts[]: clones, splits, kept originals, kept clones, kept children PAIRS; new rows = [2] + [3] + 2 [4]. */
enum { MI_TRAIN_CLONES = 0, MI_TRAIN_SPLITS, MI_TRAIN_KEPT_ORIGINALS, MI_TRAIN_KEPT_CLONES, MI_TRAIN_KEPT_CHILDREN, MI_TRAIN_NCOUNTS };
size_t mi_train_densify_workspace_bytes(int P);   /* 0 when P < 1 or P >= 2^30 */
/* split_rows: int64[P]; its first counts[MI_TRAIN_SPLITS] entries are the split rows in order -- what the caller needs to
 * draw the samples: normal(0, exp(scaling[split_rows]) repeated twice), shape (2 splits, 3). */
int mi_train_densify_plan(int P, const float* xyz_gradient_accum, const float* denom, const float* scaling, const float* opacity,
                          double max_grad, double min_opacity, double extent, double percent_dense, int use_screen_size,
                          void* workspace, size_t workspace_bytes, long long* split_rows, void* stream);
/* counts: HOST int[MI_TRAIN_NCOUNTS].  Synchronises the stream. */
int mi_train_densify_counts(int P, const void* workspace, size_t workspace_bytes, int* counts, void* stream);
/* Host tables of n_tensors (3..32) entries: src (P x cols), dst (new rows x cols), cols, kinds.  A parameter's new row is its
 * source row bit for bit, except a child's xyz = R(q / |q|) sample + xyz and scaling = log(exp(s) / 1.6), the division evaluated as
 * exp(s) * (1.f / 1.6f) in binary32 (what a device division of a float32 tensor by a number does; a true division can differ in
 * the last bit); a MOMENT's row is its
 * source row for kept originals and 0 for every new row.  Exactly one XYZ, one SCALING and one ROTATION tensor.
 * counts: the host ints the counts call returned for this workspace. */
enum { MI_TRAIN_COPY = 0, MI_TRAIN_MOMENT = 1, MI_TRAIN_XYZ = 2, MI_TRAIN_SCALING = 3, MI_TRAIN_ROTATION = 4 };
#define MI_TRAIN_DENSIFY_MAX_TENSORS 32
int mi_train_densify_apply(int P, const int* counts, int n_tensors, const float* const* src, float* const* dst, const int* cols,
                           const int* kinds, const float* samples, const void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
