/* mi_model_edit.h -- C-ABI of the model cut, in libmi_rast.so.  Error codes and mi_rast_last_error() are those of mi_rast.h.
 */
#ifndef MI_MODEL_EDIT_H
#define MI_MODEL_EDIT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Model edit: cut the Gaussian models by a selection (csrc/mi_model_edit.hip) ----
 *
 * The step that ends the segmentation workflow (scene/gaussian_model.py:376-472, scene/gaussian_model_ff.py:257-320;
 * saga_gui.py:662-688): keep the selected rows of every tensor of a model and record the cut.
 *
 * State: level [P0] f32, one entry per ORIGINAL row (the reference's _mask, all ones after load_ply), and segment_times.  The
 * CURRENT rows of the model are the original rows with level == segment_times + 1, in row order; n_rows is how many the caller's
 * tensors have.  mask [n_rows] holds one byte per current row, selected when non-zero.
 *
 * plan   : rank r of every current row among the current rows; a current row is selected when r < n_rows and mask[r] != 0; counts
 *          of current and selected rows per workgroup of 256 rows, each scanned by one workgroup.  Four launches, no host read.
 *          Nothing selected means everything kept: that rule is applied on the device, from the total, by apply's map kernel.
 * counts : the ONE host read: counts[MI_EDIT_CURRENT], [MI_EDIT_SELECTED] and [MI_EDIT_KEPT] (= selected, or current when none is
 *          selected).  Copies two ints and synchronises the stream.  A caller whose current != n_rows must not apply.
 * apply  : a map kernel writes src_of[output row] = current row (ascending) and adds one to level of every kept original row
 *          (level NULL: the map only -- a second model that shares the first one's level); then one gather launch copies
 *          n_tensors tensors, row for row through src_of, as 4-byte words: every output row is its source row bit for bit.
 *          src[k] is [n_rows][cols[k]], dst[k] is [kept][cols[k]]; a tensor with cols[k] == 0 is skipped (its pointers are not
 *          read).  counts must be what the counts call returned for this plan (they are checked against n_rows and each other);
 *          an entry of src_of outside [0, n_rows) reads row 0, so no read leaves a tensor.  Two launches.
 *          Algorithmic bytes: 5 P0 (level, flags) + n_rows (mask) in plan; 4 (kept rows read + kept rows written) in the gather.
 *
 * 1 <= n_rows <= P0 < 2^30, 0 <= segment_times < 2^24 (level is compared as binary32).  Device pointers, contiguous, 4-byte
 * aligned (mask: none); counts is a HOST pointer; outputs and the workspace must not overlap anything else of the call; `stream`
 * is a hipStream_t.  The workspace (mi_edit_workspace_bytes(P0) bytes, 5 P0 + a little) carries the plan from plan to apply and
 * is scratch otherwise.  No atomics, nothing allocated; bit-identical from run to run.  Returns 0 or an MI_RAST_ERR_* code.
 */
#define MI_EDIT_MAX_TENSORS 32
#define MI_EDIT_MAX_COLS 4096

enum { MI_EDIT_CURRENT = 0, MI_EDIT_SELECTED, MI_EDIT_KEPT, MI_EDIT_NCOUNTS };

/* 0 for P0 out of range */
size_t mi_edit_workspace_bytes(int P0);

int mi_edit_plan(int P0, const float* level /* [P0] */, int segment_times, int n_rows, const unsigned char* mask /* [n_rows] */,
                 void* workspace, size_t workspace_bytes, void* stream);

int mi_edit_counts(int P0, const void* workspace, size_t workspace_bytes, int* counts /* host, [MI_EDIT_NCOUNTS] */, void* stream);

int mi_edit_apply(int P0, int n_rows, const int* counts /* host, [MI_EDIT_NCOUNTS] */, float* level /* [P0] or NULL */,
                  int n_tensors, const float* const* src, float* const* dst, const int* cols, void* workspace,
                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
