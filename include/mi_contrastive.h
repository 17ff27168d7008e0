/* mi_contrastive.h -- C-ABI of the contrastive-loss front end, in libmi_rast.so.
 *
 * Replaces, for the caller of the rasterizer's output, train_contrastive_feature.py:234-253:
 *
 *     rendered_feature_norm = rendered_features.norm(dim=0, p=2).mean()                       (:234)
 *     rendered_features = F.interpolate(rendered_features[None], (H, W), mode='bilinear')[0]  (:237)
 *     feature_with_scale = rendered_features[None].repeat(N, 1, 1, 1) * gates[:, :, None, None]   (:247-248)
 *     sampled = feature_with_scale[:, :, sampled_ray].permute(0, 2, 1)                        (:250-252)
 *     out = F.normalize(sampled, dim=-1, p=2)                                                 (:254)
 *
 * and their autograd backward.  The reference materialises an (N, C, H, W) tensor (2.6 GB at 10 x 32 x 1080p) before
 * it keeps S ~ 1000 rays; every step is per pixel, so the rays are bilinear-sampled FIRST (same weights as
 * F.interpolate(..., align_corners=False)).  The dense part -- the feature-norm regulariser -- is one streaming pass.
 *
 * forward : ONE launch.  Reads `rendered` (C, h, w) once: norm_sum[16 k] += partial sums over pixels of ||f(:, p)||_2 for
 *           k < MI_CONTRASTIVE_NORM_SLOTS (doubles, one per 128-byte line: same-address atomics serialise; the caller zeroes the
 *           MI_CONTRASTIVE_NORM_SLOTS * 16 doubles, adds the slots up and divides by h w), inv_norm[p] = 1 / ||f(:, p)|| (0 where the norm is 0, as torch's norm
 *           backward); and for the S rays `ray_yx` (pixel coordinates in the (H, W) mask grid, row-major order = the order
 *           boolean-mask indexing produces): ray_feat (S, C) = the bilinear samples, out (N, S, C) = normalize(ray * gate),
 *           inv_len (N, S) = 1 / max(||ray * gate||, 1e-12).
 * backward: two launches.  dL_drendered (C, h, w) is WRITTEN IN FULL: g_norm / (h w) * f * inv_norm (the regulariser term;
 *           g_norm = dL/d rendered_feature_norm, a device scalar, may be NULL = 0), then the 4 S C tap gradients of the rays
 *           are added with float atomics; dL_dgates (N, C) must be zeroed by the caller and receives atomics.
 *
 * All pointers are device pointers, fp32 unless noted, contiguous; `stream` is a hipStream_t.  C >= 1, N >= 1, S >= 0; with
 * rays (S > 0) also C <= 256 (a ray's wave holds four channels per lane) and N <= MI_CONTRASTIVE_LOSS_MAX_SCALES (32, what the
 * loss below accepts): outside those limits it is mi_contrastive_forward that refuses, so no forward succeeds whose backward
 * cannot run.  With S = 0 only the dense part runs, and it takes any C and N.  The backward reduces a workgroup's gate
 * gradients in at most 64 KiB of LDS, in passes of 4096 / C gates.  Algorithmic bytes: forward 4 C h w read (+ 4 h w written), backward 4 C h w read + 4 C h w written: three
 * streams of the feature image (265 MB each at 32 x 1080p); HBM-bound.
 * Returns 0 or an MI_RAST_ERR_* code (mi_rast_last_error() holds the text). */
#ifndef MI_CONTRASTIVE_H
#define MI_CONTRASTIVE_H

#define MI_CONTRASTIVE_NORM_SLOTS 64

#ifdef __cplusplus
extern "C" {
#endif

int mi_contrastive_forward(int C, int h, int w, const float* rendered, int H, int W, int S, const int* ray_yx /* [S,2] (y, x) */,
                           int N, const float* gates /* [N,C] */, float* out /* [N,S,C] */, float* ray_feat /* [S,C] */,
                           float* inv_len /* [N,S] */, float* inv_norm /* [h w] */, double* norm_sum /* [MI_CONTRASTIVE_NORM_SLOTS * 16], zeroed by the caller */,
                           void* stream);

int mi_contrastive_backward(int C, int h, int w, const float* rendered, int H, int W, int S, const int* ray_yx, int N,
                            const float* gates, const float* out, const float* ray_feat, const float* inv_len,
                            const float* inv_norm, const float* dL_dout /* [N,S,C] */, const float* g_norm /* [1] or NULL */,
                            float* dL_drendered /* [C,h,w], written in full */, float* dL_dgates /* [N,C], zeroed by the caller */,
                            void* stream);

#ifdef __cplusplus
}
#endif

/* ---- the loss itself: SAM-mask targets and the pair loss (train_contrastive_feature.py:145-226, :255-299) ----
 *
 * Masks are bit-packed: packed (M, H, Wq) 64-bit words, Wq = ceil(W / 64), bit b of word q = pixel 64 q + b, padding bits 0.
 * Sorted order = torch.sort(mask_scales, descending=True) indices (`sort_idx`, int64, device).  Wd = ceil(M / 64).
 * `acc` is one caller-ZEROED array of 5 + M unsigned 64-bit words shared by the calls of one iteration: [0..2] the pair-class
 * counts (consistent positive, consistent negative, inconsistent; full S x S matrix, diagonal included), [3] / [4] the largest
 * / the complement of the smallest mean mask size a (float bits), [5 .. 5+M) the exact per-mask areas in the masks' own order.
 * Limits: 1 <= M <= MI_CONTRASTIVE_LOSS_MAX_MASKS, 1 <= N <= MI_CONTRASTIVE_LOSS_MAX_SCALES, 1 <= C <= 256, S >= 0.
 *
 * pack    : one launch.  masks (M, H, W) bytes 0/1 -> packed.
 * cover   : one launch over the packed masks: the areas into acc[5..], sampled_ray (H, W) bytes = (any mask covers the pixel)
 *           && ray_rand[p] < rate (f32 compare, as torch compares an f32 tensor with a Python float).
 * targets : two launches for the S rays `ray_yx` (row-major (y, x) of sampled_ray, int32): gt (S, N, Wd) words -- for scale n
 *           every covering mask of sorted index > scale_si[n] plus the highest-index covering mask <= scale_si[n], or every
 *           covering mask when scale_ub[n] != 0 or scale_si[n] < 0 -- a (S) the area-weighted mean mask size, then the class
 *           counts into acc[0..2].
 * loss_forward : two launches.  feats (N, S, C) the normalised scale-conditioned features, rand (S, S) the device draw of :266;
 *           partials (S, 8) doubles of scratch.  out_f32 = {loss (the first two terms of :293-294), cosine_pos, cosine_neg},
 *           out_i64 = {n_pos, n_neg} (pairs h < j of sampled_mask_positive / _negative).  Deterministic: per-row partials, one
 *           fixed-order final reduction.
 * loss_backward : one launch.  dL_dfeats (N, S, C) WRITTEN IN FULL from g_loss (device f32 scalar), no atomics; it takes every
 *           selection through the same device functions as the forward (same out_i64 as that forward).
 * Returns 0 or an MI_RAST_ERR_* code (mi_rast_last_error() holds the text). */
#define MI_CONTRASTIVE_LOSS_MAX_MASKS 1024
#define MI_CONTRASTIVE_LOSS_MAX_SCALES 32

#ifdef __cplusplus
extern "C" {
#endif

int mi_contrastive_pack_masks(int M, int H, int W, const unsigned char* masks /* [M,H,W] */, unsigned long long* packed /* [M,H,Wq] */,
                              void* stream);

int mi_contrastive_cover(int M, int H, int W, const unsigned long long* packed, const float* ray_rand /* [H,W] */, float rate,
                         unsigned char* sampled_ray /* [H,W] */, unsigned long long* acc /* [5 + M], zeroed by the caller */, void* stream);

int mi_contrastive_targets(int M, int H, int W, const unsigned long long* packed, const long long* sort_idx /* [M] */, int S,
                           const int* ray_yx /* [S,2] */, int N, const int* scale_si /* [N] */, const int* scale_ub /* [N] */,
                           unsigned long long* gt /* [S,N,Wd] */, float* a /* [S] */, unsigned long long* acc, void* stream);

int mi_contrastive_loss_forward(int S, int N, int C, int M, const float* feats /* [N,S,C] */, const unsigned long long* gt,
                                const float* a, const unsigned long long* acc, const float* rand /* [S,S] */, double* partials /* [S,8] */,
                                float* out_f32 /* [3] */, long long* out_i64 /* [2] */, void* stream);

int mi_contrastive_loss_backward(int S, int N, int C, int M, const float* feats, const unsigned long long* gt, const float* a,
                                 const unsigned long long* acc, const float* rand, const long long* out_i64 /* of the forward */,
                                 const float* g_loss /* [1] */, float* dL_dfeats /* [N,S,C], written in full */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
