/*
 * lgm_lpips.h -- C ABI of the LPIPS (VGG16) loss kernels in liblgm_amd.so (lgm_amd/csrc/lpips.hip): the per-tap
 * distance and the input pass of core/models.py:156-165 (kiui's LPIPS(net='vgg') on the rendered and ground-truth
 * views). The thirteen convolutions of the trunk stay torch's; these kernels take the elementwise traffic around them.
 *
 * Distance. f0, f1 [N, C, H, W] contiguous, one dtype (codes of lgm_attn.h), w [C] fp32 (the tap's 1x1 head).
 *   out[n] = (1 / HW) sum_p sum_c w_c (f0 / (|f0|_p + eps) - f1 / (|f1|_p + eps))^2        (fp32)
 * with |.|_p the L2 norm over the channels at pixel p (eps: 1e-10 as published). Arithmetic is fp32. The difference
 * is evaluated as written (no a^2 - 2ab + b^2): bitwise identical inputs give exactly 0.0 and exactly zero gradients,
 * and with w >= 0 out is never negative. The forward stores the two norms |f0|_p, |f1|_p ([N, H, W] fp32 each, 1 / C
 * of the features) for the backward when norm0 / norm1 are not NULL (both or neither).
 * Backward, with g [N] fp32 (read on the device), d = f0^ - f1^ (the normalised features), A = |f0| + eps,
 * t0 = sum_k w_k d_k f0^_k:
 *   df0_c = g / (HW) (2 w_c d_c / A - 2 t0 f0_c / (|f0| A)),    df1 the same with the first term's sign flipped,
 * rounded once to the features' dtype. Either may be NULL and then costs no write. At a pixel whose norm is exactly 0
 * the second term is dropped (torch's composition returns NaN there: sqrt's backward at 0).
 * Every reduction runs in a fixed order (per-workgroup partial sums in the workspace, then one ordered sum) without
 * floating atomics: two calls on the same inputs are bitwise equal.
 * Pointers need only be element-aligned; 16-byte aligned tensors with HW % 4 == 0 take vector accesses.
 *
 * Input pass. pred [M, 3, S, S] fp32 in [0, 1]; optionally gt [M, 3, S, S], mask [M, 1, S, S], bg [3] (all fp32).
 * x_pred, x_gt [M, 3, R, R] (dtype_x) = affine(resize(v)): v = pred, or gt m + bg (1 - m) per source texel (mask
 * NULL: gt as it is); resize is bilinear with torch's align_corners = False rule (src = max((dst + 0.5) S / R - 0.5,
 * 0), upper index clamped to S - 1); affine is v -> (2 v - 1 - shift_c) / scale_c with LPIPS's published
 * shift = (-.030, -.088, -.188), scale = (.458, .448, .450). gt NULL: x_gt is not written.
 * Backward: d_pred [M, 3, S, S] fp32 from d_x_pred (dtype_x), as a gather over the destination pixels that tap each
 * source texel, in a fixed order.
 *
 * rc < 0 (and lgm_last_error), with nothing launched, on: C <= 0 or other bad sizes, f0 / f1 dtypes that differ or are
 * unknown, a launch grid beyond 2^31 - 1 workgroups, null pointers, or a workspace that is too small.
 * All work is enqueued on `stream` (a hipStream_t, NULL = default stream); nothing synchronises.
 */
#ifndef LGM_LPIPS_H
#define LGM_LPIPS_H
#include <stddef.h>

#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch the distance forward needs (one partial sum per workgroup). */
size_t lgm_lpips_dist_workspace_size(int N, int C, int H, int W);
int lgm_lpips_dist_forward(int dtype_f0, int dtype_f1, int N, int C, int H, int W, float eps, const void *f0,
                           const void *f1, const float *w, float *out, float *norm0, float *norm1, void *workspace,
                           size_t workspace_bytes, void *stream, const lgm_diag *diag);
int lgm_lpips_dist_backward(int dtype_f0, int dtype_f1, int N, int C, int H, int W, float eps, const void *f0,
                            const void *f1, const float *w, const float *norm0, const float *norm1, const float *g,
                            void *df0, void *df1, void *stream, const lgm_diag *diag);

int lgm_lpips_prep_forward(int dtype_x, int M, int S, int R, const float *pred, const float *gt, const float *mask,
                           const float *bg, void *x_pred, void *x_gt, void *stream, const lgm_diag *diag);
int lgm_lpips_prep_backward(int dtype_x, int M, int S, int R, const void *d_x_pred, float *d_pred, void *stream,
                            const lgm_diag *diag);

#ifdef __cplusplus
}
#endif
#endif
