/*
 * lgm_norm.h -- C ABI of the fused GroupNorm + SiLU (+ resample) kernels in liblgm_amd.so (lgm_amd/csrc/gnsilu.hip).
 *
 * Replaces the elementwise chain of core/unet.py:89-94 / :97-98 (ResnetBlock.forward: norm1 -> silu -> resample,
 * norm2 -> silu) and :315-316 (UNet.forward: norm_out -> silu) with one pass per direction. Under bf16 autocast the
 * reference runs GroupNorm in fp32, SiLU and the resample on that fp32 tensor, and rounds to bf16 at the next conv;
 * here the fp32 activation is rounded once, into `dtype_y`, so the values agree by construction.
 *
 * Forward: x [N, C, H, W] contiguous (dtype_x). Per (sample, group): mean and rstd = 1 / sqrt(var + eps) in fp32
 * (biased variance, centred sums). z = (x - mean) rstd gamma + beta, a = z sigmoid(z), y = resample(a) rounded once
 * to dtype_y: [N, C, H, W] (NONE), [N, C, 2H, 2W] (UP2, nearest) or [N, C, H/2, W/2] (DOWN2: the mean of the four fp32
 * values). gamma / beta fp32 [C] (NULL: 1 / 0). mean / rstd [N, groups] fp32 are kept for the backward.
 *
 * Backward: da = resample^T(d_y) (UP2: the fp32 sum of the four children; DOWN2: d_y / 4), dz = da s (1 + z (1 - s))
 * with s = sigmoid(z) and z recomputed from x, mean, rstd; then GroupNorm's backward on dz: dx (dtype_x, one rounding),
 * dgamma, dbeta (fp32 [C]); any of the three may be NULL.
 *
 * Every reduction runs in a fixed order without floating atomics: two calls on the same inputs are bitwise equal.
 * Supported dtype pairs (codes of lgm_attn.h): dtype_y == dtype_x, or dtype_x == f32 with any dtype_y.
 * Pointers need only be element-aligned (16-byte aligned tensors with 4-element rows take vector accesses).
 * rc < 0 (and lgm_last_error), with nothing launched, on: C % groups != 0, an odd H or W with DOWN2, an unsupported
 * dtype pair, a launch grid beyond 2^31 - 1 workgroups, null pointers, or a workspace that is too small.
 * All work is enqueued on `stream` (a hipStream_t, NULL = default stream); nothing synchronises.
 */
#ifndef LGM_NORM_H
#define LGM_NORM_H
#include <stddef.h>

#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGM_GN_RESAMPLE_NONE 0
#define LGM_GN_RESAMPLE_UP2 1   /* F.interpolate(scale_factor=2, mode="nearest") */
#define LGM_GN_RESAMPLE_DOWN2 2 /* nn.AvgPool2d(2, 2); H and W must be even */

/* Bytes of device scratch the forward needs (the chunk statistics of the chunked path; 0 where one launch does it). */
size_t lgm_gn_silu_workspace_size(int N, int C, int H, int W, int groups);
int lgm_gn_silu_forward(int dtype_x, int dtype_y, int N, int C, int H, int W, int groups, float eps, int resample,
                        const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd,
                        void *workspace, size_t workspace_bytes, void *stream, const lgm_diag *diag);
/* Bytes of device scratch the backward needs (per-tile partial sums, per-channel sums, per-group coefficients). */
size_t lgm_gn_silu_backward_workspace_size(int N, int C, int H, int W, int groups);
int lgm_gn_silu_backward(int dtype_x, int dtype_y, int N, int C, int H, int W, int groups, int resample,
                         const void *x, const float *gamma, const float *beta, const float *mean, const float *rstd,
                         const void *d_y, void *dx, float *dgamma, float *dbeta, void *workspace,
                         size_t workspace_bytes, void *stream, const lgm_diag *diag);

#ifdef __cplusplus
}
#endif
#endif
