/*
 * lgm_conv.h -- C ABI of the UNet's convolutions in liblgm_amd.so: the weight / bias gradient
 * (lgm_amd/csrc/conv_wgrad.hip), and the forward and the input gradient (lgm_amd/csrc/conv_fwd.hip, below).
 *
 * lgm_conv_wgrad replaces the weight / bias part of autograd through nn.Conv2d for the stride-1 3 x 3 and 1 x 1
 * convolutions of core/unet.py (ResnetBlock conv1 / conv2 / shortcut, UpBlock upsample, UNet conv_in / conv_out) under
 * accelerate's bf16 (or fp16) autocast. The forward and the input gradient are the library convolution unless the caller
 * opts into lgm_conv_forward / lgm_conv_dgrad.
 *
 * Operation. Stride 1, dilation 1, groups 1, padding p = (ksize - 1) / 2, ksize in {1, 3}:
 *
 *   dw[co][ci][ky][kx] = sum over n, y, x of dy[n][co][y][x] * X[n][ci][y + ky - p][x + kx - p]
 *   db[co]             = sum over n, y, x of dy[n][co][y][x]
 *
 * with X = x inside the image and zero outside it (the column before x = 0 and after x = W - 1, the row above y = 0 and
 * below y = H - 1: never a neighbouring row's, channel's or sample's elements). dw is fp32, [Cout][Cin][ksize][ksize]
 * contiguous; db is fp32 [Cout]; db NULL: not computed.
 *
 * Operands. dy is [N][Cout][H][W] and x is [N][Cin][H][W], both dense NCHW, both of dtype LGM_ATTN_BF16 or LGM_ATTN_F16
 * (lgm_attn.h codes). Any Cin, Cout >= 1 and any H, W >= 1. Pointers need only element (2-byte) alignment: an 8-element
 * group of a row is read by one 16-byte load where it is whole and 16-byte aligned and element by element otherwise, and
 * both forms give the same bits (the same values reach the same places of the same sums).
 *
 * Numerics. Products are exact and accumulated in fp32 on v_mfma_f32_16x16x32_{bf16,f16}; the pixel range is split S
 * ways and the S fp32 partials of an output are summed in split order. Every sum runs in an order that is a function of
 * (N, Cin, Cout, H, W, ksize, want_db) only -- not of addresses, nor of the timing of workgroups. No floating atomics:
 * two calls give equal bits. (torch rounds its 16-bit weight gradient to 16 bits before the cast back to the fp32
 * parameter; dw / db here are the unrounded fp32 sums.)
 *
 * Degenerate sizes. N * H * W == 0 with Cout, Cin > 0 writes zeros to dw and db, rc 0. Cin == 0 or Cout == 0 returns
 * rc 0 and does nothing.
 *
 * Errors. rc < 0 with lgm_last_error() set and nothing launched on: a dtype outside the two; ksize outside {1, 3}; a
 * negative size; a null dy / x / dw with work to do; a grid beyond 2^31 - 1 workgroups (or N * H beyond 2^31 - 1 rows);
 * a workspace shorter than lgm_conv_wgrad_workspace_size (any contents; it holds the fp32 split partials).
 *
 * All element offsets are 64-bit. Everything is enqueued on `stream`; nothing synchronises. Profiler labels:
 * k_conv_wgrad and k_conv_wgrad_reduce.
 */
#ifndef LGM_CONV_H
#define LGM_CONV_H
#include <stddef.h>

#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t lgm_conv_wgrad_workspace_size(int N, int Cin, int Cout, int H, int W, int ksize, int want_db);
int lgm_conv_wgrad(int dtype, int N, int Cin, int Cout, int H, int W, int ksize, const void *dy, const void *x,
                   float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream, const lgm_diag *diag);

/*
 * lgm_conv_forward / lgm_conv_dgrad -- the forward and the input gradient of the same convolutions.
 *
 * Operation. Stride 1, dilation 1, groups 1, padding p = (ksize - 1) / 2, ksize in {1, 3}:
 *
 *   y[n][co][y][x]  = bias[co] + sum over ci, ky, kx of w[co][ci][ky][kx] * X[n][ci][y + ky - p][x + kx - p]
 *   dx[n][ci][y][x] =            sum over co, ky, kx of w[co][ci][ky][kx] * DY[n][co][y - ky + p][x - kx + p]
 *
 * with X = x (DY = dy) inside the image and zero outside it: never a neighbouring row's, channel's or sample's
 * elements. The input gradient is the forward on the transposed, tap-flipped weight; both run one kernel body, the
 * weight index map is a mode of the packing pass.
 *
 * Operands. x is [N][Cin][H][W], y and dy are [N][Cout][H][W], dx is [N][Cin][H][W]: dense NCHW of `dtype`
 * LGM_ATTN_BF16 or LGM_ATTN_F16. w is [Cout][Cin][ksize][ksize] contiguous, of w_dtype = dtype or LGM_ATTN_F32; fp32
 * weights are rounded to dtype, round to nearest even (as tensor.to(dt)), by k_conv_wpack, which runs once per call and
 * writes the K-contiguous tiles the MFMA operand needs into the workspace. bias is NULL or [Cout] of bias_dtype = dtype
 * or LGM_ATTN_F32 (rounded to dtype like the weight, as autocast's cast of it does; bias_dtype is ignored where bias is
 * NULL). Any Cin, Cout, H, W >= 1. Pointers need only element
 * alignment (fp32 ones 4 bytes): activations are read element by element, and an output's four pixels go as one
 * 8-byte store where they are in one row and 8-byte aligned and as four 2-byte stores otherwise -- the same bits.
 *
 * Numerics. Products are exact and accumulated in fp32 on v_mfma_f32_16x16x32_{bf16,f16}, the bias is added in fp32,
 * then one rounding to the 16-bit output. The K range (the input channels, in steps of 32 with all their taps) may be
 * split S ways (small images with many channels): the S fp32 partials live in the workspace and are summed in split
 * order, then bias, then the rounding. Every sum runs in an order that is a function of (N, Cin, Cout, H, W, ksize)
 * only. No floating atomics: two calls give equal bits.
 *
 * Degenerate sizes. N * H * W == 0, or no output channel (Cout == 0 forward, Cin == 0 input gradient): rc 0, nothing
 * written. Cin == 0 forward writes the bias (zeros if NULL); Cout == 0 input gradient writes zeros.
 *
 * Errors. rc < 0 with lgm_last_error() set and nothing launched on: a dtype outside the two, a w_dtype / bias_dtype that
 * is neither fp32 nor dtype; ksize outside {1, 3}; a negative size; a null x / dy / w / y / dx with work to do; a grid
 * beyond 2^31 - 1 workgroups; a workspace shorter than lgm_conv_{forward,dgrad}_workspace_size (any contents; it holds
 * the packed weight and the split partials).
 *
 * All element offsets are 64-bit. Everything is enqueued on `stream`; nothing synchronises. Profiler labels:
 * k_conv_wpack, then k_conv_fwd or k_conv_dgrad, then k_conv_fwd_reduce where the K range is split.
 */
size_t lgm_conv_forward_workspace_size(int N, int Cin, int Cout, int H, int W, int ksize);
int lgm_conv_forward(int dtype, int w_dtype, int N, int Cin, int Cout, int H, int W, int ksize, const void *x,
                     const void *w, const void *bias, int bias_dtype, void *y, void *workspace, size_t workspace_bytes,
                     void *stream, const lgm_diag *diag);
size_t lgm_conv_dgrad_workspace_size(int N, int Cin, int Cout, int H, int W, int ksize);
int lgm_conv_dgrad(int dtype, int w_dtype, int N, int Cin, int Cout, int H, int W, int ksize, const void *dy,
                   const void *w, void *dx, void *workspace, size_t workspace_bytes, void *stream, const lgm_diag *diag);

#ifdef __cplusplus
}
#endif
#endif
