/*
 * lgm_conv.h -- C ABI of the weight / bias gradient of the UNet's convolutions in liblgm_amd.so
 * (lgm_amd/csrc/conv_wgrad.hip).
 *
 * Replaces the weight / bias part of autograd through nn.Conv2d for the stride-1 3 x 3 and 1 x 1 convolutions of
 * core/unet.py (ResnetBlock conv1 / conv2 / shortcut, UpBlock upsample, UNet conv_in / conv_out) under accelerate's bf16
 * (or fp16) autocast. The forward and the input gradient stay on the library convolution.
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

#ifdef __cplusplus
}
#endif
#endif
