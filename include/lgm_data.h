/*
 * lgm_data.h -- C ABI of the training-batch assembly kernels in liblgm_amd.so (lgm_amd/csrc/data.hip): everything a
 * provider does after the PNG decode (core/provider_lvis.py:166-213 with core/utils.py get_rays, grid_distortion,
 * orbit_camera_jitter), from the decoded RGBA views and the raw poses to the `data` dict of LGM.forward. This header
 * is the specification the tests evaluate in fp64.
 *
 * lgm_data_cameras. c2w [B, V, 4, 4] fp32: OpenGL camera-to-world poses, translations already scaled by the provider.
 * Every matrix is taken in the affine form [R t; 0 1]: the last row is taken as (0, 0, 0, 1) whatever is stored there.
 *   P    = fl32(T(0, 0, cam_radius) inv(c2w[b, 0]) c2w[b, v])            (the normalised pose, all V views)
 *   pose_in[b, v] = jitter(P) for v < Vi                                  (P itself when jitter is NULL)
 *   P'   = P with columns 1 and 2 of its 3x3 block negated (OpenGL -> COLMAP); c2w_colmap[b, v] = P' for v < Vi
 *   cam_view = inv(P')^T, cam_view_proj = cam_view proj, cam_pos = -P'[:3, 3]                (all V views, from P:
 *   the jitter reaches the input poses only)
 * with proj the fp32 matrix of core/provider_lvis.py:59-65 (proj[0][0] = proj[1][1] = 1 / tan(fovy / 2),
 * proj[2][2] = (zfar + znear) / (zfar - znear), proj[3][2] = -zfar znear / (zfar - znear), proj[2][3] = 1).
 * Arithmetic is fp64, inverses by the adjugate of the 3x3 block (inv([R t; 0 1]) = [R^-1, -R^-1 t; 0 1]); each
 * output is rounded to fp32 once. cam_view and cam_view_proj are evaluated from P as rounded, so they are the
 * correctly rounded matrices of the pose the caller sees. With c2w[b, 0] the identity and cam_radius = 0, P = c2w
 * exactly: that is how a caller jitters poses that are already normalised.
 * jitter [B, Vi, 2] fp32: two uniform numbers u in [-1, 1) per input view (core/utils.py:45-61):
 *   rx = P[:3, 1] strength pi u0,   ry = P[:3, 0] strength pi / 2 u1,   rot = rodrigues(rx) rodrigues(ry),
 *   R <- rot R,  t <- rot t;   rodrigues(r) = I + a K + b K^2, K = [r]_x, theta = |r|, a = sinc(theta),
 *   b = sinc(theta / 2)^2 / 2 with sinc(0) = 1: u = (0, 0) gives rot = I and the pose comes back bitwise.
 * Outputs: pose_in [B, Vi, 4, 4], cam_view, cam_view_proj [B, V, 4, 4], cam_pos [B, V, 3]; c2w_colmap [B, Vi, 4, 4]
 * may be NULL.
 *
 * lgm_data_views. src [B, V, Hs, Ws, 4]: channel-last RGBA texels as a decoder delivers them, dtype_src =
 * LGM_DATA_U8 (bytes, value fl32(u / 255), the fp32 division's result: the u8 path equals the f32 path on u / 255 bit for bit)
 * or LGM_ATTN_F32 (values in [0, 1]). swap_rb: bit LGM_DATA_SWAP_RB: the texels are BGRA; bit LGM_DATA_NO_NORMALIZE:
 * input's channels 0..2 are img itself, without the ImageNet map (how grid_distortion alone is served). All outputs are
 * fp32, arithmetic is fp32 (sample coordinates fp64). Per source texel c = rgb a + (1 - a) (white background).
 * resize_R(f)[y, x] is bilinear with torch's align_corners = False rule, as in lgm_lpips.h, per axis:
 *   s = max((d + 0.5) S / R - 0.5, 0), i0 = min(floor(s), S - 1), i1 = min(i0 + 1, S - 1), l = s - i0,
 *   value = (1 - ly) ((1 - lx) f[y0, x0] + lx f[y0, x1]) + ly ((1 - lx) f[y1, x0] + lx f[y1, x1]),
 * for any Hs, Ws >= 1, up or down.
 *   images_output [B, V, 3, So, So] = resize_So(c),  masks_output [B, V, 1, So, So] = resize_So(a).
 *   input [B, Vi, 9, h, h]; channels 0..2 = (img - mean) / std with the ImageNet mean (.485, .456, .406) and std
 *   (.229, .224, .225), where for a view with nknots == 0 (or knots NULL) img = resize_h(c), and for a view with
 *   nknots == n, 2 <= n <= 17, img is the grid_distortion warp (core/utils.py:63-108) of resize_h(c):
 *     knots [B, Vi, 2, 17] int32 (DEVICE): row 0 the x knots kx, row 1 the y knots ky, entries 0 .. n - 1 used,
 *     non-decreasing, first 0, last h. Destination column j lies in segment i, kx[i] <= j < kx[i + 1], and has
 *       gx = g_i + (g_{i+1} - g_i) (j - kx[i]) / max(kx[i + 1] - kx[i] - 1, 1),   g_i = -1 + 2 i / (n - 1);
 *     rows the same with ky. Zero-length and one-column segments are legal. (A column no segment holds takes the
 *     last segment: that cannot happen with first 0 and last h.) Sampling is grid_sample's bilinear with zeros
 *     padding and align_corners = False: ix = ((gx + 1) h - 1) / 2, taps floor(ix) and floor(ix) + 1 with weights
 *     1 - frac and frac, a tap outside 0 .. h - 1 contributes 0 (border pixels blend with 0):
 *       img = (wy0 wx0 r[y0, x0] + wy0 wx1 r[y0, x1]) + (wy1 wx0 r[y1, x0] + wy1 wx1 r[y1, x1]),  r = resize_h(c).
 *     Each tap is evaluated from the source; the h x h view is never stored.
 *   nknots [B, Vi] int32 is a HOST array, read before the call returns (the host checks it; the kernels get the
 *   counts as launch arguments).
 *   channels 3..8 = the Pluecker embedding (o x d, d) of get_rays(pose_in[b, v], h, h, fovy) (core/utils.py:10-43):
 *     f = h / 2 / tan(fovy / 2),  dir = ((x - h / 2 + .5) / f, -(y - h / 2 + .5) / f, -1),  d = R dir,
 *     d <- d / sqrt(max(d.d, 1e-20)) (kiui's safe_normalize),  o = t, with [R t] = pose_in[b, v] (DEVICE, fp32).
 *   input, images_output or masks_output may be NULL (images_output and masks_output both or neither): that part is
 *   not computed. pose_in and nknots are needed only with input.
 * Two calls on the same inputs are bitwise equal (no atomics, one thread per output element group).
 * src must be aligned to its texel (4 bytes for u8, 16 for f32); outputs need only be element-aligned, 16-byte aligned
 * outputs with h % 4 == 0 (So % 4 == 0) take vector stores.
 *
 * rc < 0 (and lgm_last_error), with nothing launched, on: B, V, Vi, Hs, Ws, h or So <= 0 (B == 0: rc 0, nothing to
 * do), Vi > V, sizes above 32768, an unknown dtype, an nknots entry outside {0, 2 .. 17}, null required pointers, a
 * misaligned src, or a launch grid beyond 2^31 - 1 workgroups.
 * All work is enqueued on `stream` (a hipStream_t, NULL = default stream); nothing synchronises.
 */
#ifndef LGM_DATA_H
#define LGM_DATA_H
#include "lgm_attn.h"
#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGM_DATA_U8 3 /* dtype_src beside LGM_ATTN_F32: unsigned bytes, value u / 255 */
#define LGM_DATA_MAX_KNOTS 17
#define LGM_DATA_SWAP_RB 1      /* swap_rb bits */
#define LGM_DATA_NO_NORMALIZE 2

int lgm_data_cameras(int B, int V, int Vi, const float *c2w, const float *jitter, double jitter_strength,
                     double cam_radius, double fovy_deg, double znear, double zfar, float *pose_in, float *cam_view,
                     float *cam_view_proj, float *cam_pos, float *c2w_colmap, void *stream, const lgm_diag *diag);

int lgm_data_views(int dtype_src, int swap_rb, int B, int V, int Vi, int Hs, int Ws, int h, int So, const void *src,
                   const float *pose_in, const int *knots, const int *nknots, double fovy_deg, float *input,
                   float *images_output, float *masks_output, void *stream, const lgm_diag *diag);

#ifdef __cplusplus
}
#endif
#endif
