/*
 * lgm_meshraster.h -- C ABI of the triangle-mesh rasteriser in liblgm_amd.so (lgm_amd/csrc/meshraster.hip): a mesh of
 * lgm_mesh.h drawn from the Gaussian renderer's own cameras, and the gradient of the image to the mesh's texture (or to
 * its vertex colours). The reference's convert.py:364-442 rasterises its UV mesh with nvdiffrast and fits the texture to
 * renders of the Gaussians; this is the rasteriser of that stage (lgm_amd.mesh.render_mesh, fit_texture). There is no
 * antialiasing and no gradient to vertices or cameras. This header is the specification the tests
 * evaluate in fp64 (tests/mesh_raster_ref.py).
 *
 * ---- Inputs (DEVICE pointers, dense, row-major) ---------------------------------------------------------------------
 * vertices [Nv, 3] fp32, faces [Nf, 3] int32. cam_view, cam_view_proj [V, 4, 4]: exactly what lgm_render_forward takes
 * (the transposed matrices of core/gs.py:54-55, read as render_common.h xf43 / xf44 read them: row vector times matrix).
 * bg [3]. H, W >= 1: any size.
 *   texture mode (texture != NULL): uvs [Nu, 2] fp32, face_uvs [Nf, 3] int32 (per face corner, the row of uvs),
 *                texture [Ht, Wt, 3] fp32, row 0 at the top (v = 1): the layout of lgm_amd.mesh.Mesh. colors is ignored.
 *   colour mode  (texture == NULL): colors [Nv, 3] fp32; uvs, face_uvs, Nu, Ht, Wt are ignored.
 * Outputs: image [V, 3, H, W]; alpha [V, 1, H, W], 1 where a face is hit, otherwise 0; depth [V, 1, H, W], the view
 * depth of the hit, 0 where none; face_id [V, H, W] int32, -1 where none. depth and face_id may be NULL.
 *
 * ---- Forward --------------------------------------------------------------------------------------------------------
 * Projection, per (view, vertex), in fp32 with every operation rounded on its own (no contraction):
 *   clip = [x y z 1] . cam_view_proj,  w = clip.w,  z = ([x y z 1] . cam_view).z   (the view depth)
 *   X = ((clip.x / w + 1) W - 1) / 2,  Y = ((clip.y / w + 1) H - 1) / 2             (render_common.h ndc2pix: the
 *   division in fp32, the rest in fp64, rounded once), so pixel (x, y) of this rasteriser and of the Gaussian rasteriser
 *   is the same ray.
 * Near cut: a vertex is cut in a view if w <= 0.2 or any of X, Y, w, z is not finite. In a view, a face is dropped whole
 *   if any of its three vertices is cut (the renderer's own near cut, render_common.h preprocess_view; nothing is
 *   clipped). A face with an index outside [0, Nv) is dropped in every view; in texture mode so is a face with a
 *   face_uvs entry outside [0, Nu). The kernels guard this themselves (the host half never reads device memory):
 *   nothing is ever read or written out of bounds.
 * Coverage: with (xi, yi) = (Xi - x, Yi - y) the face's pixel-space vertices relative to the integer pixel centre (x, y),
 *   e0 = x1 y2 - x2 y1,  e1 = x2 y0 - x0 y2,  e2 = x0 y1 - x1 y0,  A = (e0 + e1) + e2   (the doubled signed area)
 *   b_i = e_i / A. The face covers the pixel iff A != 0 and b_0, b_1, b_2 >= 0. Both windings count (no back-face
 *   culling, as in nvdiffrast); the boundary is inclusive: a pixel on a shared edge belongs to both faces and the depth
 *   rule decides. Only the pixels of the face's box min X_i <= x <= max X_i, min Y_i <= y <= max Y_i are tested (every
 *   covered pixel lies in it).
 * Depth and visibility: q_i = b_i / w_i, iw = (q_0 + q_1) + q_2, beta_i = q_i / iw,
 *   depth = (beta_0 z_0 + beta_1 z_1) + beta_2 z_2. A hit whose depth is not in (0, inf) is discarded. The visible face
 *   of a pixel is the one with the smallest (depth, face index) pair, in lexicographic order: one 64-bit integer
 *   atomicMin of (fp32 bits of depth) << 32 | face (depth is positive: its bits order like its value). Integer atomics
 *   commute, so the forward is bitwise repeatable whatever the launch order. The shading pass recomputes beta for the
 *   winning face by the same operations (it is not stored).
 * Shading, texture mode: (u, v) = (beta_0 uv_0 + beta_1 uv_1) + beta_2 uv_2 with uv_i = uvs[face_uvs[f][i]];
 *   tx = u Wt - 1/2, ty = (1 - v) Ht - 1/2; ix = floor(tx), fx = tx - ix, likewise iy, fy; the four texels
 *   (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1), indices clamped to the texture (clamp to edge), with weights
 *   (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy, the four products summed in that order.
 * Shading, colour mode: (beta_0 c_0 + beta_1 c_1) + beta_2 c_2 with c_i = colors[faces[f][i]].
 * Pixels without a face get bg. Nf == 0 is valid: an all-background image.
 *
 * Kernels: k_mr_project (per (view, vertex): X, Y, w, z into the workspace, w = 0 marking a cut vertex: projected once,
 * reused by every face of the view), k_mr_vis (one thread per (view, face): walks the face's box when it holds at most
 * LGM_MESHRASTER_SMALL_BOX pixels, otherwise appends the face to a list in the workspace), k_mr_vis_big (one
 * workgroup per listed face at a time: its 256 threads stride over the box together, so no single lane serialises a
 * screen-sized box), k_mr_shade (one thread per pixel). Both visibility paths evaluate the same function on the same
 * operands, so which path a face takes changes no bit.
 *
 * ---- Backward -------------------------------------------------------------------------------------------------------
 * d_image [V, 3, H, W] -> d_texture [Ht, Wt, 3] (texture mode) or d_colors [Nv, 3] (colour mode): the exact adjoint of
 * the forward for fixed visibility. Every covered pixel adds, per channel, d_image times each of its four bilinear
 * weights to the four (clamped) texels, or times its three beta_i to the face's three vertices; bg and alpha get
 * nothing. The forward leaves the visibility buffer and the projected vertices in the workspace; the backward takes the
 * same workspace, untouched, with the same mesh and sizes, and leaves them as they are: a second backward on one forward
 * works. It is bitwise repeatable: the sums are int64 fixed point, integer atomics commute. With amax the largest
 * |d_image| of the call (k_mr_absmax, one reduction pass over all of d_image) and E the integer with
 * 2^(E - 1) <= amax < 2^E, the unit is 2^(E - S), S = lgm_meshraster_unit_log2(V, H, W) = 61 - ceil(log2(V H W)):
 * each product d w (fp32, rounded) is rounded to the nearest multiple of the unit (k_mr_scatter) and the sum converted
 * to fp32 once (k_mr_convert). Overflow bound: a pixel's weights sum to at most 1 + 2^-20 (fp32 rounding), so a
 * pixel adds fewer than 2^(S + 1) units in magnitude to any one accumulator, and the V H W <= 2^(61 - S) pixels together
 * fewer than 2^62: int64 cannot wrap.
 * The resolution is 2^-S of amax, at least 2^-30 (V H W < 2^31) and 2^-40 at 8 views of 512^2. amax == 0: zeros. A
 * non-finite amax (an Inf or NaN anywhere in d_image): every output element is NaN.
 *
 * ---- Errors ---------------------------------------------------------------------------------------------------------
 * rc < 0 (and lgm_last_error), with nothing launched, on: a null required pointer (cam_view, cam_view_proj, bg, image,
 * alpha, ws; vertices with Nv > 0; faces with Nf > 0; texture mode with Nf > 0: uvs, face_uvs; colour mode with Nf > 0:
 * colors; backward: d_image and d_texture or d_colors), V < 1, H or W < 1, a negative count, an element count >= 2^31
 * (3 Nv, 3 Nf, 2 Nu, 3 Ht Wt, 3 V H W, V Nv, V Nf), texture mode with Ht or Wt < 1, a workspace shorter than
 * lgm_meshraster_workspace_size says (LGM_E_WORKSPACE).
 * All work is enqueued on `stream` (a hipStream_t, NULL = default stream); nothing synchronises. The library keeps no
 * state: what the forward leaves for the backward lives in the caller's workspace.
 */
#ifndef LGM_MESHRASTER_H
#define LGM_MESHRASTER_H
#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGM_MESHRASTER_SMALL_BOX 64 /* a face whose box holds more pixels than this is drawn by a whole workgroup */

/* bytes of the workspace shared by forward and backward (Ht = Wt = 0 in colour mode); 0 on invalid sizes */
size_t lgm_meshraster_workspace_size(int V, long long Nv, long long Nf, int H, int W, int Ht, int Wt);

/* S of the backward's fixed-point unit (above): 61 - ceil(log2(V H W)); negative on invalid sizes */
int lgm_meshraster_unit_log2(int V, int H, int W);

int lgm_meshraster_forward(const float *vertices, long long Nv, const int *faces, long long Nf, const float *uvs,
                           long long Nu, const int *face_uvs, const float *texture, int Ht, int Wt, const float *colors,
                           const float *cam_view, const float *cam_view_proj, int V, const float *bg, int H, int W,
                           float *image, float *alpha, float *depth, int *face_id, void *ws, size_t ws_bytes,
                           void *stream, const lgm_diag *diag);

/* texture mode iff d_texture != NULL (then uvs, face_uvs, Ht, Wt as in the forward); otherwise d_colors */
int lgm_meshraster_backward(long long Nv, const int *faces, long long Nf, const float *uvs, long long Nu,
                            const int *face_uvs, int Ht, int Wt, int V, int H, int W, const float *d_image,
                            float *d_texture, float *d_colors, void *ws, size_t ws_bytes, void *stream,
                            const lgm_diag *diag);

#ifdef __cplusplus
}
#endif
#endif
