/*
 * lgm_render.h -- C ABI of the MI355X-native Gaussian-splat render path (liblgm_amd.so).
 *
 * Replaces the external CUDA extension `diff_gaussian_rasterization._C` that LGM reaches through
 * core/gs.py:7-10 and calls once per (scene b, view v) at core/gs.py:58-85:
 *   - lgm_render_forward  replaces _C.rasterize_gaussians          (the per-view forward behind
 *                         GaussianRasterizer(...)(...) at core/gs.py:73-85), batched over all B x V views;
 *   - lgm_render_backward replaces _C.rasterize_gaussians_backward (driven by autograd from main.py:102
 *                         through the EXT autograd Function), batched likewise, and additionally performs the
 *                         sum over views + slice-gradient scatter that autograd does through the slices of
 *                         core/gs.py:45-49, writing dL/dgaussians [B,N,14] directly.
 * The Python side (lgm_amd/gs.py) keeps the reference's GaussianRenderer API (core/gs.py:16-98).
 *
 * Conventions (all pointers are DEVICE pointers unless stated; all arrays dense, row-major, fp32):
 *   gaussians      [B,N,14]  pos(3) opacity(1) scale(3) rotation(4: w,x,y,z) rgb(3)   (core/gs.py:45-49)
 *                  ([B,N,11 + 3K] with the LGM_RENDER_SH_MASK bits: spherical-harmonics coefficients in place of rgb)
 *   cam_view       [B,V,4,4] the transposed w2c exactly as core/gs.py:54 passes it (read column-major)
 *   cam_view_proj  [B,V,4,4] likewise (core/gs.py:55)
 *   bg             [3]
 *   image          [B,V,3,H,W] unclamped, or clamp(0, 1) as core/gs.py:87 when options has LGM_RENDER_CLAMP_IMAGE
 *   depth, alpha   [B,V,1,H,W]
 * Error behaviour: every entry point returns 0 on success and a negative LGM_E* code on failure; it never
 * throws across the ABI. lgm_last_error() returns a thread-local description of the last failure.
 * Threading: stream-ordered (all work is enqueued on `stream`, a hipStream_t passed as void*), no host
 * synchronisation inside forward/backward, reentrant; no global mutable state other than the error string: every
 * behaviour switch is a per-call `options` bit and diagnostics are a per-call `diag` (lgm_common.h; NULL = none).
 * Memory: caller-owned. Scratch and saved-for-backward state live in ONE caller-allocated workspace whose size
 * is given by lgm_render_workspace_size(); the same workspace must be passed, untouched, to the backward.
 */
#ifndef LGM_RENDER_H
#define LGM_RENDER_H

#include <stddef.h>
#include <stdint.h>

#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes for B x V renders of N Gaussians at H x W. pair_capacity <= 0 selects SLOT mode: every tile owns
 * room for N pairs (B*V*N*tiles*8 bytes, no counting pass, no host sync). pair_capacity > 0 selects PACKED mode
 * with room for that many (Gaussian, tile) pairs in total (from lgm_render_count_pairs). */
size_t lgm_render_workspace_size(int B, int V, int N, int H, int W, long long pair_capacity);

/* Exact pair counts over all B x V views. Enqueues a counting pass and writes pairs_out (a DEVICE int64[2]):
 *   [0] pairs actually binned (upstream's 3-sigma tile rect minus tiles where alpha < 1/255 is provable for every
 *       pixel -- the capacity a packed workspace needs), [1] upstream's num_rendered summed over views.
 * Used by callers that cannot afford the slot workspace; they synchronise once, size the workspace from [0] and
 * call lgm_render_forward with that pair_capacity. */
int lgm_render_count_pairs(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                           const float *cam_view_proj, float tanfovx, float tanfovy, float scale_modifier,
                           void *workspace, size_t workspace_bytes, long long *pairs_out, void *stream,
                           const lgm_diag *diag);

/* Forward of all B x V renders (replaces B*V calls of _C.rasterize_gaussians). radii_out [B,V,N] int32 may be
 * NULL. stats_out, if not NULL, is a DEVICE int64[2] with the counts described at lgm_render_count_pairs. */
int lgm_render_forward(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                       const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                       float scale_modifier, float *image, float *depth, float *alpha, int *radii_out,
                       void *workspace, size_t workspace_bytes, long long pair_capacity, long long *stats_out,
                       int options, void *stream, const lgm_diag *diag);

/* Backward of all B x V renders (replaces B*V calls of _C.rasterize_gaussians_backward plus the autograd sum
 * over views). d_image / d_depth / d_alpha may be NULL (treated as zero). Writes d_gaussians [B,N,14] (overwrites;
 * the width of gaussians with the LGM_RENDER_SH_MASK bits).
 * d_means2D [B,V,N,2] (screen-space gradients, what upstream returns for means2D) may be NULL. */
int lgm_render_backward(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                        const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                        float scale_modifier, const float *d_image, const float *d_depth, const float *d_alpha,
                        float *d_gaussians, float *d_means2D, void *workspace, size_t workspace_bytes,
                        long long pair_capacity, int options, void *stream, const lgm_diag *diag);

/* Loss-fused variants for training (core/models.py:133-167): with gt_images [B,V,3,H,W] and gt_masks [B,V,1,H,W]
 * (DEVICE fp32), the forward also composites the ground truth over bg (gt * mask + bg * (1 - mask)) and writes
 * loss_out (DEVICE float[4]) = (loss_mse, mse_image, mse_alpha, psnr) with loss_mse = F.mse_loss(image, gt) +
 * F.mse_loss(alpha, mask) and psnr = -10 log10(mse_image) -- per-tile partial sums inside the compositing kernel,
 * one fixed-order reduction, no separate loss kernels. The backward seeds dL/dimage and dL/dalpha in-kernel from
 * d_loss (DEVICE float[2] = dL/dmse_image, dL/dmse_alpha; both equal dL/dloss_mse for the plain sum) and the same
 * ground truth: 2 (image - gt) d_loss[0] / numel(image) (image after the clamp when LGM_RENDER_CLAMP_IMAGE) and
 * 2 (alpha - mask) d_loss[1] / numel(alpha), plus the optional d_image / d_alpha of other losses on the same
 * outputs (e.g. LPIPS, core/models.py:150-158; NULL = none). Pass the same options to both. */
int lgm_render_forward_loss(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                            const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                            float scale_modifier, float *image, float *depth, float *alpha, const float *gt_images,
                            const float *gt_masks, float *loss_out, void *workspace, size_t workspace_bytes,
                            long long pair_capacity, int options, void *stream, const lgm_diag *diag);
int lgm_render_backward_loss(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                             const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                             float scale_modifier, const float *d_image, const float *d_alpha,
                             const float *gt_images, const float *gt_masks, const float *d_loss,
                             float *d_gaussians, void *workspace, size_t workspace_bytes, long long pair_capacity,
                             int options, void *stream, const lgm_diag *diag);

/* Inspection of the state a forward left in its workspace (the equivalent of upstream's saved binningBuffer /
 * imgBuffer: point_list + ranges, n_contrib, accum_alpha), for parity tests and debugging. Stream-ordered.
 * lgm_render_tile_lists: tile_counts_out (DEVICE int32 [B*V*T], T = ceil(W/16)*ceil(H/16), tile-major per view)
 * receives each (view, tile)'s list length; if ids_out is not NULL, the tile's Gaussian ids in compositing
 * (depth, then id) order are copied to ids_out[offsets[bv*T + t] ...] (offsets: DEVICE int64 [B*V*T], e.g. the
 * exclusive cumsum of the counts). Replaces reading point_list[ranges[t].x .. ranges[t].y) of the EXT.
 * lgm_render_pixel_state: per-pixel n_contrib (1 + list position of the last accepted entry) and final
 * transmittance, [B,V,H,W] each (DEVICE; either may be NULL). */
int lgm_render_tile_lists(int B, int V, int N, int H, int W, const void *workspace, size_t workspace_bytes,
                          long long pair_capacity, int *tile_counts_out, const long long *offsets,
                          unsigned *ids_out, void *stream);
int lgm_render_pixel_state(int B, int V, int N, int H, int W, const void *workspace, size_t workspace_bytes,
                           long long pair_capacity, int *n_contrib_out, float *final_T_out, void *stream);
/* lgm_render_records: the per-(view, Gaussian) compositing records the binning wrote (upstream's geomBuffer:
 * means2D, conic_opacity, depths, tile rects), DEVICE, each [B,V,N,...] and each may be NULL:
 *   P_out [4] = (x, y, A', B'), Q_out [4] = (C', log2 opacity, tau', depth) with the conic pre-scaled as
 *   A' = -log2(e)/2 A, B' = -log2(e) B, C' = -log2(e)/2 C (tau' likewise; render_common.h rec_p / rec_q);
 *   rects_out [2] u32 = (x0 | y0 << 16, x1 | y1 << 16 | needle << 31), needle = the record's conic partials are
 *   accumulated in fp64 (float mode). Invisible records: rects (0, 0). */
int lgm_render_records(int B, int V, int N, int H, int W, const void *workspace, size_t workspace_bytes,
                       long long pair_capacity, float *P_out, float *Q_out, unsigned *rects_out, void *stream);
/* lgm_render_needle_flags: the float mode's needle decision (render_common.h rec_needle: conic condition
 * (A + C)^2 / (AC - B^2) above 300, or not positive definite; the record's conic partials then go to fp64
 * accumulators) evaluated on n caller-given DEVICE triples abc [n,3] = (A', B', C') as a record stores them ->
 * flags_out [n] (DEVICE u8, 1 = needle). The binning and the backward's flush take this same decision on the stored
 * record; a test pins it to separately rounded IEEE operations (no FP contraction) near the threshold. */
int lgm_render_needle_flags(long long n, const float *abc, unsigned char *flags_out, void *stream);
/* lgm_render_det_flush_limit_log2: LGM_RENDER_DETERMINISTIC's overflow bound, log2 of the largest |flush| (in
 * fixed-point units) the backward accepts into one int64 accumulator of a render with `views` views per scene and
 * `tiles` tiles per view: 62 - ceil(log2 F), F = the flushes one accumulator can take -- `tiles` for the per-view
 * records (mean2D, conic, depth), views * tiles for the per-scene ones (scene_record != 0: opacity, colour, summed
 * over the scene's views). Pure host function (no GPU); the kernel derives the same value. A flush above it is
 * counted and the call's gradients are poisoned with NaN. */
int lgm_render_det_flush_limit_log2(int views, int tiles, int scene_record);

/* Diagnostics: when diag->render_counters (a DEVICE uint64 buffer, caller-zeroed) is set, that call's render kernels
 * record per-workgroup timelines in it: [0..7] the backward's section cycles in the LGM_BWD_STAMPS diagnostic build (else unused);
 * then 8 entries per tile t (B*V*T tiles): s_memrealtime stamps (100 MHz) [8+8t] fwd start, [+1] fwd end,
 * [+2], [+3] the start / end of preprocess-backward workgroup t (t < its grid), [+4] sort start, [+5] sort end,
 * [+6] the tile's binned list length (low 32 bits; k_sort writes it, k_render_fwd rewrites it with the HW_ID of the
 * wave that composited the tile -- SE / CU / SIMD / slot -- in the high 32 bits), [+7] list entries the forward
 * staged (bits 0-31), wave 0's 4-entry steps (bits 32-55) and the XCC_ID of the XCD it ran on (bits 56-63); then 8
 * entries per binning workgroup
 * (room for B*V*ceil(N/512); the binning launch uses its first B*ceil(V/3)*ceil(N/512)): phase stamps [0] start,
 * [1] preprocessed, [2] tile tests done, [3] reserved, [4] end, [5] its binned pairs, [6] HW_ID and [7] XCC_ID of where it
 * ran; then 4 entries per backward work item (at most 3*B*V*tiles + 16 items: one per tile, rounded up to 8, and
 * one per checkpoint slot): start/end stamps, (entries | chunk << 20 | tile << 40) and (XCC_ID | HW_ID << 8) -- so the buffer
 * must hold 8 + 8*B*V*tiles + 8*B*V*ceil(N/512) + 4*(3*B*V*tiles + 16) entries. */

/* Per-call `options` of lgm_render_forward / lgm_render_backward (pass the same value to both).
 * LGM_RENDER_CLAMP_IMAGE: the forward writes clamp(image, 0, 1) (core/gs.py:87) and keeps a per-pixel mask in
 * the workspace; the backward passes d_image only where 0 <= unclamped <= 1 (torch's clamp gradient), so no
 * separate clamp kernels or unclamped copy are needed. */
#define LGM_RENDER_CLAMP_IMAGE 2
/* LGM_RENDER_BACKWARD_AGAIN (lgm_render_backward only): this workspace's forward has already been through a
 * backward (autograd with retain_graph): its gradient accumulators are cleared first. The forward's binning
 * zeroes them, so a first backward needs no clearing pass. */
#define LGM_RENDER_BACKWARD_AGAIN 4
/* (internal) set by lgm_render_forward_loss / lgm_render_backward_loss; ignored in `options`. */
#define LGM_RENDER_FUSED_LOSS 8
/* LGM_RENDER_DETERMINISTIC: bit-reproducible gradients. The per-view gradient accumulators become
 * int64 fixed point (integer atomics commute, so the sums do not depend on the order in which the backward's work
 * items finish) instead of fp32 float atomics. The units follow the data: 2^-30 of the call's largest per-pixel
 * seed |dL/dpixel| (found by one extra pass over the seeds), times per-(view, Gaussian) power-of-two normalisers of
 * the screen-space mean and conic partials -- so a mean-MSE loss's ~1e-9 seeds keep full resolution and large
 * footprints cannot overflow. The forward is deterministic in either mode. The workspace is larger: size it with
 * lgm_render_workspace_size_opts(..., options). Pass it to forward and backward alike. */
#define LGM_RENDER_DETERMINISTIC 16
size_t lgm_render_workspace_size_opts(int B, int V, int N, int H, int W, long long pair_capacity, int options);

/* LGM_RENDER_NO_CULL: bin upstream's full 3-sigma tile rects instead of dropping (Gaussian, tile) pairs where
 * alpha < 1/255 is provable for every pixel; outputs are identical either way
 * (tests/test_render_gpu.py::test_exact_culling_is_output_preserving), only the work differs. A packed workspace for
 * it needs lgm_render_count_pairs' pairs_out[1] (upstream's count) as its capacity. Per call, like every option. */
#define LGM_RENDER_NO_CULL 1

/* LGM_RENDER_ANTIALIAS: opacity compensation of the 0.3 px^2 dilation (the 3DGS rasteriser's `antialiasing` switch,
 * the Mip-Splatting 2D filter), so a splat smaller than a pixel keeps its integrated alpha instead of covering the
 * dilated footprint at full opacity. Per (view, Gaussian), with (a0, b, c0) the 2D covariance BEFORE the dilation
 * (the very sums the dilated a = a0 + 0.3, c = c0 + 0.3 are formed from, never a - 0.3):
 *   det0 = a0 c0 - b^2,  det = a c - b^2,  r = det0 / det,
 *   s = sqrt(min(1, fmaxf(2.5e-5, r)))      (fmaxf semantics: a NaN r gives 2.5e-5; r < 1 in exact arithmetic, the
 *                                            upper clamp only guards fp32 rounding and makes o^ <= o hold),
 *   o^ = o s  replaces the opacity o wherever it is consumed downstream: the record's L = log2(o^) (so
 *   lgm_render_records returns that), the o^ <= 1/255 early-out and tau = 2 ln(255 o^) of the exact cull.
 * Radius, 3-sigma rect, conic and depth do not change. With the bit off, not one operation or operand changes.
 * s is evaluated in fp64, by a pass of its own ahead of the binning, from the same fp32 inputs and the same sums
 * (a0 = T0 . Sigma T0, b, c0) and kept as fp32 per (view, Gaussian) in the workspace for the backward: det0 cancels
 * for an elongated splat (a0 c0 / det0 in the hundreds), and an fp32 evaluation carries that amplification of its
 * operands' rounding into log2 o^ (1e-5..1e-4). The constants are the rasteriser's fp32 literals (0.3f, 2.5e-5f).
 * Backward, the exact derivative: with G_v = dL/do^ of view v (what the compositing backward accumulates as the
 * opacity partial),
 *   dL/do = sum_v s_v G_v,   dL/ds_v = o G_v,   dL/dr = dL/ds_v / (2 s_v)  where 2.5e-5 < r <= 1, else 0,
 *   dr/da0 = (c0 det - det0 c) / det^2,  dr/dc0 = (a0 det - det0 a) / det^2,  dr/db = 2 b (det0 - det) / det^2
 *   (evaluated as 0.3 (c0 c + b^2), 0.3 (a0 a + b^2) and -2 b (0.3 (a0 + c0) + 0.09) over det^2: the same
 *   numerators with a - a0 = c - c0 = 0.3 put in, free of the cancellation of a large splat's products),
 * added to the conic's dL/da, dL/db, dL/dc before they are carried to the 3D covariance and the mean.
 * The opacity partial is then kept per VIEW ([B,V,N], fp32, or int64 fixed point with the per-view flush bound in
 * deterministic mode) after the other accumulators, followed by the factors s [B,V,N]: the workspace is larger, size
 * it with
 * lgm_render_workspace_size_opts(..., options); without the bit the workspace is byte for byte what it was. Pass
 * the bit to forward and backward alike (the loss-fused pair and packed mode included).
 * Packed capacity: lgm_render_count_pairs takes no options and counts with the uncompensated opacity. Its
 * pairs_out[0] remains a valid capacity for an antialiased forward: s <= 1, so o^ <= o, and every step of the cull
 * (the early-out, tau, the candidate rect, the tile tests) is monotone in the opacity -- the antialiased forward's
 * own stats_out[0] is at most that count. */
#define LGM_RENDER_ANTIALIAS 32

/* LGM_RENDER_SH_MASK: view-dependent colour from spherical harmonics (the 3DGS rasteriser's shs / sh_degree / campos
 * inputs). The degree is d = (options >> LGM_RENDER_SH_SHIFT) & 3. d = 0 is the plain RGB path: with the bits clear,
 * not one operation or operand changes. For d in 1..3, K = (d + 1)^2 and
 *   gaussians and d_gaussians are [B,N,11 + 3K]: columns 0:11 as ever, coefficient k of channel c at column
 *   11 + 3k + c (the 3DGS shs [N,K,3] order, DC first).
 * Colour, per (view v, Gaussian) with p the position:
 *   campos_v = -t M^-1, the point cam_view_v sends to the origin (M = cam_view[:3,:3], t = cam_view[3,:3] in the
 *   row-vector convention above; the inverse is taken in fp64, once per view and workgroup),
 *   dir = (p - campos_v) / |p - campos_v| = (x, y, z),   colour_c = max(0, 1/2 + sum_k Y_k(dir) sh[k][c]),
 * with the 3DGS rasteriser's real basis, signs and fp32 constants:
 *   C0 = 0.28209479177387814, C1 = 0.4886025119029199,
 *   C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396),
 *   C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
 *         1.445305721320277, -0.5900435899266435),
 *   Y_0 = C0;  Y_1..3 = -C1 y, C1 z, -C1 x;
 *   Y_4..8 = C2[0] xy, C2[1] yz, C2[2] (2zz - xx - yy), C2[3] xz, C2[4] (xx - yy);
 *   Y_9..15 = C3[0] y (3xx - yy), C3[1] xyz, C3[2] y (4zz - xx - yy), C3[3] z (2zz - 3xx - 3yy),
 *             C3[4] x (4zz - xx - yy), C3[5] z (xx - yy), C3[6] x (xx - 3yy).
 * A record the preprocess cuts in a view (view depth <= 0.2, zero radius, an empty tile rect ...) gets no colour and
 * no gradient from that view.
 * Backward: with G_vc the compositing backward's colour partial of view v and m_vc = 1 where the unclamped colour is
 * positive (else 0; upstream's `clamped`),
 *   dL/dsh[k][c] = sum_v Y_k(dir_v) m_vc G_vc,
 *   dL/dp += sum_v J_v^T g_v,  g_v = sum_c m_vc G_vc d(colour_c)/d(dir),  J_v the Jacobian of the normalisation,
 * added to the mean gradient the projection produces. No gradient reaches the cameras. The sums over views and
 * coefficients run in a fixed order, one writer per Gaussian, without float atomics in either accumulator mode.
 * The workspace is larger (per-view colours, clamp masks and colour partials -- fp32, or int64 fixed point with the
 * per-view bound lgm_render_det_flush_limit_log2(views, tiles, 0) in deterministic mode -- and 14-wide copies of the
 * rows for the kernels that know no other width): size it with lgm_render_workspace_size_opts(..., options). A
 * workspace sized without the bits is too short and returns LGM_E_WORKSPACE with nothing launched. Without the bits
 * the workspace is byte for byte what it was. Pass the bits to forward and backward alike; they combine with every
 * other option, the loss-fused pair and packed mode.
 * lgm_render_count_pairs takes no options and reads 14-wide rows: hand it a contiguous [B,N,14] copy of columns 0:14
 * (only 0:11 are read; colour does not enter the binning, so its counts hold for every degree). The inspection entry
 * points read regions that the bits do not move. */
#define LGM_RENDER_SH_SHIFT 6
#define LGM_RENDER_SH_MASK (3 << 6)

#ifdef __cplusplus
}
#endif
#endif
