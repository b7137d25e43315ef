"""Drop-in GaussianRenderer (core/gs.py:16-190) on the MI355X-native render path.

Same constructor (reads opt.fovy/znear/zfar at construction like core/gs.py:19-29 and opt.output_size at EVERY
render call like core/gs.py:59-60,92-93, because convert.py:188,265,366 mutate it), same `render` signature and
returned keys ("image" clamped to [0,1] as core/gs.py:87, "alpha"), plus an additive "depth" key, and the same
save_ply / load_ply. The B x V python loop of core/gs.py:42-90 and its B*V per-view extension calls (each with a
device->host sync) are replaced by ONE batched C-ABI call (include/lgm_render.h) per forward and per backward.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _native as nat
from . import sh as shm
from ._native import ptr
from .ply import read_ply, write_ply

# Slot-mode (sync-free, worst-case B*V*T*N pair slots) workspace when it fits; otherwise the pairs are counted
# exactly first (one host sync per batch -- the reference syncs once per VIEW for num_rendered). The slot workspace
# costs address space, not traffic (only the used part of each tile bucket is touched), but it is held from the
# forward to the backward: up to _WS_FREE_SLOT bytes it is taken without asking (cfg3 needs 1.2 GB, the 8-scene
# pool 9.8 GB); above, only if it fits half of the memory torch could still hand out (free device memory plus
# torch's cached-but-unused blocks) -- LGM 'big' with 20 views at 512^2 needs 25 GB, a 64-view training batch at
# 512^2 34 GB: taken on an idle 288 GB MI355X, counted exactly next to a large model. LGM_AMD_WS_BUDGET_GB fixes
# the limit instead.
_WS_BUDGET = int(float(os.environ["LGM_AMD_WS_BUDGET_GB"]) * (1 << 30)) if "LGM_AMD_WS_BUDGET_GB" in os.environ \
    else None
_WS_FREE_SLOT = 16 << 30


def _slot_fits(ws_bytes: int, dev) -> bool:
    if _WS_BUDGET is not None:
        return ws_bytes <= _WS_BUDGET
    if ws_bytes <= _WS_FREE_SLOT:
        return True
    free, _ = torch.cuda.mem_get_info(dev)
    avail = free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    return ws_bytes <= avail // 2


def _tiles(H: int, W: int) -> int:
    return ((W + 15) // 16) * ((H + 15) // 16)


def _count_pairs(g, cam_view, cam_view_proj, tanx, tany, scale_modifier, H, W):
    """lgm_render_count_pairs -> device int64 [2]: the (binned, reference) pair counts over all B x V views. The entry
    point takes no options and reads 14-wide rows: SH rows go in as a contiguous copy of their columns 0:14 (only 0:11
    are read -- colour does not enter the binning)."""
    g = _rows14(g)
    B, N, V = g.shape[0], g.shape[1], cam_view.shape[1]
    ws, ws_bytes = nat.workspace("lgm_render_workspace_size", g.device, B, V, N, H, W, 1, min_bytes=0)
    k = torch.zeros(2, dtype=torch.int64, device=g.device)
    nat.call("lgm_render_count_pairs", g.device, B, V, N, H, W, ptr(g), ptr(cam_view), ptr(cam_view_proj), tanx, tany,
             scale_modifier, ptr(ws), ws_bytes, ptr(k))
    return k


def _rows14(g):
    """What lgm_render_count_pairs is handed: the rows themselves if 14 wide, else a contiguous [B,N,14] copy of
    columns 0:14."""
    return g if g.shape[-1] == 14 else g[..., :14].contiguous()


class _RasterizeBatched(torch.autograd.Function):
    """Autograd Function over all B x V renders (replaces B*V applications of the EXT _RasterizeGaussians)."""

    @staticmethod
    def forward(ctx, g, cam_view, cam_view_proj, bg, tanx, tany, scale_modifier, H, W, options, gt_img=None,
                gt_mask=None):
        L = nat.lib()
        B, N = g.shape[0], g.shape[1]
        V = cam_view.shape[1]
        dev = g.device
        cap = 0
        ws_bytes = L.lgm_render_workspace_size_opts(B, V, N, H, W, 0, options)
        if not _slot_fits(ws_bytes, dev):
            # exact pair count (the reference syncs once per view for this; we sync once per batch)
            k = _count_pairs(g, cam_view, cam_view_proj, tanx, tany, scale_modifier, H, W)
            # pairs actually binned (upstream's full count with LGM_RENDER_NO_CULL). The count takes no options: with
            # LGM_RENDER_ANTIALIAS the forward bins with the compensated opacity o s <= o, and every step of the cull
            # is monotone in the opacity, so the uncompensated count is a valid (upper-bound) capacity for it
            # (include/lgm_render.h)
            cap = max(int(k[1 if options & nat.RENDER_NO_CULL else 0].item()), 1)
            ws_bytes = L.lgm_render_workspace_size_opts(B, V, N, H, W, cap, options)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)  # (sized above: not one nat.workspace question)
        image = torch.empty(B, V, 3, H, W, dtype=torch.float32, device=dev)
        depth = torch.empty(B, V, 1, H, W, dtype=torch.float32, device=dev)
        alpha = torch.empty(B, V, 1, H, W, dtype=torch.float32, device=dev)
        if gt_img is None:
            loss4 = torch.empty(0, dtype=torch.float32, device=dev)
            nat.call("lgm_render_forward", dev, B, V, N, H, W, ptr(g), ptr(cam_view), ptr(cam_view_proj), ptr(bg), tanx,
                     tany, scale_modifier, ptr(image), ptr(depth), ptr(alpha), None, ptr(ws), ws_bytes, cap, None,
                     options)
        else:
            # (loss_mse, mse_image, mse_alpha, psnr) of core/models.py:145-148,167, computed by the kernels
            loss4 = torch.empty(4, dtype=torch.float32, device=dev)
            nat.call("lgm_render_forward_loss", dev, B, V, N, H, W, ptr(g), ptr(cam_view), ptr(cam_view_proj), ptr(bg),
                     tanx, tany, scale_modifier, ptr(image), ptr(depth), ptr(alpha), ptr(gt_img), ptr(gt_mask),
                     ptr(loss4), ptr(ws), ws_bytes, cap, options)
        # the workspace is saved like an input: autograd frees it after a (non-retain_graph) backward, so a training
        # loop that keeps the previous step's outputs alive does not hold two workspaces
        ctx.save_for_backward(g, cam_view, cam_view_proj, bg, ws, gt_img, gt_mask, loss4)
        ctx.set_materialize_grads(False)  # unused outputs (LGM never uses depth) arrive as None, not zeros
        ctx.ws_bytes, ctx.cap = ws_bytes, cap
        ctx.params = (tanx, tany, scale_modifier, H, W, options)
        ctx.backwards = 0  # a repeated backward (retain_graph) must clear the previous one's accumulators
        return image, depth, alpha, loss4

    @staticmethod
    def backward(ctx, d_image, d_depth, d_alpha, d_loss4):
        g, cam_view, cam_view_proj, bg, ws, gt_img, gt_mask, loss4 = ctx.saved_tensors
        tanx, tany, scale_modifier, H, W, options = ctx.params
        B, N = g.shape[0], g.shape[1]
        V = cam_view.shape[1]
        d_image = None if d_image is None else d_image.float().contiguous()
        d_depth = None if d_depth is None else d_depth.float().contiguous()
        d_alpha = None if d_alpha is None else d_alpha.float().contiguous()
        d_g = torch.empty_like(g)
        bwd_options = options | (nat.RENDER_BACKWARD_AGAIN if ctx.backwards else 0)
        ctx.backwards += 1
        if gt_img is not None and d_loss4 is not None:
            if d_depth is not None:
                raise NotImplementedError("a depth gradient together with the fused loss (LGM's loss has no depth)")
            # d/dmse_image of loss_mse, mse_image and psnr = -10 log10(mse_image); d/dmse_alpha of loss_mse, mse_alpha
            d4 = d_loss4.float()
            # the PSNR term only where psnr is actually differentiated (GaussianRenderer.render detaches it, as the
            # reference computes it under no_grad): an exact fit (mse_image == 0) must not turn 0 / 0 into NaN
            d_psnr = torch.where(d4[3] != 0, d4[3] * (10.0 / math.log(10.0)) / loss4[1], torch.zeros_like(d4[3]))
            s2 = torch.stack([d4[0] + d4[1] - d_psnr, d4[0] + d4[2]]).contiguous()
            nat.call("lgm_render_backward_loss", g.device, B, V, N, H, W, ptr(g), ptr(cam_view), ptr(cam_view_proj),
                     ptr(bg), tanx, tany, scale_modifier, ptr(d_image), ptr(d_alpha), ptr(gt_img), ptr(gt_mask), ptr(s2),
                     ptr(d_g), ptr(ws), ctx.ws_bytes, ctx.cap, bwd_options)
        else:
            nat.call("lgm_render_backward", g.device, B, V, N, H, W, ptr(g), ptr(cam_view), ptr(cam_view_proj), ptr(bg),
                     tanx, tany, scale_modifier, ptr(d_image), ptr(d_depth), ptr(d_alpha), ptr(d_g), None, ptr(ws),
                     ctx.ws_bytes, ctx.cap, bwd_options)
        return d_g, None, None, None, None, None, None, None, None, None, None, None


def deterministic_enabled() -> bool:
    """Bit-reproducible render gradients (LGM_RENDER_DETERMINISTIC) when torch's deterministic algorithms are on
    (torch.use_deterministic_algorithms(True)) or LGM_AMD_DETERMINISTIC=1."""
    return torch.are_deterministic_algorithms_enabled() or os.environ.get("LGM_AMD_DETERMINISTIC", "0") == "1"


def rasterize(gaussians, cam_view, cam_view_proj, bg, tanfovx, tanfovy, H, W, scale_modifier=1.0, clamp=False,
              gt_images=None, gt_masks=None, deterministic=None, no_cull=False, antialias=False, sh_degree=None):
    """Functional form: returns (image [B,V,3,H,W], depth [B,V,1,H,W], alpha [B,V,1,H,W]). The image is
    unclamped unless clamp=True, which applies core/gs.py:87's clamp(0, 1) (and its gradient) inside the kernels.
    With gt_images [B,V,3,H,W] and gt_masks [B,V,1,H,W] a 4th output (loss_mse, mse_image, mse_alpha, psnr) holds
    LGM's training MSE terms (core/models.py:145-148,167), fused into the kernels; it is differentiable.
    no_cull=True bins upstream's full 3-sigma tile rects (LGM_RENDER_NO_CULL: same outputs, more work).
    antialias=True compensates the opacity for the 0.3 px^2 dilation (LGM_RENDER_ANTIALIAS, include/lgm_render.h:
    o sqrt(det cov / det(cov + 0.3 I)), the 3DGS rasteriser's `antialiasing`), forward and backward.
    sh_degree: view-dependent colour from spherical harmonics (LGM_RENDER_SH_MASK). None infers the degree from the
    row width: 14 is plain RGB, 23 / 38 / 59 are [B,N,11 + 3K] rows of degree 1 / 2 / 3 (coefficient k of channel c at
    column 11 + 3k + c, lgm_amd/sh.py); any other width, or one that contradicts an explicit degree, is a ValueError.
    The camera positions are derived from cam_view."""
    if gaussians.dim() != 3:
        raise ValueError(f"gaussians must be [B,N,14] or SH rows [B,N,23 / 38 / 59], got {tuple(gaussians.shape)}")
    degree = shm.degree_of(gaussians.shape[-1], sh_degree)
    if not gaussians.is_cuda:  # CPU tensors: the torch path of BASELINE config 1 (lgm_amd/cpu.py), never the oracle
        from .cpu import render_cpu
        bgc = torch.as_tensor(bg, dtype=torch.float32).detach().cpu()
        out = render_cpu(gaussians, cam_view.cpu(), cam_view_proj.cpu(), bgc, tanfovx, tanfovy, int(H), int(W),
                         scale_modifier, clamp=clamp, antialias=antialias)
        if gt_images is None and gt_masks is None:
            return out
        gt_c = gt_images * gt_masks + bgc.view(1, 1, 3, 1, 1) * (1 - gt_masks)  # core/models.py:145
        mi, ma = torch.nn.functional.mse_loss(out[0], gt_c), torch.nn.functional.mse_loss(out[2], gt_masks)
        return out + (torch.stack([mi + ma, mi, ma, -10 * torch.log10(mi)]),)
    for t, n in ((gaussians, "gaussians"), (cam_view, "cam_view"), (cam_view_proj, "cam_view_proj")):
        nat.require_device_tensor(t, n)
    g = gaussians.float().contiguous()
    dev = g.device
    cv = cam_view.to(dev, torch.float32).contiguous()
    cvp = cam_view_proj.to(dev, torch.float32).contiguous()
    bgt = torch.as_tensor(bg, dtype=torch.float32).to(dev).contiguous().detach()
    if cv.shape[:2] != cvp.shape[:2] or cv.shape[0] != g.shape[0] or cv.shape[-2:] != (4, 4):
        raise ValueError("cam_view / cam_view_proj must be [B,V,4,4] with B matching gaussians")
    gti = gtm = None
    if gt_images is not None or gt_masks is not None:
        B, V = cv.shape[0], cv.shape[1]
        gti = gt_images.to(dev, torch.float32).contiguous().detach()
        gtm = gt_masks.to(dev, torch.float32).contiguous().detach()
        if tuple(gti.shape) != (B, V, 3, H, W) or tuple(gtm.shape) != (B, V, 1, H, W):
            raise ValueError("gt_images / gt_masks must be [B,V,3,H,W] / [B,V,1,H,W]")
    options = (nat.RENDER_CLAMP_IMAGE if clamp else 0) | (nat.RENDER_NO_CULL if no_cull else 0) | \
        (nat.RENDER_ANTIALIAS if antialias else 0) | (degree << nat.RENDER_SH_SHIFT)
    if deterministic_enabled() if deterministic is None else deterministic:
        options |= nat.RENDER_DETERMINISTIC
    out = _RasterizeBatched.apply(g, cv, cvp, bgt, float(tanfovx), float(tanfovy), float(scale_modifier),
                                  int(H), int(W), options, gti, gtm)
    return out if gti is not None else out[:3]


def count_pairs(gaussians, cam_view, cam_view_proj, tanfovx, tanfovy, H, W, scale_modifier=1.0):
    """(binned, reference) (Gaussian, tile) pair counts over all B x V views (one host sync): `binned` after the
    exact opacity-aware tile culling, `reference` = upstream's num_rendered summed over views (SURVEY §8(d)'s K)."""
    g = gaussians.float().contiguous()
    cv = cam_view.to(g.device, torch.float32).contiguous()
    cvp = cam_view_proj.to(g.device, torch.float32).contiguous()
    kk = _count_pairs(g, cv, cvp, float(tanfovx), float(tanfovy), float(scale_modifier), H, W).tolist()
    return int(kk[0]), int(kk[1])


def forward_state(gaussians, cam_view, cam_view_proj, tanfovx, tanfovy, H, W, scale_modifier=1.0, lists=False,
                  no_cull=False, records=False, antialias=False, sh_degree=None):
    """Runs one forward and returns what it left in its workspace (numpy, one host sync), for parity tests and
    debugging -- the equivalent of reading upstream's saved buffers (radii, point_list/ranges, n_contrib):
      radii [B,V,N] int32; K_binned / K_reference (as count_pairs); tile_counts [B,V,T] int32;
      n_contrib, final_T [B,V,H,W]; with lists=True, ids[b][v] = the view's tile lists concatenated (tile-major,
      each in compositing order); with records=True, the compositing records P, Q [B,V,N,4] and rects [B,V,N,2]
      (uint32) of lgm_render_records. no_cull=True bins upstream's full 3-sigma rects (LGM_RENDER_NO_CULL);
      antialias=True renders with LGM_RENDER_ANTIALIAS (the records' L is then log2 of the compensated opacity);
      sh_degree as rasterize (SH rows; the state read here does not depend on the colours)."""
    options = (nat.RENDER_NO_CULL if no_cull else 0) | (nat.RENDER_ANTIALIAS if antialias else 0) | \
        (shm.degree_of(gaussians.shape[-1], sh_degree) << nat.RENDER_SH_SHIFT)
    L = nat.lib()
    g = gaussians.float().contiguous()
    dev = g.device
    B, N, V = g.shape[0], g.shape[1], cam_view.shape[1]
    cv = cam_view.to(dev, torch.float32).contiguous()
    cvp = cam_view_proj.to(dev, torch.float32).contiguous()
    stream = nat.stream_of(dev)  # (the inspection copies below take a stream and no diag: plain lib() calls)
    # (sized with the options: LGM_RENDER_ANTIALIAS's workspace is larger; the state read below lies before that)
    ws, ws_bytes = nat.workspace("lgm_render_workspace_size_opts", dev, B, V, N, H, W, 0, options, min_bytes=0)
    bg = torch.zeros(3, device=dev)
    image = torch.empty(B, V, 3, H, W, device=dev)
    depth = torch.empty(B, V, 1, H, W, device=dev)
    alpha = torch.empty(B, V, 1, H, W, device=dev)
    radii = torch.empty(B, V, N, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    nat.call("lgm_render_forward", dev, B, V, N, H, W, ptr(g), ptr(cv), ptr(cvp), ptr(bg), float(tanfovx),
             float(tanfovy), float(scale_modifier), ptr(image), ptr(depth), ptr(alpha), ptr(radii), ptr(ws), ws_bytes, 0,
             ptr(stats), options)
    T = _tiles(H, W)
    counts = torch.empty(B * V * T, dtype=torch.int32, device=dev)
    nat.check(L.lgm_render_tile_lists(B, V, N, H, W, ptr(ws), ws_bytes, 0, ptr(counts), None, None, stream),
              "lgm_render_tile_lists")
    n_contrib = torch.empty(B, V, H, W, dtype=torch.int32, device=dev)
    final_T = torch.empty(B, V, H, W, dtype=torch.float32, device=dev)
    nat.check(L.lgm_render_pixel_state(B, V, N, H, W, ptr(ws), ws_bytes, 0, ptr(n_contrib), ptr(final_T), stream),
              "lgm_render_pixel_state")
    out = {"radii": radii.cpu().numpy(), "tile_counts": counts.view(B, V, T).cpu().numpy(),
           "n_contrib": n_contrib.cpu().numpy(), "final_T": final_T.cpu().numpy()}
    k = stats.tolist()
    out["K_binned"], out["K_reference"] = int(k[0]), int(k[1])
    if lists:
        c64 = counts.to(torch.int64)
        offsets = (torch.cumsum(c64, 0) - c64).contiguous()
        total = int(c64.sum().item())
        ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        nat.check(L.lgm_render_tile_lists(B, V, N, H, W, ptr(ws), ws_bytes, 0, ptr(counts), ptr(offsets), ptr(ids),
                                          stream), "lgm_render_tile_lists")
        flat = ids[:total].cpu().numpy()
        per_view = c64.view(B * V, T).sum(1).tolist()
        bounds = np.concatenate([[0], np.cumsum(per_view)])
        out["ids"] = [[flat[bounds[b * V + v]:bounds[b * V + v + 1]] for v in range(V)] for b in range(B)]
    if records:
        P = torch.empty(B, V, N, 4, device=dev)
        Q = torch.empty(B, V, N, 4, device=dev)
        rects = torch.empty(B, V, N, 2, dtype=torch.int32, device=dev)
        nat.check(L.lgm_render_records(B, V, N, H, W, ptr(ws), ws_bytes, 0, ptr(P), ptr(Q), ptr(rects), stream),
                  "lgm_render_records")
        out["P"], out["Q"] = P.cpu().numpy(), Q.cpu().numpy()
        out["rects"] = rects.cpu().numpy().view(np.uint32)
    return out


class GaussianRenderer:
    """core/gs.py:16 GaussianRenderer, same API."""

    def __init__(self, opt):
        self.opt = opt
        # core/gs.py:20 creates this on "cuda"; here it follows the Gaussians' device at render time.
        self.bg_color = torch.tensor([1, 1, 1], dtype=torch.float32,
                                     device="cuda" if torch.cuda.is_available() else "cpu")
        self.tan_half_fov = np.tan(0.5 * np.deg2rad(self.opt.fovy))
        self.proj_matrix = torch.zeros(4, 4, dtype=torch.float32)
        self.proj_matrix[0, 0] = 1 / self.tan_half_fov
        self.proj_matrix[1, 1] = 1 / self.tan_half_fov
        self.proj_matrix[2, 2] = (opt.zfar + opt.znear) / (opt.zfar - opt.znear)
        self.proj_matrix[3, 2] = -(opt.zfar * opt.znear) / (opt.zfar - opt.znear)
        self.proj_matrix[2, 3] = 1

    def render(self, gaussians, cam_view, cam_view_proj, cam_pos, bg_color=None, scale_modifier=1, gt_images=None,
               gt_masks=None, antialias=None, sh_degree=None):
        """core/gs.py:31-98. gaussians [B,N,14], or SH rows [B,N,23 / 38 / 59] (sh_degree as rasterize: None infers
        it from the width); cam_view, cam_view_proj [B,V,4,4]; cam_pos [B,V,3] is accepted and unused: the SH
        directions take the camera positions the kernels derive from cam_view. Additive: with gt_images / gt_masks (the `images_output` / `masks_output` of
        core/models.py:140-141) the result also holds LGM's MSE loss terms, computed in the render kernels:
        "loss_mse" (differentiable: its backward seeds the render backward in-kernel), "mse_image", "mse_alpha"
        and "psnr" (core/models.py:145-148,165-167). antialias (additive; None reads opt.antialias, default off):
        the opacity compensation of rasterize(antialias=True)."""
        S = int(self.opt.output_size)
        bg = self.bg_color if bg_color is None else bg_color
        tan = float(self.tan_half_fov)
        # core/gs.py:87's clamp(0, 1) and its gradient are applied inside the kernels
        out = rasterize(gaussians, cam_view, cam_view_proj, bg, tan, tan, S, S, scale_modifier, clamp=True,
                        gt_images=gt_images, gt_masks=gt_masks,
                        antialias=bool(getattr(self.opt, "antialias", False) if antialias is None else antialias),
                        sh_degree=sh_degree)
        res = {"image": out[0], "alpha": out[2], "depth": out[1]}
        if len(out) == 4:
            loss4 = out[3]
            res.update(loss_mse=loss4[0], mse_image=loss4[1], mse_alpha=loss4[2], psnr=loss4[3].detach())
        return res

    def save_ply(self, gaussians, path, compatible=True):
        """core/gs.py:101-152: B == 1, prune opacity < 0.005, optionally invert activations (3DGS PLY layout).
        SH rows [1,N,11 + 3K] (lgm_amd/sh.py) also write f_rest_0 .. f_rest_{3(K-1)-1} in 3DGS's property order
        (channel-major: f_rest_i holds coefficient 1 + i % (K - 1) of channel i // (K - 1), after f_dc_*); their
        coefficients are stored as they are (the DC is a coefficient already: no C0 x + 1/2 to invert)."""
        assert gaussians.shape[0] == 1, "only support batch size 1"
        g = gaussians[0].detach().float().cpu()
        degree = shm.degree_of(g.shape[-1])
        means3D, opacity, scales, rotations = g[:, 0:3], g[:, 3:4], g[:, 4:7], g[:, 7:11]
        shs = g[:, 11:].reshape(g.shape[0], -1, 3)  # [N, K, 3] (K = 1: the RGB)
        mask = opacity.squeeze(-1) >= 0.005
        means3D, opacity, scales, rotations, shs = means3D[mask], opacity[mask], scales[mask], rotations[mask], shs[mask]
        if compatible:
            o = opacity.clamp(1e-6, 1 - 1e-6)
            opacity = torch.log(o / (1 - o))  # kiui.op.inverse_sigmoid
            scales = torch.log(scales + 1e-8)
            if not degree:
                shs = (shs - 0.5) / 0.28209479177387814
        f_dc = shs[:, :1].transpose(1, 2).flatten(start_dim=1).contiguous()
        f_rest = shs[:, 1:].transpose(1, 2).flatten(start_dim=1).contiguous()  # [N, 3 (K - 1)], channel-major
        names = ["x", "y", "z"] + [f"f_dc_{i}" for i in range(f_dc.shape[1])] + \
                [f"f_rest_{i}" for i in range(f_rest.shape[1])] + ["opacity"] + \
                [f"scale_{i}" for i in range(scales.shape[1])] + [f"rot_{i}" for i in range(rotations.shape[1])]
        data = torch.cat([means3D, f_dc, f_rest, opacity, scales, rotations], dim=1).numpy().astype(np.float32)
        write_ply(path, names, data)

    def save_mesh(self, gaussians, path, **kw):
        """Additive (the reference's convert.py step): B == 1 as in save_ply; the Gaussians as a closed, coloured triangle
        mesh (lgm_amd.mesh.gaussians_to_mesh, whose keywords `kw` are) written as .obj, or .ply by the path's
        extension. fit_iters=K (with texels): the baked texture fitted to renders from this renderer's cameras
        (lgm_amd.meshraster.fit_texture). Returns the Mesh."""
        from .mesh import gaussians_to_mesh
        assert gaussians.shape[0] == 1, "only support batch size 1"
        if kw.get("fit_iters"):
            kw.setdefault("opt", self.opt)
        mesh = gaussians_to_mesh(gaussians, **kw)
        if str(path).lower().endswith(".ply"):
            mesh.save_ply(path)
        else:
            mesh.save_obj(path)
        return mesh

    def load_ply(self, path, compatible=True, sh=False):
        """core/gs.py:154-190: returns a CPU [N,14] tensor (the f_rest_* properties of an SH file are dropped: its DC
        colour). sh=True keeps them: a file with 9 / 24 / 45 f_rest_* properties (degree 1 / 2 / 3; another count is
        a ValueError) gives [N,11 + 3K] SH rows (lgm_amd/sh.py) -- the DC kept as a coefficient, without the
        C0 x + 1/2 activation, f_rest_i read in 3DGS's channel-major order i = c (K - 1) + (k - 1); a file without
        f_rest_* gives the [N,14] tensor either way."""
        props = read_ply(path)
        xyz = np.stack([props["x"], props["y"], props["z"]], axis=1)
        print("Number of points at loading : ", xyz.shape[0])
        opac = props["opacity"][:, None]
        shs = np.stack([props["f_dc_0"], props["f_dc_1"], props["f_dc_2"]], axis=1)
        sn = sorted([k for k in props if k.startswith("scale_")], key=lambda s: int(s.split("_")[-1]))
        rn = sorted([k for k in props if k.startswith("rot_")], key=lambda s: int(s.split("_")[-1]))
        scales = np.stack([props[k] for k in sn], axis=1)
        rots = np.stack([props[k] for k in rn], axis=1)
        rest = sorted([k for k in props if k.startswith("f_rest_")], key=lambda s: int(s.split("_")[-1]))
        if sh and rest:
            if len(rest) not in (9, 24, 45):
                raise ValueError(f"{path}: {len(rest)} f_rest_* properties; SH degree 1 / 2 / 3 has 9 / 24 / 45")
            K1 = len(rest) // 3  # K - 1; f_rest is [3, K - 1] channel-major -> rows [K - 1, 3]
            fr = np.stack([props[k] for k in rest], axis=1).reshape(-1, 3, K1).transpose(0, 2, 1).reshape(-1, 3 * K1)
            shs = np.concatenate([shs, fr], axis=1)
        gaussians = torch.from_numpy(np.concatenate([xyz, opac, scales, rots, shs], axis=1).astype(np.float64)).float()
        if compatible:
            gaussians[..., 3:4] = torch.sigmoid(gaussians[..., 3:4])
            gaussians[..., 4:7] = torch.exp(gaussians[..., 4:7])
            if gaussians.shape[-1] == 14:
                gaussians[..., 11:] = 0.28209479177387814 * gaussians[..., 11:] + 0.5
        return gaussians


def tan_half_fov(fovy: float) -> float:
    return math.tan(0.5 * math.radians(fovy))
