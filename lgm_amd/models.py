"""LGM (core/models.py:14-174) on lgm_amd's modules: the UNet of lgm_amd/unet.py (fused GroupNorm+SiLU kernels,
MVAttention on the HIP attention kernels), the fused Gaussian head, and the GaussianRenderer with the MSE terms
computed inside the render kernels. Same submodule names (`unet`, `conv`), so reference checkpoints load unchanged.

LPIPS: the reference builds kiui's LPIPS(net='vgg') from downloaded weights. Here the weights come from the caller:
LGM(opt, lpips=...) takes a state_dict or a path to one (the native lgm_amd.lpips.LPIPS is built from it), an
lgm_amd.lpips.LPIPS, or any fn(gt, pred) -> per-image distances on [-1, 1] images; opt.lambda_lpips > 0 with nothing
passed is an error at construction. With the native module the loss term runs on its fused input and distance kernels
(LPIPS.loss_from_render); any other callable gets the reference's own lines.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .cameras import default_rays
from .gs import GaussianRenderer
from .head import gaussian_head
from .lpips import LPIPS
from .options import Options
from .unet import UNet


class LGM(nn.Module):
    def __init__(self, opt: Options, lpips=None):
        super().__init__()
        self.opt = opt
        self.unet = UNet(9, 14, down_channels=opt.down_channels, down_attention=opt.down_attention,
                         mid_attention=opt.mid_attention, up_channels=opt.up_channels, up_attention=opt.up_attention,
                         num_frames=opt.num_input_views)
        self.conv = nn.Conv2d(14, 14, kernel_size=1)  # core/models.py:34
        self.gs = GaussianRenderer(opt)
        if opt.lambda_lpips > 0:
            if lpips is None:
                raise ValueError("opt.lambda_lpips > 0 needs a perceptual network: pass LGM(opt, lpips=...) with LPIPS "
                                 "weights (a state_dict or a path: they are not part of this package), an "
                                 "lgm_amd.lpips.LPIPS, or fn(gt, pred) -> distances; or set lambda_lpips = 0")
            if isinstance(lpips, (str, os.PathLike, dict)):
                lpips = LPIPS(weights=lpips)
            self.lpips_loss = lpips
            if isinstance(lpips, nn.Module):
                lpips.requires_grad_(False)

    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        for k in list(sd.keys()):  # core/models.py:52-58
            if "lpips_loss" in k:
                del sd[k]
        return sd

    def prepare_default_rays(self, device, elevation=0):
        """core/models.py:61-85: the Pluecker embeddings [4, 6, h, w] of the four default input views."""
        return default_rays(self.opt.input_size, self.opt.fovy, self.opt.cam_radius, elevation, device=device)

    def forward_gaussians(self, images):
        """images [B, V, 9, H, W] -> Gaussians [B, V * splat_size^2, 14] (core/models.py:88-117)."""
        B, V, C, H, W = images.shape
        x = self.unet(images.reshape(B * V, C, H, W))
        return gaussian_head(x, self.conv, B, V)

    def forward(self, data, step_ratio=1):
        """core/models.py:120-174: data['input'] [B, V, 9, h, w], cam_view / cam_view_proj [B, Vo, 4, 4], cam_pos
        [B, Vo, 3], images_output [B, Vo, 3, S, S], masks_output [B, Vo, 1, S, S]."""
        gaussians = self.forward_gaussians(data["input"])
        if self.training:  # random background in training, white in eval
            bg_color = torch.rand(3, dtype=torch.float32, device=gaussians.device)
        else:
            bg_color = torch.ones(3, dtype=torch.float32, device=gaussians.device)
        gt_images, gt_masks = data["images_output"], data["masks_output"]
        # the two MSE terms of core/models.py:151-153 come from the render kernels (gt composited on bg_color there)
        out = self.gs.render(gaussians, data["cam_view"], data["cam_view_proj"], data["cam_pos"], bg_color=bg_color,
                             gt_images=gt_images, gt_masks=gt_masks)
        results = {"gaussians": gaussians, "images_pred": out["image"], "alphas_pred": out["alpha"]}
        loss = out["loss_mse"]
        if self.opt.lambda_lpips > 0:
            if isinstance(self.lpips_loss, LPIPS):  # composite, resize and distances on the fused kernels
                loss_lpips = self.lpips_loss.loss_from_render(gt_images, gt_masks, bg_color, out["image"]).mean()
            else:
                S = self.opt.output_size
                gt = gt_images * gt_masks + bg_color.view(1, 1, 3, 1, 1) * (1 - gt_masks)
                loss_lpips = self.lpips_loss(
                    F.interpolate(gt.reshape(-1, 3, S, S) * 2 - 1, (256, 256), mode="bilinear", align_corners=False),
                    F.interpolate(out["image"].reshape(-1, 3, S, S) * 2 - 1, (256, 256), mode="bilinear",
                                  align_corners=False)).mean()
            results["loss_lpips"] = loss_lpips
            loss = loss + self.opt.lambda_lpips * loss_lpips
        results["loss"] = loss
        results["psnr"] = out["psnr"]
        return results
