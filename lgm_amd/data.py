"""Training-batch assembly (core/provider_lvis.py:166-213 with core/utils.py get_rays, grid_distortion and
orbit_camera_jitter): from the decoded RGBA views and raw poses of a batch to the `data` dict LGM.forward reads.

A dataloader worker hands over the decoded **uint8 RGBA** views [B, V, Hs, Ws, 4] and the OpenGL poses c2w [B, V, 4, 4]
(translations already scaled, core/provider_lvis.py:139); `build_batch` does the rest. GPU tensors run the two C calls
of include/lgm_data.h (lgm_data_cameras, lgm_data_views); CPU tensors take a vectorised torch composition of the
provider's own lines (`build_batch_torch`, which also runs on GPU tensors: the comparison of the tests and of
scripts/bench_data.py). `get_rays`, `grid_distortion` and `orbit_camera_jitter` are drop-ins for core/utils.py: same
signatures, same draws from the global RNGs in the same order.

Random stream of `build_batch` (its own: the reference draws in per-worker streams that cannot be reproduced). All
draws come from one CPU torch.Generator (`generator`, None = torch's default CPU generator), in this order, and only
when training:
  1. torch.rand(B, 2): sample b is distorted if [b, 0] < opt.prob_grid_distortion and jittered if
     [b, 1] < opt.prob_cam_jitter;
  2. for every distorted sample in order: torch.randint(8, 17, (1,)) knots, then torch.rand(Vi - 1, 2, n) (per input
     view 1 .. Vi - 1: the x row, the y row) perturbing them as grid_distortion does;
  3. torch.rand(B, Vi, 2) * 2 - 1: the jitter numbers (u0, u1) of every input view (used for views >= 1 of jittered
     samples).
View 0 is never distorted or jittered. `draw_augmentation` makes the draws; `build_batch(..., augmentation=...)` takes
them ready-made (how the tests replay the reference's draws).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _native as nat
from ._native import ptr
from .cameras import projection_matrix
from .options import Options

MAX_KNOTS = 17  # include/lgm_data.h LGM_DATA_MAX_KNOTS
SWAP_RB, NO_NORMALIZE = 1, 2  # include/lgm_data.h
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# ---------------------------------------------------------------- knots (the host half of grid_distortion)

def _knots_from_uniform(r: torch.Tensor, size: int, strength: float) -> torch.Tensor:
    """r [..., n] uniform in [0, 1) -> the integer knots of core/utils.py:77-81 along an axis of `size` pixels."""
    n = r.shape[-1]
    steps = torch.linspace(0, 1, n)
    steps = (steps + strength * (r - 0.5) / (n - 1)).clamp(0, 1)
    k = (steps * size).long()
    k[..., 0] = 0
    k[..., -1] = size
    return k


def _pack_knots(kx: torch.Tensor, ky: torch.Tensor) -> torch.Tensor:
    """kx, ky [N, n] -> int32 [N, 2, 17] (row 0 x, row 1 y; entries past n repeat the last knot)."""
    N, n = kx.shape
    out = torch.empty(N, 2, MAX_KNOTS, dtype=torch.int32)
    out[:, 0, :n], out[:, 1, :n] = kx, ky
    out[:, 0, n:], out[:, 1, n:] = kx[:, -1:], ky[:, -1:]
    return out


def sample_grid_knots(n: int, H: int, W: int, strength: float = 0.5):
    """The random half of grid_distortion (core/utils.py:70-91) for n images of H x W: draws np.random.randint(8, 17)
    once, then per image torch.rand_like for x and then for y, exactly as the reference consumes the global RNGs.
    Returns (knots int32 [n, 2, 17]: row 0 the x knots, row 1 the y knots; the knot count)."""
    num_steps = int(np.random.randint(8, 17))
    kx, ky = [], []
    for _ in range(n):
        kx.append(_knots_from_uniform(torch.rand(num_steps), W, strength))
        ky.append(_knots_from_uniform(torch.rand(num_steps), H, strength))
    return _pack_knots(torch.stack(kx), torch.stack(ky)), num_steps


def knot_coords(k: torch.Tensor, n: int, size: int) -> torch.Tensor:
    """k [N, >= n] integer knots -> the grid coordinate in [-1, 1] of every destination index, float64 [N, size]
    (include/lgm_data.h: index j lies in segment i, k[i] <= j < k[i + 1])."""
    k = k[:, :n].long().contiguous()
    j = torch.arange(size, device=k.device).expand(k.shape[0], size).contiguous()
    i = (torch.searchsorted(k, j, right=True) - 1).clamp(0, n - 2)
    k0, k1 = k.gather(1, i), k.gather(1, i + 1)
    g0 = -1.0 + 2.0 * i.double() / (n - 1)
    g1 = -1.0 + 2.0 * (i + 1).double() / (n - 1)
    return g0 + (g1 - g0) * (j - k0).double() / (k1 - k0 - 1).clamp_min(1).double()


def _warp_torch(images: torch.Tensor, knots: torch.Tensor, n: int) -> torch.Tensor:
    """F.grid_sample of images [N, C, H, W] under the knots [N, 2, 17] (count n)."""
    N, _, H, W = images.shape
    knots = knots.to(images.device)
    xs = knot_coords(knots[:, 0], n, W).to(images.dtype)
    ys = knot_coords(knots[:, 1], n, H).to(images.dtype)
    grid = torch.stack([xs[:, None, :].expand(N, H, W), ys[:, :, None].expand(N, H, W)], -1)
    return F.grid_sample(images, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


# ---------------------------------------------------------------- the two C calls

def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def data_cameras(c2w: torch.Tensor, Vi: int, jitter: Optional[torch.Tensor], jitter_strength: float, cam_radius: float,
                 fovy: float, znear: float, zfar: float):
    """lgm_data_cameras on GPU tensors: c2w [B, V, 4, 4], jitter [B, Vi, 2] or None -> (pose_in [B, Vi, 4, 4],
    cam_view, cam_view_proj [B, V, 4, 4], cam_pos [B, V, 3], c2w_colmap [B, Vi, 4, 4])."""
    nat.require_device_tensor(c2w, "c2w")
    c2w = _f32c(c2w)
    B, V = c2w.shape[:2]
    dev = c2w.device
    if jitter is not None:
        jitter = _f32c(jitter.to(dev))
        assert jitter.shape == (B, Vi, 2), jitter.shape
    pose_in = torch.empty(B, Vi, 4, 4, device=dev)
    cam_view, cam_view_proj = torch.empty(B, V, 4, 4, device=dev), torch.empty(B, V, 4, 4, device=dev)
    cam_pos, colmap = torch.empty(B, V, 3, device=dev), torch.empty(B, Vi, 4, 4, device=dev)
    with torch.cuda.device(dev):
        nat.call("lgm_data_cameras", dev, B, V, Vi, ptr(c2w), ptr(jitter), float(jitter_strength), float(cam_radius),
                 float(fovy), float(znear), float(zfar), ptr(pose_in), ptr(cam_view), ptr(cam_view_proj), ptr(cam_pos),
                 ptr(colmap))
    return pose_in, cam_view, cam_view_proj, cam_pos, colmap


def data_views(src: torch.Tensor, pose_in: Optional[torch.Tensor], knots: Optional[torch.Tensor],
               nknots: Optional[torch.Tensor], fovy: float, Vi: int, h: int, So: int, swap_rb: bool = False,
               normalize: bool = True, want_input: bool = True, want_output: bool = True):
    """lgm_data_views on GPU tensors: src [B, V, Hs, Ws, 4] uint8 or float32, pose_in [B, Vi, 4, 4], knots int32
    [B, Vi, 2, 17] (any device) with nknots int32 [B, Vi] (host) or None -> (input [B, Vi, 9, h, h], images_output
    [B, V, 3, So, So], masks_output [B, V, 1, So, So]); a part not wanted is None."""
    nat.require_device_tensor(src, "src")
    if src.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"src must be uint8 or float32, got {src.dtype}")
    src = src.contiguous()
    B, V, Hs, Ws, four = src.shape
    assert four == 4, src.shape
    dev = src.device
    inp = torch.empty(B, Vi, 9, h, h, device=dev) if want_input else None
    img = torch.empty(B, V, 3, So, So, device=dev) if want_output else None
    msk = torch.empty(B, V, 1, So, So, device=dev) if want_output else None
    if knots is not None:
        knots = knots.to(dev, torch.int32).contiguous()
        nknots = nknots.to("cpu", torch.int32).contiguous()
        assert knots.shape == (B, Vi, 2, MAX_KNOTS) and nknots.shape == (B, Vi), (knots.shape, nknots.shape)
    if want_input:
        pose_in = _f32c(pose_in.to(dev))
        assert pose_in.shape == (B, Vi, 4, 4), pose_in.shape
    flags = (SWAP_RB if swap_rb else 0) | (0 if normalize else NO_NORMALIZE)
    with torch.cuda.device(dev):
        # (nknots is a host array: the one pointer here that is not a device address)
        nat.call("lgm_data_views", dev, nat.DATA_U8 if src.dtype == torch.uint8 else 0, flags, B, V, Vi, Hs, Ws, h, So,
                 ptr(src), ptr(pose_in) if want_input else None, ptr(knots), ptr(nknots) if knots is not None else None,
                 float(fovy), ptr(inp), ptr(img), ptr(msk))
    return inp, img, msk


# ---------------------------------------------------------------- rays

def plucker_rays(poses: torch.Tensor, h: int, fovy: float) -> torch.Tensor:
    """The Pluecker embeddings (o x d, d) [N, 6, h, h] of get_rays(pose, h, h, fovy) for poses [N, 4, 4] (OpenGL c2w;
    core/provider_lvis.py:190-196). GPU tensors run lgm_data_views."""
    poses = poses.reshape(-1, 4, 4).to(torch.float32)
    N = poses.shape[0]
    if poses.is_cuda:
        src = torch.zeros(N, 1, 1, 1, 4, dtype=torch.uint8, device=poses.device)  # (the image planes are not kept)
        inp, _, _ = data_views(src, poses[:, None], None, None, fovy, 1, h, 1, want_output=False)
        return inp[:, 0, 3:9].contiguous()
    focal = h * 0.5 / np.tan(0.5 * np.deg2rad(fovy))
    px = torch.arange(h, dtype=torch.float32)
    dx = ((px - h * 0.5 + 0.5) / focal)[None, None, :].expand(N, h, h)
    dy = (-(px - h * 0.5 + 0.5) / focal)[None, :, None].expand(N, h, h)
    dirs = torch.stack([dx, dy, -torch.ones_like(dx)], -1)  # [N, h, h, 3]
    d = torch.einsum("nyxj,nij->nyxi", dirs, poses[:, :3, :3])
    d = d / torch.sqrt(torch.clamp((d * d).sum(-1, keepdim=True), min=1e-20))
    o = poses[:, None, None, :3, 3].expand_as(d)
    return torch.cat([torch.cross(o, d, dim=-1), d], -1).permute(0, 3, 1, 2).contiguous()


def get_rays(pose: torch.Tensor, h: int, w: int, fovy: float, opengl: bool = True):
    """core/utils.py:10-43: ray origins and unit directions [h, w, 3] of one c2w pose [4, 4]. A GPU pose with h == w
    (OpenGL) runs the kernel; anything else takes cameras.get_rays' torch lines."""
    if pose.is_cuda and h == w and opengl:
        d = plucker_rays(pose[None], h, fovy)[0, 3:6].permute(1, 2, 0).contiguous()
        return pose[:3, 3].to(torch.float32).expand(h, w, 3), d
    from .cameras import get_rays as rays_torch
    return rays_torch(pose, h, w, fovy, opengl)


# ---------------------------------------------------------------- the two augmentations (drop-ins)

def grid_distortion(images: torch.Tensor, strength: float = 0.5) -> torch.Tensor:
    """core/utils.py:63-108: images [B, C, H, W] warped by a random piecewise-linear grid. GPU float32 images with
    C == 3 and H == W run lgm_data_views (other GPU shapes are an error: there is no kernel for them); CPU tensors take
    one vectorised grid_sample."""
    B, C, H, W = images.shape
    knots, n = sample_grid_knots(B, H, W, strength)
    if not images.is_cuda:
        return _warp_torch(images, knots, n)
    if C != 3 or H != W or images.dtype != torch.float32:
        raise nat.NativeError(f"grid_distortion on the GPU takes float32 [B, 3, h, h] images, got "
                              f"{tuple(images.shape)} {images.dtype}")
    src = torch.cat([images.permute(0, 2, 3, 1), images.new_ones(B, H, W, 1)], -1)[:, None]  # opaque RGBA texels
    pose = images.new_zeros(B, 1, 4, 4)
    inp, _, _ = data_views(src, pose, knots[:, None], torch.full((B, 1), n, dtype=torch.int32), 60.0, 1, H, 1,
                           normalize=False, want_output=False)
    return inp[:, 0, :3].contiguous()


def _rodrigues64(r: torch.Tensor) -> torch.Tensor:
    """r [N, 3] float64 -> rotation matrices [N, 3, 3]: I + sinc(t) K + sinc(t / 2)^2 / 2 K^2 (exactly I at r = 0)."""
    th = r.norm(dim=-1)
    a = torch.sinc(th / math.pi)[:, None, None]
    b = (0.5 * torch.sinc(0.5 * th / math.pi) ** 2)[:, None, None]
    K = torch.zeros(r.shape[0], 3, 3, dtype=r.dtype, device=r.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -r[:, 2], r[:, 1], r[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -r[:, 0], -r[:, 1], r[:, 0]
    return torch.eye(3, dtype=r.dtype, device=r.device) + a * K + b * (K @ K)


def _jitter_torch(poses: torch.Tensor, u: torch.Tensor, strength: float) -> torch.Tensor:
    """poses [N, 4, 4] float32, u [N, 2] in [-1, 1) -> jittered poses (include/lgm_data.h, in float64, rounded once;
    the last row is written as (0, 0, 0, 1))."""
    P, u = poses.double(), u.double()
    rx = P[:, :3, 1] * (strength * math.pi) * u[:, 0:1]
    ry = P[:, :3, 0] * (strength * math.pi / 2) * u[:, 1:2]
    rot = _rodrigues64(rx) @ _rodrigues64(ry)
    out = torch.zeros_like(P)
    out[:, :3, :3] = rot @ P[:, :3, :3]
    out[:, :3, 3:] = rot @ P[:, :3, 3:]
    out[:, 3, 3] = 1.0
    return out.float()


def orbit_camera_jitter(poses: torch.Tensor, strength: float = 0.1) -> torch.Tensor:
    """core/utils.py:45-61: poses [B, 4, 4] (OpenGL orbit cameras) under a random orbital rotation; draws
    torch.rand(B, 1) twice on the poses' device, as the reference does. GPU poses run lgm_data_cameras."""
    B = poses.shape[0]
    u = torch.cat([torch.rand(B, 1, device=poses.device) * 2 - 1, torch.rand(B, 1, device=poses.device) * 2 - 1], 1)
    if not poses.is_cuda:
        return _jitter_torch(poses.float(), u, strength).to(poses.dtype)
    # identity first pose and radius 0: the normalisation returns the poses as they are (include/lgm_data.h)
    c2w = torch.cat([torch.eye(4, device=poses.device)[None], poses.float()], 0)[None]
    jit = torch.cat([u.new_zeros(1, 2), u], 0)[None]
    pose_in = data_cameras(c2w, B + 1, jit, strength, 0.0, 60.0, 0.5, 2.5)[0]
    return pose_in[0, 1:].to(poses.dtype)


# ---------------------------------------------------------------- the batch

@dataclass
class Augmentation:
    """The random decisions of one batch (CPU tensors): knots int32 [B, Vi, 2, 17] with their counts nknots int32
    [B, Vi] (0: the view is not distorted), and the jitter numbers float32 [B, Vi, 2] in [-1, 1) ((0, 0): none)."""
    knots: torch.Tensor
    nknots: torch.Tensor
    jitter: torch.Tensor


def draw_augmentation(opt: Options, B: int, generator: Optional[torch.Generator] = None,
                      grid_strength: float = 0.5) -> Augmentation:
    """The draws of build_batch, in the order the module docstring lists."""
    Vi, h = opt.num_input_views, opt.input_size
    knots = torch.zeros(B, Vi, 2, MAX_KNOTS, dtype=torch.int32)
    nknots = torch.zeros(B, Vi, dtype=torch.int32)
    decide = torch.rand(B, 2, generator=generator)
    for b in range(B):
        if Vi > 1 and float(decide[b, 0]) < opt.prob_grid_distortion:
            n = int(torch.randint(8, 17, (1,), generator=generator))
            r = torch.rand(Vi - 1, 2, n, generator=generator)
            knots[b, 1:] = _pack_knots(_knots_from_uniform(r[:, 0], h, grid_strength),
                                       _knots_from_uniform(r[:, 1], h, grid_strength))
            nknots[b, 1:] = n
    jitter = torch.rand(B, Vi, 2, generator=generator) * 2 - 1
    jitter[:, 0] = 0
    jitter[decide[:, 1] >= opt.prob_cam_jitter] = 0
    return Augmentation(knots, nknots, jitter)


def cameras_torch(c2w: torch.Tensor, Vi: int, jitter: Optional[torch.Tensor], jitter_strength: float,
                  cam_radius: float, fovy: float, znear: float, zfar: float):
    """The provider's camera lines (core/provider_lvis.py:166-171, 200-213) in torch on c2w's device: float32 with
    torch.inverse, as the reference runs them (the jitter as _jitter_torch). Same returns as data_cameras."""
    c2w = c2w.float()
    B, V = c2w.shape[:2]
    T = torch.eye(4, device=c2w.device)
    T[2, 3] = cam_radius
    P = (T @ torch.inverse(c2w[:, 0]))[:, None] @ c2w
    pose_in = P[:, :Vi].clone()
    if jitter is not None:
        pose_in = _jitter_torch(pose_in.reshape(-1, 4, 4), jitter.to(c2w.device).reshape(-1, 2),
                                jitter_strength).reshape(B, Vi, 4, 4)
    P = P.clone()
    P[:, :, :3, 1:3] *= -1
    cam_view = torch.inverse(P).transpose(2, 3)
    cam_view_proj = cam_view @ projection_matrix(fovy, znear, zfar).to(c2w.device)
    return pose_in, cam_view, cam_view_proj, -P[:, :, :3, 3], P[:, :Vi].clone()


def views_torch(rgba: torch.Tensor, pose_in: torch.Tensor, knots: Optional[torch.Tensor],
                nknots: Optional[torch.Tensor], fovy: float, Vi: int, h: int, So: int, swap_rb: bool = False):
    """The provider's image and ray lines (core/provider_lvis.py:141-198) as torch ops on rgba's device: what
    lgm_data_views replaces. Same arguments and returns as data_views."""
    B, V = rgba.shape[:2]
    x = rgba.float() / 255 if rgba.dtype == torch.uint8 else rgba.float()
    x = x.permute(0, 1, 4, 2, 3)  # [B, V, 4, Hs, Ws]
    mask = x[:, :, 3:4]
    img = x[:, :, :3] * mask + (1 - mask)
    if swap_rb:
        img = img[:, :, [2, 1, 0]]
    Hs, Ws = img.shape[-2:]
    img_in = F.interpolate(img[:, :Vi].reshape(B * Vi, 3, Hs, Ws), size=(h, h), mode="bilinear", align_corners=False)
    if knots is not None:
        nk = nknots.reshape(-1).cpu()
        kn = knots.reshape(-1, 2, MAX_KNOTS).cpu()
        for n in sorted(set(nk.tolist()) - {0}):
            sel = (nk == n).nonzero()[:, 0].to(img_in.device)
            img_in[sel] = _warp_torch(img_in[sel], kn[nk == n], n)
    mean = torch.tensor(IMAGENET_MEAN, device=img.device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=img.device).view(1, 3, 1, 1)
    img_in = (img_in - mean) / std
    pose_in = pose_in.to(img.device).float()
    if pose_in.is_cuda:  # (plucker_rays would take the kernel: this function is the torch composition)
        from .cameras import get_rays as rays_torch
        rays = []
        for p in pose_in.reshape(-1, 4, 4):
            o, d = rays_torch(p, h, h, fovy)
            rays.append(torch.cat([torch.cross(o, d, dim=-1), d], -1))
        rays = torch.stack(rays).permute(0, 3, 1, 2)
    else:
        rays = plucker_rays(pose_in, h, fovy)
    inp = torch.cat([img_in, rays], 1).reshape(B, Vi, 9, h, h)
    img_out = F.interpolate(img.reshape(B * V, 3, Hs, Ws), size=(So, So), mode="bilinear", align_corners=False)
    msk_out = F.interpolate(mask.reshape(B * V, 1, Hs, Ws), size=(So, So), mode="bilinear", align_corners=False)
    return inp, img_out.reshape(B, V, 3, So, So), msk_out.reshape(B, V, 1, So, So)


def build_batch_torch(opt: Options, rgba: torch.Tensor, c2w: torch.Tensor, aug: Optional[Augmentation] = None,
                      swap_rb: bool = False, jitter_strength: float = 0.1) -> dict:
    """The provider's tail as torch ops on the tensors' device (CPU or GPU): the composition build_batch's kernels
    replace. aug None: no augmentation."""
    Vi = opt.num_input_views
    pose_in, cam_view, cam_view_proj, cam_pos, colmap = cameras_torch(
        c2w.to(rgba.device), Vi, aug.jitter if aug is not None else None, jitter_strength, opt.cam_radius, opt.fovy,
        opt.znear, opt.zfar)
    inp, img, msk = views_torch(rgba, pose_in, aug.knots if aug is not None else None,
                                aug.nknots if aug is not None else None, opt.fovy, Vi, opt.input_size,
                                opt.output_size, swap_rb)
    return {"input": inp, "images_output": img, "masks_output": msk, "cam_view": cam_view,
            "cam_view_proj": cam_view_proj, "cam_pos": cam_pos, "c2w_colmap": colmap}


def build_batch(opt: Options, rgba: torch.Tensor, c2w: torch.Tensor, training: bool,
                generator: Optional[torch.Generator] = None, *, augmentation: Optional[Augmentation] = None,
                swap_rb: bool = False, jitter_strength: float = 0.1) -> dict:
    """rgba [B, V, Hs, Ws, 4] (uint8 as decoded, or float32 in [0, 1]; swap_rb: BGRA as cv2 delivers) and c2w
    [B, V, 4, 4] (OpenGL, translations scaled) -> the `data` dict of LGM.forward: input [B, Vi, 9, h, h],
    images_output [B, V, 3, So, So], masks_output [B, V, 1, So, So], cam_view, cam_view_proj [B, V, 4, 4], cam_pos
    [B, V, 3], plus c2w_colmap [B, Vi, 4, 4]; V >= opt.num_input_views = Vi, h = opt.input_size, So = opt.output_size.
    training: the augmentations are drawn (module docstring) or taken from `augmentation`; otherwise nothing random
    is applied. GPU tensors run the kernels, CPU tensors build_batch_torch."""
    B, V = rgba.shape[:2]
    Vi = opt.num_input_views
    if c2w.shape != (B, V, 4, 4) or V < Vi or rgba.shape[-1] != 4:
        raise ValueError(f"rgba {tuple(rgba.shape)} / c2w {tuple(c2w.shape)}: want [B, V, Hs, Ws, 4] and [B, V, 4, 4] "
                         f"with V >= {Vi}")
    aug = None
    if training:
        aug = augmentation if augmentation is not None else draw_augmentation(opt, B, generator)
    if not rgba.is_cuda:
        return build_batch_torch(opt, rgba, c2w, aug, swap_rb, jitter_strength)
    c2w = c2w.to(rgba.device)
    pose_in, cam_view, cam_view_proj, cam_pos, colmap = data_cameras(
        c2w, Vi, aug.jitter if aug is not None else None, jitter_strength, opt.cam_radius, opt.fovy, opt.znear,
        opt.zfar)
    distorted = aug is not None and bool(aug.nknots.any())
    inp, img, msk = data_views(rgba, pose_in, aug.knots if distorted else None, aug.nknots if distorted else None,
                               opt.fovy, Vi, opt.input_size, opt.output_size, swap_rb=swap_rb)
    return {"input": inp, "images_output": img, "masks_output": msk, "cam_view": cam_view,
            "cam_view_proj": cam_view_proj, "cam_pos": cam_pos, "c2w_colmap": colmap}
