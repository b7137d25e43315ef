"""LPIPS (VGG16) perceptual loss, the `lambda_lpips` term of LGM's training loss (core/models.py:46-49, :156-165:
kiui's LPIPS(net='vgg')), on the fused HIP distance and input kernels (include/lgm_lpips.h, lgm_amd/csrc/lpips.hip).

The thirteen 3x3 convolutions of the VGG16 trunk (with their ReLUs and four 2x2 max-pools) are torch ops. What the
kernels take is the elementwise traffic around them: per tap (after relu1_2, 2_2, 3_3, 4_3, 5_3) the channel-normalise
-> subtract -> square -> 1x1 head -> spatial mean chain, one pass per direction, and the composite -> bilinear resize ->
scaling-layer chain on the way in (`loss_from_render`). `fused` (a property, default True) switches both; fused = False
is the plain torch composition, which is also the CPU path and what runs for any dtype or device the kernels do not take.

Weights are not part of this package. `weights` is a state_dict, a path to one (torch.load), or a list of those
(merged), under these key spellings:
  * torchvision's VGG16 trunk: `features.{i}.weight|bias`, i in 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28;
  * the lpips package's heads: `lin{k}.model.1.weight` [1, C, 1, 1], k in 0..4 (`lins.{k}.model.1.weight` is taken as
    the same tensor);
  * a whole lpips module: `net.slice{s}.{i}.weight|bias` + `lin{k}.model.1.weight` + `scaling_layer.shift|scale`.
These names were written from memory of the published packages: neither torchvision nor lpips was at hand to check
them against, so the loaders are tested against synthetic dicts that use these names. Loading is strict: every trunk and
head tensor must be present and an unknown key raises. weights = None gives a random trunk and random non-negative
heads, with a warning: for tests and timing only.
"""
from __future__ import annotations

import os
import re
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from ._native import ptr
from .attention import _autocast_dtype

# Deprecated and unused in this package: the name under which the GPU tests of earlier revisions import the table.
# New code and new tests say nat.DTYPE_CODES.
_DTYPES = nat.DTYPE_CODES

# torchvision's vgg16().features: (index, in, out) of the convolutions; a ReLU follows each; max-pools at POOLS
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
POOLS = (4, 9, 16, 23)
TAPS = (3, 8, 15, 22, 29)  # the ReLUs after conv1_2, 2_2, 3_3, 4_3, 5_3
CHANNELS = (64, 128, 256, 512, 512)
SLICE_STARTS = (0, 4, 9, 16, 23, 30)  # lpips's net.slice{s} holds features[SLICE_STARTS[s-1]:SLICE_STARTS[s]]
SHIFT = (-.030, -.088, -.188)  # lpips's ScalingLayer
SCALE = (.458, .448, .450)
_GRID_MAX = 2 ** 31 - 1


class VGG16Features(nn.Module):
    """VGG16's convolutional trunk up to relu5_3 with torchvision's module indices (`features.{i}`); forward returns
    the five LPIPS taps [N, 64, H, W], [N, 128, H/2, W/2], [N, 256, H/4, W/4], [N, 512, H/8, W/8], [N, 512, H/16, W/16]."""

    def __init__(self):
        super().__init__()
        layers = [None] * (TAPS[-1] + 1)
        for i, cin, cout in CONVS:
            layers[i] = nn.Conv2d(cin, cout, kernel_size=3, padding=1)
            layers[i + 1] = nn.ReLU(inplace=False)
        for i in POOLS:
            layers[i] = nn.MaxPool2d(kernel_size=2, stride=2)
        self.features = nn.Sequential(*layers)

    def forward(self, x):
        taps = []
        for i, m in enumerate(self.features):
            x = m(x)
            if i in TAPS:
                taps.append(x)
        return taps


def convert_state_dict(sd) -> dict:
    """A state_dict in any of the spellings of the module docstring -> this module's own keys
    (`net.features.{i}.weight|bias`, `lins.{k}` [C], `shift`, `scale` [3]). Unknown keys raise KeyError."""
    out = {}
    for k, v in sd.items():
        m = re.fullmatch(r"features\.(\d+)\.(weight|bias)", k)
        if m:
            out[f"net.features.{m.group(1)}.{m.group(2)}"] = v
            continue
        m = re.fullmatch(r"net\.slice(\d)\.(\d+)\.(weight|bias)", k)
        if m:
            s, i = int(m.group(1)), int(m.group(2))
            if not (1 <= s <= 5 and SLICE_STARTS[s - 1] <= i < SLICE_STARTS[s]):
                raise KeyError(f"LPIPS weights: {k!r}: layer {i} is not in slice {s}")
            out[f"net.features.{i}.{m.group(3)}"] = v
            continue
        m = re.fullmatch(r"lins?\.?(\d)\.model\.1\.weight", k)
        if m and (k.startswith("lins.") or k.startswith("lin" + m.group(1))):
            kk = int(m.group(1))
            if kk >= len(CHANNELS) or tuple(v.shape) != (1, CHANNELS[kk], 1, 1):
                raise KeyError(f"LPIPS weights: {k!r} must be [1, C, 1, 1] of a VGG16 tap, got {tuple(v.shape)}")
            out.setdefault(f"lins.{kk}", v.reshape(-1))
            continue
        m = re.fullmatch(r"scaling_layer\.(shift|scale)", k)
        if m:
            if v.numel() != 3:
                raise KeyError(f"LPIPS weights: {k!r} must have 3 elements, got {tuple(v.shape)}")
            out[m.group(1)] = v.reshape(3)
            continue
        raise KeyError(f"LPIPS weights: unexpected key {k!r}")
    return out


def _load_source(src) -> dict:
    if isinstance(src, (str, os.PathLike)):
        src = torch.load(src, map_location="cpu", weights_only=True)
    if isinstance(src, (list, tuple)):
        merged = {}
        for s in src:
            merged.update(_load_source(s))
        return merged
    if not hasattr(src, "items"):
        raise TypeError(f"LPIPS weights: a path, a state_dict or a list of those, got {type(src).__name__}")
    return dict(src)


def _torch_distance(f0, f1, w, eps):
    """lpips's normalize_tensor -> (difference)^2 -> 1x1 conv -> spatial mean, as torch ops: [N]."""
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + eps)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + eps)
    return F.conv2d((n0 - n1) ** 2, w.view(1, -1, 1, 1)).mean(dim=(2, 3)).reshape(-1)


class _LpipsDist(torch.autograd.Function):
    """lgm_lpips_dist_forward / _backward (the dtypes are _dist_takes' to check)."""

    @staticmethod
    def forward(ctx, f0, f1, w, eps: float):
        N, C, H, W = f0.shape
        f0, f1 = f0.contiguous(), f1.contiguous()
        w = w.detach().float().contiguous()
        dev = f0.device
        need0, need1 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        out = torch.empty(N, device=dev, dtype=torch.float32)
        norms = torch.empty((2, N, H, W), device=dev, dtype=torch.float32) if need0 or need1 else None
        ws, ws_bytes = nat.workspace("lgm_lpips_dist_workspace_size", dev, N, C, H, W, min_bytes=0)
        np_ = ptr(norms)
        nat.call("lgm_lpips_dist_forward", dev, nat.DTYPE_CODES[f0.dtype], nat.DTYPE_CODES[f1.dtype], N, C, H, W, eps,
                 ptr(f0), ptr(f1), ptr(w), ptr(out), np_, None if np_ is None else np_ + 4 * N * H * W, ptr(ws),
                 ws_bytes)
        if norms is not None:
            ctx.save_for_backward(f0, f1, w, norms)
            ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, g):
        f0, f1, w, norms = ctx.saved_tensors
        N, C, H, W = f0.shape
        need0, need1 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g.float().contiguous()
        df0 = torch.empty_like(f0) if need0 else None
        df1 = torch.empty_like(f1) if need1 else None
        code = nat.DTYPE_CODES[f0.dtype]
        np_ = ptr(norms)
        nat.call("lgm_lpips_dist_backward", f0.device, code, code, N, C, H, W, ctx.eps, ptr(f0), ptr(f1), ptr(w), np_,
                 np_ + 4 * N * H * W, ptr(g), ptr(df0), ptr(df1))
        return df0, df1, None, None


class _LpipsPrep(torch.autograd.Function):
    """lgm_lpips_prep_forward / _backward: (pred, gt, mask, bg) -> VGG-ready (x_pred, x_gt) [M, 3, R, R]."""

    @staticmethod
    def forward(ctx, pred, gt, mask, bg, R: int, dtype):
        M, _, S, _ = pred.shape
        pred = pred.float().contiguous()
        gt, mask, bg = gt.float().contiguous(), mask.float().contiguous(), bg.float().contiguous()
        xp = torch.empty((M, 3, R, R), device=pred.device, dtype=dtype)
        xg = torch.empty_like(xp)
        nat.call("lgm_lpips_prep_forward", pred.device, nat.DTYPE_CODES[dtype], M, S, R, ptr(pred), ptr(gt),
                 ptr(mask), ptr(bg), ptr(xp), ptr(xg))
        ctx.meta = (M, S, R, dtype)
        ctx.mark_non_differentiable(xg)
        return xp, xg

    @staticmethod
    def backward(ctx, d_xp, _d_xg):
        M, S, R, dtype = ctx.meta
        d_xp = d_xp.to(dtype).contiguous()
        d_pred = torch.empty((M, 3, S, S), device=d_xp.device, dtype=torch.float32)
        nat.call("lgm_lpips_prep_backward", d_xp.device, nat.DTYPE_CODES[dtype], M, S, R, ptr(d_xp), ptr(d_pred))
        return d_pred, None, None, None, None, None


def _dist_takes(f0, f1, w) -> bool:
    """What lgm_lpips_dist_* accepts (include/lgm_lpips.h); everything else is torch's."""
    if not (f0.is_cuda and f1.device == f0.device and w.device == f0.device) or f0.dim() != 4 or f0.shape != f1.shape:
        return False
    if f0.dtype not in nat.DTYPE_CODES or f1.dtype != f0.dtype or w.dtype not in nat.DTYPE_CODES or f0.numel() == 0:
        return False
    if w.requires_grad and torch.is_grad_enabled():  # trainable heads: the kernels return no gradient for them
        return False
    N, C, H, W = f0.shape
    return w.numel() == C and N * (-(-H * W // 16)) <= _GRID_MAX and f0.numel() < 2 ** 60


def lpips_distance(f0, f1, w, eps: float = 1e-10, fused: bool = True):
    """(1 / HW) sum_p sum_c w_c (f0 / (|f0|_p + eps) - f1 / (|f1|_p + eps))^2 of two feature maps [N, C, H, W] -> [N].
    GPU float32 / bfloat16 / float16 maps of one dtype run one HIP pass per direction (fp32 result); anything else, and
    fused = False, is the torch composition."""
    if fused and _dist_takes(f0, f1, w):
        return _LpipsDist.apply(f0, f1, w, eps)
    return _torch_distance(f0, f1, w, eps)


class LPIPS(nn.Module):
    """LPIPS(net='vgg') of the lpips / kiui packages. forward(in0, in1) takes two [N, 3, H, W] images in [-1, 1] and
    returns their distances [N, 1, 1, 1] (the contract LGM.forward calls). Frozen (no parameter requires a gradient)
    and in eval mode by default; the trunk runs under no_grad on an input that needs no gradient. `size` is the side the
    inputs of `loss_from_render` are resized to (the reference: 256)."""

    def __init__(self, weights=None, size: int = 256, eps: float = 1e-10):
        super().__init__()
        self.size = int(size)
        self.eps = float(eps)
        self._fused = True
        self.net = VGG16Features()
        self.lins = nn.ParameterList([nn.Parameter(torch.rand(c) / c) for c in CHANNELS])
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32))
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32))
        self._published_scaling = True  # the input kernel has the published shift / scale built in
        if weights is None:
            warnings.warn("LPIPS(weights=None): random VGG16 trunk and heads -- distances mean nothing; for tests and "
                          "timing only", stacklevel=2)
        else:
            sd = convert_state_dict(_load_source(weights))
            for name, ref in (("shift", SHIFT), ("scale", SCALE)):
                if name in sd:
                    self._published_scaling &= bool(torch.equal(sd[name].detach().float().cpu(),
                                                                torch.tensor(ref, dtype=torch.float32)))
                else:
                    sd[name] = getattr(self, name)
            self.load_state_dict(sd, strict=True)
        self.requires_grad_(False)
        self.eval()

    @property
    def fused(self) -> bool:
        return self._fused

    @fused.setter
    def fused(self, value: bool):
        self._fused = bool(value)

    def _features(self, x):
        need = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.net.parameters()))
        with torch.set_grad_enabled(need):
            return self.net(x)

    def _distance(self, x0, x1):
        """Distances [N, 1, 1, 1] of two inputs that already went through the scaling layer."""
        total = None
        for f0, f1, w in zip(self._features(x0), self._features(x1), self.lins):
            d = lpips_distance(f0, f1, w, self.eps, self._fused)
            total = d if total is None else total + d
        return total.view(-1, 1, 1, 1)

    def forward(self, in0, in1):
        shift, scale = self.shift.view(1, 3, 1, 1), self.scale.view(1, 3, 1, 1)
        return self._distance((in0 - shift) / scale, (in1 - shift) / scale)

    def _prep_takes(self, pred, gt, mask, bg) -> bool:
        if not (self._fused and self._published_scaling and pred.is_cuda and pred.dim() == 4):
            return False
        M, C, S, S2 = pred.shape
        if C != 3 or S != S2 or M == 0 or gt.shape != pred.shape or mask.shape != (M, 1, S, S) or bg.numel() != 3:
            return False
        if any(t.device != pred.device or t.dtype not in nat.DTYPE_CODES for t in (pred, gt, mask, bg)):
            return False
        if torch.is_grad_enabled() and (gt.requires_grad or mask.requires_grad or bg.requires_grad):
            return False  # the input kernel differentiates with respect to pred only
        return max(S, self.size) <= 32768 and M * max(S, self.size) ** 2 // 256 < _GRID_MAX

    def loss_from_render(self, gt_images, gt_masks, bg_color, pred_images):
        """core/models.py:156-165 from the renderer's tensors: gt_images, pred_images [..., 3, S, S] in [0, 1],
        gt_masks [..., 1, S, S], bg_color [3]. The ground truth is composited on bg_color, both are resized to
        size x size (bilinear, align_corners = False) and mapped to LPIPS's input range; returns the per-image
        distances [M, 1, 1, 1] (gt first: it is the side without a gradient)."""
        S = pred_images.shape[-1]
        pred, gt = pred_images.reshape(-1, 3, S, S), gt_images.reshape(-1, 3, S, S)
        mask = gt_masks.reshape(-1, 1, S, S)
        if self._prep_takes(pred, gt, mask, bg_color):
            ac = _autocast_dtype("cuda")
            x_pred, x_gt = _LpipsPrep.apply(pred, gt, mask, bg_color, self.size,
                                            ac if ac in nat.DTYPE_CODES else torch.float32)
            return self._distance(x_gt, x_pred)
        gt = gt * mask + bg_color.view(1, 3, 1, 1) * (1 - mask)
        R = (self.size, self.size)
        return self(F.interpolate(gt * 2 - 1, R, mode="bilinear", align_corners=False),
                    F.interpolate(pred * 2 - 1, R, mode="bilinear", align_corners=False))
