"""LGM's UNet (core/unet.py:51-319) on the fused GroupNorm + SiLU (+ resample) HIP kernels (include/lgm_norm.h,
lgm_amd/csrc/gnsilu.hip) and lgm_amd's MVAttention.

Drop-in modules: ResnetBlock, DownBlock, MidBlock, UpBlock and UNet have the constructors, submodule names and
forward signatures of the reference, and create their parameters in the same order, so reference state_dicts load
with strict=True and a seeded construction draws the same weights. Every GroupNorm -> SiLU (-> resample) site goes
through `group_norm_silu`, one HIP pass per direction, while `fused` (a plain attribute, default True) is set;
fused = False runs torch ops as upstream. Attention head dims outside the flash kernels' 32 / 64 / 128 (no LGM preset
has one; test-sized UNets do) take the reference's own fallback attention in torch ops. The stride-1 convolutions go
through lgm_amd.conv.conv2d while `native_wgrad` (a plain attribute, default True) is set: torch's forward and input
gradient, the weight / bias gradient on the HIP split-K kernel (include/lgm_conv.h); the stride-2 downsample
convolutions, torch.cat and the residual (x + shortcut(res)) * skip_scale stay torch. `native_conv` (a plain attribute,
default False) sends the same convolutions through lgm_amd.conv.conv2d_native instead: forward and input gradient on the
HIP implicit-GEMM kernel as well, with or without a recorded graph. Additive: UNet(..., num_frames=4) is passed to every MVAttention (the reference hard-codes 4).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from ._native import ptr
from .attention import MemEffAttention, MVAttention, _autocast_dtype
from .conv import conv2d, conv2d_native
from .cpu import attention_cpu

# Deprecated and unused in this package: the name under which the GPU tests of earlier revisions import the table.
# New code and new tests say nat.DTYPE_CODES.
_DTYPES = nat.DTYPE_CODES

_RESAMPLE = {None: 0, "default": 0, "up": 1, "down": 2}  # include/lgm_norm.h LGM_GN_RESAMPLE_*
_GRID_MAX = 2 ** 31 - 1


_FLASH_HEAD_DIMS = (32, 64, 128)  # what lgm_attn_forward takes (include/lgm_attn.h)


class _FallbackAttention(MemEffAttention):
    """core/attention.py:51-64, the reference's own fallback attention in torch ops, for head dims outside the HIP
    flash kernels' 32 / 64 / 128. No LGM preset has one (512 or 1024 channels over 16 heads: 32 and 64); test-sized
    UNets do (64 channels over 16 heads: 4)."""

    def _attend(self, x: torch.Tensor) -> torch.Tensor:
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads)
        return self.proj_drop(self.proj(attention_cpu(qkv, self.scale).reshape(B, N, C)))


def _mv_attention(dim: int, heads: int, skip_scale: float, num_frames: int) -> MVAttention:
    """The block's MVAttention (same parameters, created in the same order, whatever the head dim)."""
    m = MVAttention(dim, heads, skip_scale=skip_scale, num_frames=num_frames)
    if dim // heads not in _FLASH_HEAD_DIMS:
        m.attn.__class__ = _FallbackAttention  # the same module and parameters; only _attend differs
    return m


def _torch_gn_silu(x, norm: nn.GroupNorm, rs: int):
    y = F.silu(norm(x))
    if rs == 1:
        y = F.interpolate(y, scale_factor=2.0, mode="nearest")
    elif rs == 2:
        y = F.avg_pool2d(y, kernel_size=2, stride=2)
    return y


def _f32(p):
    return None if p is None else p.detach().float().contiguous()


class _GnSilu(torch.autograd.Function):
    """lgm_gn_silu_forward / lgm_gn_silu_backward (the dtypes are _kernel_takes' to check)."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups: int, eps: float, rs: int, y_dtype):
        N, C, H, W = x.shape
        x = x.contiguous()
        oh, ow = (2 * H, 2 * W) if rs == 1 else (H // 2, W // 2) if rs == 2 else (H, W)
        y = torch.empty((N, C, oh, ow), device=x.device, dtype=y_dtype)
        stats = torch.empty((2, N, groups), device=x.device, dtype=torch.float32)  # mean, rstd
        w, b = _f32(weight), _f32(bias)
        # (0 bytes where one launch does it: then nothing is allocated and the workspace is NULL)
        ws, ws_bytes = nat.workspace("lgm_gn_silu_workspace_size", x.device, N, C, H, W, groups, min_bytes=0)
        sp = ptr(stats)
        nat.call("lgm_gn_silu_forward", x.device, nat.DTYPE_CODES[x.dtype], nat.DTYPE_CODES[y_dtype], N, C, H, W,
                 groups, eps, rs, ptr(x), ptr(w), ptr(b), ptr(y), sp, sp + 4 * N * groups, ptr(ws), ws_bytes)
        ctx.save_for_backward(x, w, b, stats)
        ctx.meta = (groups, rs, y_dtype, None if weight is None else weight.dtype, None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, d_y):
        x, w, b, stats = ctx.saved_tensors
        groups, rs, y_dtype, wdt, bdt = ctx.meta
        N, C, H, W = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_w, need_b = need_w and wdt is not None, need_b and bdt is not None
        if not (need_x or need_w or need_b):
            return None, None, None, None, None, None, None
        d_y = d_y.to(y_dtype).contiguous()
        dx = torch.empty_like(x) if need_x else None
        dwb = torch.empty((2, C), device=x.device, dtype=torch.float32) if need_w or need_b else None  # dgamma, dbeta
        ws, ws_bytes = nat.workspace("lgm_gn_silu_backward_workspace_size", x.device, N, C, H, W, groups, min_bytes=0)
        sp = ptr(stats)
        nat.call("lgm_gn_silu_backward", x.device, nat.DTYPE_CODES[x.dtype], nat.DTYPE_CODES[y_dtype], N, C, H, W,
                 groups, rs, ptr(x), ptr(w), ptr(b), sp, sp + 4 * N * groups, ptr(d_y), ptr(dx),
                 ptr(dwb) if need_w else None, ptr(dwb) + 4 * C if need_b else None, ptr(ws), ws_bytes)
        return dx, (dwb[0].to(wdt) if need_w else None), (dwb[1].to(bdt) if need_b else None), None, None, None, None


def _kernel_takes(x: torch.Tensor, norm: nn.GroupNorm, rs: int, y_dtype) -> bool:
    """What lgm_gn_silu_* accepts (include/lgm_norm.h); everything else is torch's."""
    if not x.is_cuda or x.dim() != 4 or x.numel() == 0 or x.dtype not in nat.DTYPE_CODES or \
            y_dtype not in nat.DTYPE_CODES:
        return False
    if x.dtype != torch.float32 and y_dtype != x.dtype:
        return False
    N, C, H, W = x.shape
    if C != norm.num_channels or (rs == 2 and (H % 2 or W % 2)):
        return False
    for p in (norm.weight, norm.bias):
        if p is not None and (p.device != x.device or p.dtype not in nat.DTYPE_CODES):
            return False
    # the launch grids (one workgroup per 1024 pixels of a plane, per 4096 elements of a group) and the element count
    return N * C * (-(-H * W // 1024)) <= _GRID_MAX and N * C * (-(-H * W // 4096) + 1) <= _GRID_MAX and \
        N * C * H * W * 4 < 2 ** 60


def group_norm_silu(x: torch.Tensor, norm: nn.GroupNorm, resample=None) -> torch.Tensor:
    """resample(silu(norm(x))) of x [N, C, H, W]; resample: None / 'default', 'up' (2x nearest) or 'down' (2x2 average
    pool). GPU float32 / bfloat16 / float16 tensors run one HIP pass per direction; the output dtype is the autocast
    dtype while CUDA autocast is active, else x's (under autocast the reference rounds the fp32 activation once, at the
    next conv's cast: the same values). Anything the kernels do not take -- CPU tensors, other dtypes, odd sizes with
    'down' -- is the torch composition F.group_norm -> F.silu -> F.avg_pool2d / F.interpolate."""
    if resample not in _RESAMPLE:
        raise ValueError(f"resample must be None, 'default', 'up' or 'down', got {resample!r}")
    rs = _RESAMPLE[resample]
    ac = _autocast_dtype("cuda") if x.is_cuda else None
    y_dtype = ac if ac is not None else x.dtype
    if not _kernel_takes(x, norm, rs, y_dtype):
        return _torch_gn_silu(x, norm, rs)
    return _GnSilu.apply(x, norm.weight, norm.bias, norm.num_groups, norm.eps, rs, y_dtype)


def _conv_site(x, conv: nn.Conv2d, wgrad: bool, native_conv: bool):
    """One stride-1 convolution of a fused block: every direction on the HIP kernels (native_conv), the weight gradient
    alone (wgrad: the module-level conv2d), or the module itself."""
    if native_conv:
        return conv2d_native(x, conv)
    return conv2d(x, conv) if wgrad else conv(x)


class ResnetBlock(nn.Module):
    """core/unet.py:51-103."""

    def __init__(self, in_channels: int, out_channels: int, resample: str = "default", groups: int = 32,
                 eps: float = 1e-5, skip_scale: float = 1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.skip_scale = skip_scale
        self.norm1 = nn.GroupNorm(num_groups=groups, num_channels=in_channels, eps=eps, affine=True)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.norm2 = nn.GroupNorm(num_groups=groups, num_channels=out_channels, eps=eps, affine=True)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.act = F.silu
        self.resample_mode = resample if resample in ("up", "down") else None
        self.shortcut = nn.Identity()
        if self.in_channels != self.out_channels:
            self.shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=1, bias=True)
        self.fused = True  # the HIP GroupNorm+SiLU(+resample) kernels (False: torch ops, as upstream)
        self.native_wgrad = True  # the HIP conv weight gradient while fused (False: torch's autograd through the convs)
        self.native_conv = False  # the HIP conv forward and input gradient too, while fused (opt-in)

    def _resample(self, t):
        if self.resample_mode == "up":
            return F.interpolate(t, scale_factor=2.0, mode="nearest")
        return F.avg_pool2d(t, kernel_size=2, stride=2)

    def forward(self, x):
        res = x
        native = self.fused and self.native_wgrad
        nconv = self.fused and self.native_conv
        if self.fused:
            x = group_norm_silu(x, self.norm1, self.resample_mode)
            if self.resample_mode:
                res = self._resample(res)
            x = _conv_site(x, self.conv1, native, nconv)
            x = group_norm_silu(x, self.norm2)
        else:
            x = self.act(self.norm1(x))
            if self.resample_mode:
                res = self._resample(res)
                x = self._resample(x)
            x = self.conv1(x)
            x = self.act(self.norm2(x))
        x = _conv_site(x, self.conv2, native, nconv)
        if self.in_channels != self.out_channels:
            res = _conv_site(res, self.shortcut, native, nconv)
        else:
            res = self.shortcut(res)
        return (x + res) * self.skip_scale


class DownBlock(nn.Module):
    """core/unet.py:105-147."""

    def __init__(self, in_channels: int, out_channels: int, num_layers: int = 1, downsample: bool = True,
                 attention: bool = True, attention_heads: int = 16, skip_scale: float = 1, num_frames: int = 4):
        super().__init__()
        nets, attns = [], []
        for i in range(num_layers):
            in_channels = in_channels if i == 0 else out_channels
            nets.append(ResnetBlock(in_channels, out_channels, skip_scale=skip_scale))
            attns.append(_mv_attention(out_channels, attention_heads, skip_scale, num_frames)
                         if attention else None)
        self.nets = nn.ModuleList(nets)
        self.attns = nn.ModuleList(attns)
        self.downsample = None
        if downsample:
            self.downsample = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        xs = []
        for attn, net in zip(self.attns, self.nets):
            x = net(x)
            if attn:
                x = attn(x)
            xs.append(x)
        if self.downsample:
            x = self.downsample(x)
            xs.append(x)
        return x, xs


class MidBlock(nn.Module):
    """core/unet.py:150-181."""

    def __init__(self, in_channels: int, num_layers: int = 1, attention: bool = True, attention_heads: int = 16,
                 skip_scale: float = 1, num_frames: int = 4):
        super().__init__()
        nets, attns = [], []
        nets.append(ResnetBlock(in_channels, in_channels, skip_scale=skip_scale))
        for i in range(num_layers):
            nets.append(ResnetBlock(in_channels, in_channels, skip_scale=skip_scale))
            attns.append(_mv_attention(in_channels, attention_heads, skip_scale, num_frames)
                         if attention else None)
        self.nets = nn.ModuleList(nets)
        self.attns = nn.ModuleList(attns)

    def forward(self, x):
        x = self.nets[0](x)
        for attn, net in zip(self.attns, self.nets[1:]):
            if attn:
                x = attn(x)
            x = net(x)
        return x


class UpBlock(nn.Module):
    """core/unet.py:184-230."""

    def __init__(self, in_channels: int, prev_out_channels: int, out_channels: int, num_layers: int = 1,
                 upsample: bool = True, attention: bool = True, attention_heads: int = 16, skip_scale: float = 1,
                 num_frames: int = 4):
        super().__init__()
        nets, attns = [], []
        for i in range(num_layers):
            cin = in_channels if i == 0 else out_channels
            cskip = prev_out_channels if (i == num_layers - 1) else out_channels
            nets.append(ResnetBlock(cin + cskip, out_channels, skip_scale=skip_scale))
            attns.append(_mv_attention(out_channels, attention_heads, skip_scale, num_frames)
                         if attention else None)
        self.nets = nn.ModuleList(nets)
        self.attns = nn.ModuleList(attns)
        self.upsample = None
        if upsample:
            self.upsample = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.native_wgrad = True  # the HIP conv weight gradient of `upsample`, while the block's ResnetBlocks are fused
        self.native_conv = False  # its forward and input gradient on the HIP kernel too (opt-in)

    def forward(self, x, xs):
        for attn, net in zip(self.attns, self.nets):
            res_x = xs[-1]
            xs = xs[:-1]
            x = torch.cat([x, res_x], dim=1)
            x = net(x)
            if attn:
                x = attn(x)
        if self.upsample:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            fused = self.nets[0].fused
            x = _conv_site(x, self.upsample, self.native_wgrad and fused, self.native_conv and fused)
        return x


class UNet(nn.Module):
    """core/unet.py:234-319 (it may be asymmetric: fewer up blocks than down blocks)."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3,
                 down_channels: Tuple[int, ...] = (64, 128, 256, 512, 1024),
                 down_attention: Tuple[bool, ...] = (False, False, False, True, True), mid_attention: bool = True,
                 up_channels: Tuple[int, ...] = (1024, 512, 256), up_attention: Tuple[bool, ...] = (True, True, False),
                 layers_per_block: int = 2, skip_scale: float = np.sqrt(0.5), num_frames: int = 4):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels, down_channels[0], kernel_size=3, stride=1, padding=1)
        down_blocks = []
        cout = down_channels[0]
        for i in range(len(down_channels)):
            cin, cout = cout, down_channels[i]
            down_blocks.append(DownBlock(cin, cout, num_layers=layers_per_block,
                                         downsample=(i != len(down_channels) - 1), attention=down_attention[i],
                                         skip_scale=skip_scale, num_frames=num_frames))
        self.down_blocks = nn.ModuleList(down_blocks)
        self.mid_block = MidBlock(down_channels[-1], attention=mid_attention, skip_scale=skip_scale,
                                  num_frames=num_frames)
        up_blocks = []
        cout = up_channels[0]
        for i in range(len(up_channels)):
            cin, cout = cout, up_channels[i]
            cskip = down_channels[max(-2 - i, -len(down_channels))]  # for the asymmetric case
            up_blocks.append(UpBlock(cin, cskip, cout, num_layers=layers_per_block + 1,
                                     upsample=(i != len(up_channels) - 1), attention=up_attention[i],
                                     skip_scale=skip_scale, num_frames=num_frames))
        self.up_blocks = nn.ModuleList(up_blocks)
        self.norm_out = nn.GroupNorm(num_channels=up_channels[-1], num_groups=32, eps=1e-5)
        self.conv_out = nn.Conv2d(up_channels[-1], out_channels, kernel_size=3, stride=1, padding=1)
        self._fused = True
        self._native_wgrad = True
        self._native_conv = False

    @property
    def native_conv(self) -> bool:
        """The HIP conv forward and input gradient at conv_in / conv_out (while `fused`); setting it sets every
        ResnetBlock's and UpBlock's `native_conv` too. Off by default."""
        return self._native_conv

    @native_conv.setter
    def native_conv(self, value: bool):
        self._native_conv = bool(value)
        for m in self.modules():
            if isinstance(m, (ResnetBlock, UpBlock)):
                m.native_conv = bool(value)

    @property
    def native_wgrad(self) -> bool:
        """The HIP conv weight gradient at conv_in / conv_out (while `fused`); setting it sets every ResnetBlock's and
        UpBlock's `native_wgrad` too (the MVAttention blocks keep their own switch for their Linears)."""
        return self._native_wgrad

    @native_wgrad.setter
    def native_wgrad(self, value: bool):
        self._native_wgrad = bool(value)
        for m in self.modules():
            if isinstance(m, (ResnetBlock, UpBlock)):
                m.native_wgrad = bool(value)

    @property
    def fused(self) -> bool:
        """The HIP GroupNorm+SiLU kernels at norm_out; setting it sets every ResnetBlock's `fused` too (the
        MVAttention blocks keep their own switch)."""
        return self._fused

    @fused.setter
    def fused(self, value: bool):
        self._fused = bool(value)
        for m in self.modules():
            if isinstance(m, ResnetBlock):
                m.fused = bool(value)

    def forward(self, x):
        native = self._fused and self._native_wgrad
        nconv = self._fused and self._native_conv
        x = _conv_site(x, self.conv_in, native, nconv)
        xss = [x]
        for block in self.down_blocks:
            x, xs = block(x)
            xss.extend(xs)
        x = self.mid_block(x)
        for block in self.up_blocks:
            xs = xss[-len(block.nets):]
            xss = xss[:-len(block.nets)]
            x = block(x, xs)
        x = group_norm_silu(x, self.norm_out) if self._fused else F.silu(self.norm_out(x))
        return _conv_site(x, self.conv_out, native, nconv)
