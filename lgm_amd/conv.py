"""The UNet's stride-1 3 x 3 and 1 x 1 convolutions (core/unet.py: ResnetBlock conv1 / conv2 / shortcut, UpBlock
upsample, UNet conv_in / conv_out) under 16-bit autocast, with the weight and bias gradients on the HIP split-K MFMA
kernel (lgm_amd/csrc/conv_wgrad.hip, include/lgm_conv.h).

The forward and the input gradient are the library convolutions torch's autocast runs for nn.Conv2d (F.conv2d on the
16-bit casts of input, weight and bias; aten.convolution_backward for the input alone). The weight and bias gradients
-- reductions over every pixel of the batch -- come from lgm_conv_wgrad, in fp32 straight into the fp32 parameters'
gradients (torch rounds them to the autocast dtype first and casts back). fp32 convolutions (no autocast), strided,
dilated, grouped and other kernel sizes stay on torch.

Opt-in: conv2d_native runs the forward and the input gradient on the HIP implicit-GEMM kernel too (lgm_conv_forward /
lgm_conv_dgrad, lgm_amd/csrc/conv_fwd.hip), reading the fp32 parameter directly (the kernel's packing pass rounds it:
no per-call weight cast in torch), with and without a recorded graph. conv2d is unchanged by it.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from ._native import ptr

DTYPES = (torch.bfloat16, torch.float16)  # the operand dtypes the kernels take
_GRID_MAX = 2 ** 31 - 1


def wgrad(dy: torch.Tensor, x: torch.Tensor, ksize: int, want_db: bool):
    """lgm_conv_wgrad on dense NCHW 16-bit GPU tensors dy [N, Cout, H, W] and x [N, Cin, H, W]: (dw fp32
    [Cout, Cin, ksize, ksize], db fp32 [Cout] or None). The tensors may start at any element of their storage."""
    N, Cout, H, W = dy.shape
    Cin = x.shape[1]
    dw = torch.empty((Cout, Cin, ksize, ksize), device=dy.device, dtype=torch.float32)
    db = torch.empty((Cout,), device=dy.device, dtype=torch.float32) if want_db else None
    ws, ws_bytes = nat.workspace("lgm_conv_wgrad_workspace_size", dy.device, N, Cin, Cout, H, W, ksize, int(want_db))
    nat.call("lgm_conv_wgrad", dy.device, nat.DTYPE_CODES[dy.dtype], N, Cin, Cout, H, W, ksize, ptr(dy), ptr(x), ptr(dw),
             ptr(db), ptr(ws), ws_bytes)
    return dw, db


def _w_code(t: torch.Tensor, dt) -> int:
    return nat.DTYPE_CODES[torch.float32 if t.dtype == torch.float32 else dt]


def conv_forward(x16: torch.Tensor, w: torch.Tensor, bias, ksize: int) -> torch.Tensor:
    """lgm_conv_forward: y [N, Cout, H, W] of x16's dtype from the dense NCHW 16-bit GPU tensor x16 [N, Cin, H, W], the
    contiguous weight w [Cout, Cin, ksize, ksize] and bias [Cout] or None, each fp32 or x16's dtype. The tensors may
    start at any element of their storage."""
    N, Cin, H, W = x16.shape
    Cout = w.shape[0]
    dt = x16.dtype
    y = torch.empty((N, Cout, H, W), device=x16.device, dtype=dt)
    ws, ws_bytes = nat.workspace("lgm_conv_forward_workspace_size", x16.device, N, Cin, Cout, H, W, ksize)
    nat.call("lgm_conv_forward", x16.device, nat.DTYPE_CODES[dt], _w_code(w, dt), N, Cin, Cout, H, W, ksize, ptr(x16),
             ptr(w), ptr(bias), 0 if bias is None else _w_code(bias, dt), ptr(y), ptr(ws), ws_bytes)
    return y


def conv_dgrad(dy16: torch.Tensor, w: torch.Tensor, ksize: int) -> torch.Tensor:
    """lgm_conv_dgrad: dx [N, Cin, H, W] of dy16's dtype from the dense NCHW 16-bit GPU tensor dy16 [N, Cout, H, W] and
    the contiguous weight w [Cout, Cin, ksize, ksize] (fp32 or dy16's dtype)."""
    N, Cout, H, W = dy16.shape
    Cin = w.shape[1]
    dt = dy16.dtype
    dx = torch.empty((N, Cin, H, W), device=dy16.device, dtype=dt)
    ws, ws_bytes = nat.workspace("lgm_conv_dgrad_workspace_size", dy16.device, N, Cin, Cout, H, W, ksize)
    nat.call("lgm_conv_dgrad", dy16.device, nat.DTYPE_CODES[dt], _w_code(w, dt), N, Cin, Cout, H, W, ksize, ptr(dy16),
             ptr(w), ptr(dx), ptr(ws), ws_bytes)
    return dx


class _Conv16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, dt, pad: int):
        with torch.autocast("cuda", enabled=False):
            x16 = x.to(dt)
            w16 = weight.to(dt)
            out = F.conv2d(x16, w16, None if bias is None else bias.to(dt), 1, pad)
        ctx.save_for_backward(x16, w16)
        ctx.meta = (x.dtype, weight.dtype, None if bias is None else bias.dtype, dt, pad)
        return out

    @staticmethod
    def backward(ctx, g):
        x16, w16 = ctx.saved_tensors
        xdt, wdt, bdt, dt, pad = ctx.meta
        g16 = g.to(dt)
        gx = None
        if ctx.needs_input_grad[0]:
            with torch.autocast("cuda", enabled=False):
                gx = torch.ops.aten.convolution_backward(g16, x16, w16, None, [1, 1], [pad, pad], [1, 1], False, [0, 0],
                                                         1, [True, False, False])[0].to(xdt)
        dw = db = None
        want_w = ctx.needs_input_grad[1]
        want_b = bdt is not None and ctx.needs_input_grad[2]
        if want_w or want_b:
            # dense NCHW for the C ABI (a channels_last activation or gradient is copied; a view into a larger buffer
            # that is already dense goes as it is, at whatever element it starts: the kernel takes any alignment)
            dw, db = wgrad(g16.contiguous(), x16.contiguous(), w16.shape[-1], want_b)
            dw = dw.to(wdt) if want_w else None
            db = None if db is None else db.to(bdt)
        return gx, dw, db, None, None


# (Cin, Cout, H, W, ksize) on which MIOpen's weight + bias gradient measured faster than k_conv_wgrad at 4 or at 32 views
# (DESIGN §4 "Conv weight gradient", profiles/conv_wgrad/bench_conv.json): one of the 43 stride-1 shapes of LGM 'big'
_TORCH_FASTER = {(768, 256, 64, 64, 3)}


def _shape_goes_native(Cin: int, Cout: int, H: int, W: int, ksize: int) -> bool:
    """The dispatch rule: a shape goes to the kernel unless the table has it slower than torch's arm at either view
    count by more than the spread between two runs (shapes the table does not have go to the kernel: it won or tied
    on 85 of its 86 rows)."""
    return (Cin, Cout, H, W, ksize) not in _TORCH_FASTER


# (Cin, Cout, H, W, ksize) on which the library's forward / input gradient measured faster than k_conv_fwd /
# k_conv_dgrad at 4 or at 32 views by more than the spread between two runs (7.8 %: DESIGN §4 "Conv forward and input
# gradient", profiles/conv_fwd/bench_conv_fwd.json): 40 and 41 of the 43 stride-1 shapes of LGM 'big'. With the switch on
# these still take the library's arm; shapes the tables do not have go to the kernel.
_FWD_TORCH_FASTER = {
    (64, 64, 256, 256, 3), (64, 128, 128, 128, 3), (128, 14, 128, 128, 3), (128, 128, 128, 128, 3),
    (128, 256, 64, 64, 3), (192, 128, 128, 128, 1), (192, 128, 128, 128, 3), (256, 128, 128, 128, 1),
    (256, 128, 128, 128, 3), (256, 256, 64, 64, 3), (256, 256, 128, 128, 3), (256, 512, 32, 32, 1),
    (256, 512, 32, 32, 3), (384, 128, 128, 128, 1), (384, 128, 128, 128, 3), (384, 256, 64, 64, 1),
    (384, 256, 64, 64, 3), (512, 256, 64, 64, 1), (512, 256, 64, 64, 3), (512, 512, 32, 32, 3),
    (512, 512, 64, 64, 3), (512, 1024, 16, 16, 1), (512, 1024, 16, 16, 3), (768, 256, 64, 64, 1),
    (768, 256, 64, 64, 3), (768, 512, 32, 32, 1), (768, 512, 32, 32, 3), (1024, 512, 32, 32, 1),
    (1024, 512, 32, 32, 3), (1024, 1024, 8, 8, 3), (1024, 1024, 16, 16, 3), (1024, 1024, 32, 32, 3),
    (1536, 512, 32, 32, 1), (1536, 512, 32, 32, 3), (1536, 1024, 16, 16, 1), (1536, 1024, 16, 16, 3),
    (2048, 1024, 8, 8, 1), (2048, 1024, 8, 8, 3), (2048, 1024, 16, 16, 1), (2048, 1024, 16, 16, 3),
}
_DGRAD_TORCH_FASTER = {
    (9, 64, 256, 256, 3), (64, 64, 256, 256, 3), (64, 128, 128, 128, 3), (128, 128, 128, 128, 3),
    (128, 256, 64, 64, 1), (128, 256, 64, 64, 3), (192, 128, 128, 128, 1), (192, 128, 128, 128, 3),
    (256, 128, 128, 128, 1), (256, 128, 128, 128, 3), (256, 256, 64, 64, 3), (256, 256, 128, 128, 3),
    (256, 512, 32, 32, 1), (256, 512, 32, 32, 3), (384, 128, 128, 128, 1), (384, 128, 128, 128, 3),
    (384, 256, 64, 64, 1), (384, 256, 64, 64, 3), (512, 256, 64, 64, 1), (512, 256, 64, 64, 3),
    (512, 512, 32, 32, 3), (512, 512, 64, 64, 3), (512, 1024, 16, 16, 1), (512, 1024, 16, 16, 3),
    (768, 256, 64, 64, 1), (768, 256, 64, 64, 3), (768, 512, 32, 32, 1), (768, 512, 32, 32, 3),
    (1024, 512, 32, 32, 1), (1024, 512, 32, 32, 3), (1024, 1024, 8, 8, 3), (1024, 1024, 16, 16, 3),
    (1024, 1024, 32, 32, 3), (1536, 512, 32, 32, 1), (1536, 512, 32, 32, 3), (1536, 1024, 16, 16, 1),
    (1536, 1024, 16, 16, 3), (2048, 1024, 8, 8, 1), (2048, 1024, 8, 8, 3), (2048, 1024, 16, 16, 1),
    (2048, 1024, 16, 16, 3),
}


def _fwd_goes_native(Cin: int, Cout: int, H: int, W: int, ksize: int) -> bool:
    return (Cin, Cout, H, W, ksize) not in _FWD_TORCH_FASTER


def _dgrad_goes_native(Cin: int, Cout: int, H: int, W: int, ksize: int) -> bool:
    return (Cin, Cout, H, W, ksize) not in _DGRAD_TORCH_FASTER


def _takes(x: torch.Tensor, conv: nn.Conv2d):
    """(autocast dtype, padding) where lgm_conv_wgrad serves this call, else None."""
    t = _takes_kind(x, conv)
    if t is None or not _shape_goes_native(x.shape[1], conv.out_channels, x.shape[2], x.shape[3], conv.kernel_size[0]):
        return None
    return t


def _takes_kind(x: torch.Tensor, conv: nn.Conv2d):
    """_takes without the weight gradient's per-shape rule: (autocast dtype, padding) where the conv kernels'
    operation, operands and grids fit this call, else None."""
    if not isinstance(conv, nn.Conv2d) or not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_cuda:
        return None
    w = conv.weight
    if w.device != x.device or (conv.bias is not None and conv.bias.device != x.device):
        return None
    if torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        if not x.is_floating_point():
            return None
    elif x.dtype in DTYPES and w.dtype == x.dtype:
        dt = x.dtype
    else:
        return None
    k = conv.kernel_size[0]
    if dt not in DTYPES or conv.kernel_size not in ((1, 1), (3, 3)) or conv.stride != (1, 1) or \
            conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros" or conv.transposed:
        return None
    pad = (k - 1) // 2
    if conv.padding != (pad, pad) and conv.padding != "same":
        return None
    N, C, H, W = x.shape
    if C != conv.in_channels or x.numel() == 0 or N * H > _GRID_MAX:
        return None
    tiles = (-(-conv.out_channels // 64)) * (-(-C // 64))
    if tiles * 9 * 16 > _GRID_MAX:
        return None
    return dt, pad


def conv2d(x: torch.Tensor, conv: nn.Conv2d) -> torch.Tensor:
    """conv(x), with the HIP weight / bias gradient where the convolution runs in 16 bits on the GPU (under bf16 / fp16
    autocast, or a 16-bit module on a 16-bit input), is stride 1, dilation 1, groups 1, 1 x 1 or 3 x 3 with zero padding
    of (k - 1) / 2, and the shape is one the kernel is not slower on. Anything else -- fp32, CPU tensors, stride 2, other
    kernels and paddings -- is conv(x), and so is a call that records no graph (inference)."""
    if not (torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad or
                                         (conv.bias is not None and conv.bias.requires_grad))):
        return conv(x)
    t = _takes(x, conv)
    if t is None:
        return conv(x)
    return _Conv16.apply(x, conv.weight, conv.bias, t[0], t[1])


class _ConvNative(torch.autograd.Function):
    """Forward on lgm_conv_forward (the parameter as it is: fp32 under autocast), backward on lgm_conv_dgrad and
    lgm_conv_wgrad; the per-shape tables send an arm to the library convolution instead."""

    @staticmethod
    def forward(ctx, x, weight, bias, dt, pad: int):
        k = weight.shape[-1]
        shape = (weight.shape[1], weight.shape[0], x.shape[2], x.shape[3], k)
        x16 = x.detach().to(dt).contiguous()
        w = weight.detach()
        w = (w if w.dtype in (torch.float32, dt) else w.to(dt)).contiguous()
        b = None if bias is None else bias.detach()
        b = b if b is None or b.dtype in (torch.float32, dt) else b.to(dt)
        if _fwd_goes_native(*shape):
            out = conv_forward(x16, w, None if b is None else b.contiguous(), k)
        else:
            with torch.autocast("cuda", enabled=False):
                out = F.conv2d(x16, w.to(dt), None if b is None else b.to(dt), 1, pad)
        ctx.save_for_backward(x16, weight)
        ctx.meta = (x.dtype, weight.dtype, None if bias is None else bias.dtype, dt, pad, shape)
        return out

    @staticmethod
    def backward(ctx, g):
        x16, weight = ctx.saved_tensors
        xdt, wdt, bdt, dt, pad, shape = ctx.meta
        k = shape[-1]
        g16 = g.to(dt).contiguous()
        w = weight.detach()
        w = (w if w.dtype in (torch.float32, dt) else w.to(dt)).contiguous()
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_b = bdt is not None and ctx.needs_input_grad[2]
        gx = dw = db = None
        native_x = _dgrad_goes_native(*shape)
        native_w = _shape_goes_native(*shape)
        if want_x and native_x:
            gx = conv_dgrad(g16, w, k).to(xdt)
        if (want_w or want_b) and native_w:
            dw, db = wgrad(g16, x16, k, want_b)
        aten_x, aten_w = want_x and not native_x, (want_w or want_b) and not native_w
        if aten_x or aten_w:
            with torch.autocast("cuda", enabled=False):
                r = torch.ops.aten.convolution_backward(g16, x16, w.to(dt), [w.shape[0]] if aten_w and want_b else None,
                                                        [1, 1], [pad, pad], [1, 1], False, [0, 0], 1,
                                                        [aten_x, aten_w, aten_w and want_b])
            if aten_x:
                gx = r[0].to(xdt)
            if aten_w:
                dw, db = r[1], (r[2] if want_b else None)
        dw = dw.to(wdt) if want_w and dw is not None else None
        db = db.to(bdt) if want_b and db is not None else None
        return gx, dw, db, None, None


def conv2d_native(x: torch.Tensor, conv: nn.Conv2d) -> torch.Tensor:
    """conv(x) with the forward, the input gradient and the weight / bias gradient on the HIP kernels, for the calls
    conv2d takes (16-bit on the GPU, stride 1, 1 x 1 or 3 x 3 with zero padding (k - 1) / 2) and also where no graph is
    recorded (inference). The weight gradient keeps conv2d's per-shape rule (a shape it excludes takes aten's weight
    gradient); the forward and the input gradient have tables of their own. Anything else is conv(x)."""
    t = _takes_kind(x, conv)
    if t is None:
        return conv(x)
    return _ConvNative.apply(x, conv.weight, conv.bias, t[0], t[1])
