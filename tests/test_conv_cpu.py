"""lgm_amd.conv.conv2d where the HIP weight gradient does not apply (CPU tensors, fp32): conv(x) itself; and the UNet's
`native_wgrad` switch reaches every block."""
import torch
import torch.nn as nn

from lgm_amd import UNet
from lgm_amd.conv import conv2d
from lgm_amd.unet import ResnetBlock, UpBlock
from tests.golden.make_unet_golden import TINY


def _grads(conv, x0, native, autocast=None):
    conv.zero_grad()
    x = x0.clone().requires_grad_(True)
    if autocast is None:
        y = conv2d(x, conv) if native else conv(x)
    else:
        with torch.autocast("cpu", dtype=autocast):
            y = conv2d(x, conv) if native else conv(x)
    y.float().square().sum().backward()
    return y.detach(), x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()


def test_conv2d_on_cpu_is_conv():
    torch.manual_seed(0)
    for k in (1, 3):
        conv = nn.Conv2d(8, 12, k, padding=k // 2)
        x0 = torch.randn(2, 8, 9, 7)
        for autocast in (None, torch.bfloat16):  # fp32, and CPU autocast (not the GPU path either)
            for a, b in zip(_grads(conv, x0, True, autocast), _grads(conv, x0, False, autocast)):
                assert a.dtype == b.dtype and torch.equal(a, b)
    conv16 = nn.Conv2d(8, 12, 3, padding=1).to(torch.bfloat16)  # a 16-bit module on a 16-bit CPU input
    x16 = torch.randn(2, 8, 9, 7).to(torch.bfloat16)
    for a, b in zip(_grads(conv16, x16, True), _grads(conv16, x16, False)):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_unet_native_wgrad_reaches_every_block():
    u = UNet(9, 14, **TINY)
    blocks = [m for m in u.modules() if isinstance(m, (ResnetBlock, UpBlock))]
    assert len(blocks) > 8 and u.native_wgrad and all(m.native_wgrad for m in blocks)
    attn = [m for m in u.modules() if hasattr(m, "native_wgrad") and not isinstance(m, (ResnetBlock, UpBlock, UNet))]
    assert attn  # MVAttention's own switch (its Linears) is not this one
    u.native_wgrad = False
    assert not u.native_wgrad and not any(m.native_wgrad for m in blocks) and all(m.native_wgrad for m in attn)
    u.native_wgrad = True
    assert u.native_wgrad and all(m.native_wgrad for m in blocks)
    # the switch is no parameter or buffer, and the CPU forward is the same module either way
    assert not [k for k in u.state_dict() if "native" in k]
    x = torch.randn(4, 9, 16, 16)
    ya = u(x)
    u.native_wgrad = False
    assert torch.equal(ya, u(x))
