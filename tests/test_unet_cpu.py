"""The native UNet / LGM modules (lgm_amd/unet.py, lgm_amd/models.py) on the CPU, against data recorded from the
reference's own UNet (tests/golden/make_unet_golden.py): state_dict keys and shapes of the four presets, a seeded tiny
UNet's output and gradients, the 'big' UNet's output on the catstatue views, and group_norm_silu's torch fallback."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from lgm_amd import LGM, Options, UNet, group_norm_silu, preset
from tests.golden.make_unet_golden import GRAD_PARAMS, PRESETS, TINY, unet_kwargs
from tests.render_cases import rel_l2

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
KEYS = json.load(open(os.path.join(GOLDEN, "unet_keys.json")))


@pytest.mark.parametrize("name", PRESETS)
def test_state_dict_keys_match_reference(name):
    with torch.device("meta"):
        u = UNet(9, 14, **unet_kwargs(preset(name)))
    mine = {k: list(v.shape) for k, v in u.state_dict().items()}
    assert list(mine) == list(KEYS[name])  # the same keys in the same (construction) order
    assert mine == KEYS[name]
    # a reference state_dict (these keys and shapes) loads strictly
    sd = {k: torch.empty(s, device="meta") for k, s in KEYS[name].items()}
    res = u.load_state_dict(sd, strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_preset_fields():
    assert Options() == preset("lrm") and Options().lambda_lpips == 0.0
    big = preset("big")
    assert (big.splat_size, big.output_size, len(big.up_channels)) == (128, 512, 5)
    assert preset("tiny").down_channels == (32, 64, 128, 256, 512)
    assert preset("small", output_size=128).output_size == 128
    with pytest.raises(ValueError):
        preset("huge")


def test_lgm_keys_and_lpips_rule():
    opt = Options(input_size=16, splat_size=16, output_size=32, **TINY)
    with torch.device("meta"):
        m = LGM(opt)
        u = UNet(9, 14, **TINY)
    assert list(m.state_dict()) == ["unet." + k for k in u.state_dict()] + ["conv.weight", "conv.bias"]
    with pytest.raises(ValueError, match="lpips"):
        LGM(Options(lambda_lpips=1.0, **TINY))

    class Perceptual(nn.Module):  # a stand-in with parameters: they stay out of the state_dict
        def __init__(self):
            super().__init__()
            self.net = nn.Conv2d(3, 1, 1)

        def forward(self, a, b):
            return self.net(a - b)

    with torch.device("meta"):
        m2 = LGM(Options(lambda_lpips=1.0, **TINY), lpips=Perceptual())
    assert list(m2.state_dict()) == list(m.state_dict())
    assert not any(p.requires_grad for p in m2.lpips_loss.parameters())
    assert list(m.prepare_default_rays("cpu").shape) == [4, 6, 16, 16]


def test_tiny_unet_matches_reference_fixture():
    z = np.load(os.path.join(GOLDEN, "unet_tiny.npz"))
    torch.manual_seed(0)
    u = UNet(9, 14, **TINY)
    assert sum(p.numel() for p in u.parameters()) == int(z["n_params"]) == 907470
    assert len(u.state_dict()) == int(z["n_keys"]) == 150
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    y = u(x)
    (y * torch.from_numpy(z["w"])).sum().backward()
    params = dict(u.named_parameters())
    errs = {"y": rel_l2(y.detach().numpy(), z["y"]), "grad_x": rel_l2(x.grad.numpy(), z["grad_x"])}
    for k in GRAD_PARAMS:
        errs[k] = rel_l2(params[k].grad.numpy(), z["grad_" + k])
    print(errs)
    assert max(errs.values()) < 1e-5, errs


@pytest.mark.slow
def test_big_unet_matches_recorded_reference_output():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "scripts"))
    import cfg1_cpu as H
    torch.manual_seed(0)
    u = UNet(9, 14, **H.BIG).eval()
    views = H.load_views(os.path.join(GOLDEN, "catstatue_rgba.png"))
    with torch.no_grad():
        y = u(views.view(4, 9, H.INPUT_SIZE, H.INPUT_SIZE)).numpy()
    ref = np.stack([np.load(os.path.join(GOLDEN, f"cfg1_unet_big_v{v}.npz"))["unet_out"] for v in range(4)])
    assert y.shape == ref.shape == (4, 14, 128, 128)
    e = rel_l2(y, ref)
    print("big UNet vs recorded reference output: rel L2", e)
    assert e < 1e-5


@pytest.mark.parametrize("resample", [None, "up", "down"])
def test_group_norm_silu_cpu_is_the_torch_composition(resample):
    torch.manual_seed(3)
    norm = nn.GroupNorm(4, 8)
    with torch.no_grad():
        norm.weight.normal_()
        norm.bias.normal_()
    x = torch.randn(2, 8, 5, 7) if resample != "down" else torch.randn(2, 8, 6, 4)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = group_norm_silu(xa, norm, resample)
    yb = F.silu(F.group_norm(xb, 4, norm.weight, norm.bias, norm.eps))
    if resample == "up":
        yb = F.interpolate(yb, scale_factor=2.0, mode="nearest")
    elif resample == "down":
        yb = F.avg_pool2d(yb, 2, 2)
    assert torch.equal(ya, yb)
    g = torch.randn_like(ya)
    ga, = torch.autograd.grad(ya, xa, g)
    gb, = torch.autograd.grad(yb, xb, g)
    assert torch.equal(ga, gb)
    # odd sizes with 'down' and integer-like dtypes never raise where torch works
    assert group_norm_silu(torch.randn(1, 8, 5, 7), norm, "down").shape == (1, 8, 2, 3)
    assert group_norm_silu(torch.randn(1, 8, 3, 3, dtype=torch.float64), norm.double(), None).dtype == torch.float64
