"""The subset of core/options.py:6-75 `Options` that the model, render and attention path reads. Plain dataclass:
tyro and the training-loop settings are out of scope. `preset(name)` gives the model shapes of the reference's
config_defaults (core/options.py:78-121)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple


@dataclass
class Options:
    input_size: int = 256
    splat_size: int = 64
    output_size: int = 256
    fovy: float = 49.1
    znear: float = 0.5
    zfar: float = 2.5
    num_views: int = 12
    num_input_views: int = 4
    cam_radius: float = 1.5
    # the UNet (core/options.py:12-16)
    down_channels: Tuple[int, ...] = (64, 128, 256, 512, 1024, 1024)
    down_attention: Tuple[bool, ...] = (False, False, False, True, True, True)
    mid_attention: bool = True
    up_channels: Tuple[int, ...] = (1024, 1024, 512, 256)
    up_attention: Tuple[bool, ...] = (True, True, True, False)
    # LPIPS weight of the loss. The reference defaults to 1.0 with downloaded VGG weights; here the weights (for the
    # native lgm_amd.lpips.LPIPS) or a network are supplied by the caller (lgm_amd.models.LGM(opt, lpips=...)), so the
    # default is off.
    lambda_lpips: float = 0.0
    # augmentation probabilities of the provider (core/options.py:62-64), read by lgm_amd.data.build_batch
    prob_grid_distortion: float = 0.5
    prob_cam_jitter: float = 0.5
    # opacity compensation of the rasteriser's 0.3 px^2 dilation (include/lgm_render.h LGM_RENDER_ANTIALIAS; the 3DGS
    # rasteriser's `antialiasing`): read by GaussianRenderer.render at every call. Off: the rasteriser LGM pins.
    antialias: bool = False


_PRESETS = {
    "lrm": {},
    "small": dict(input_size=256, splat_size=64, output_size=256),
    "big": dict(input_size=256, up_channels=(1024, 1024, 512, 256, 128),
                up_attention=(True, True, True, False, False), splat_size=128, output_size=512, num_views=8),
    "tiny": dict(input_size=256, down_channels=(32, 64, 128, 256, 512),
                 down_attention=(False, False, False, False, True), up_channels=(512, 256, 128),
                 up_attention=(True, False, False, False), splat_size=64, output_size=256, num_views=8),
}


def preset(name: str, **overrides) -> Options:
    """Options of the reference's 'lrm' / 'small' / 'big' / 'tiny' configuration (model and render fields)."""
    if name not in _PRESETS:
        raise ValueError(f"unknown preset {name!r}: one of {sorted(_PRESETS)}")
    return Options(**{**_PRESETS[name], **overrides})
