"""Golden data for tests/test_unet_cpu.py and tests/test_unet_gpu.py, recorded with a checkout of the reference LGM
at hand (its code is imported here and never stored; the files hold names, shapes, inputs and recorded results only):

  unet_keys.json  state_dict key -> shape of the reference UNet(9, 14, ...) for the 'lrm', 'small', 'big' and 'tiny'
                  presets (built on the meta device: no weights are materialised);
  unet_tiny.npz   the reference UNet with down_channels (32, 64), down_attention (F, T), mid_attention, up_channels
                  (64, 32), up_attention (T, F) -- 907,470 parameters, 150 keys; its concatenations give a 96-channel
                  GroupNorm (3 channels per group) -- built under torch.manual_seed(0), fp32 on the CPU with the
                  reference's fallback attention (XFORMERS_DISABLED=1): the input x [8, 9, 16, 16], the output
                  y [8, 14, 16, 16], the weights w of the scalar sum(y * w), and that scalar's gradients with respect
                  to x and five parameters. No weights are stored: the seed reproduces them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unet_golden.py --reference LGM_CHECKOUT
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

TINY = dict(down_channels=(32, 64), down_attention=(False, True), mid_attention=True, up_channels=(64, 32),
            up_attention=(True, False))
GRAD_PARAMS = ("conv_in.weight", "down_blocks.1.nets.0.norm1.weight", "mid_block.attns.0.attn.qkv.weight",
               "up_blocks.0.nets.2.shortcut.bias", "norm_out.bias")
PRESETS = ("lrm", "small", "big", "tiny")


def unet_kwargs(opt):
    return dict(down_channels=opt.down_channels, down_attention=opt.down_attention, mid_attention=opt.mid_attention,
                up_channels=opt.up_channels, up_attention=opt.up_attention)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference LGM (its core/unet.py)")
    a = ap.parse_args()
    os.environ.setdefault("XFORMERS_DISABLED", "1")
    sys.dont_write_bytecode = True  # the reference checkout is read-only
    sys.path.insert(0, a.reference)
    from core.unet import UNet  # noqa: E402  (reference code, imported and never stored)

    from lgm_amd.options import preset
    keys = {}
    for name in PRESETS:
        with torch.device("meta"):
            u = UNet(9, 14, **unet_kwargs(preset(name)))
        keys[name] = {k: list(v.shape) for k, v in u.state_dict().items()}
    with open(os.path.join(HERE, "unet_keys.json"), "w") as f:
        json.dump(keys, f, separators=(",", ":"))

    torch.manual_seed(0)
    u = UNet(9, 14, **TINY)
    n_params = sum(p.numel() for p in u.parameters())
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(8, 9, 16, 16, generator=gen).requires_grad_(True)
    w = torch.randn(8, 14, 16, 16, generator=gen)
    y = u(x)
    (y * w).sum().backward()
    params = dict(u.named_parameters())
    out = {"x": x.detach().numpy(), "y": y.detach().numpy(), "w": w.numpy(), "grad_x": x.grad.numpy(),
           "n_params": np.int64(n_params), "n_keys": np.int64(len(u.state_dict()))}
    for k in GRAD_PARAMS:
        out["grad_" + k] = params[k].grad.numpy()
    np.savez_compressed(os.path.join(HERE, "unet_tiny.npz"), **out)
    print("tiny:", n_params, "parameters,", len(u.state_dict()), "keys; presets:",
          {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    main()
