"""The antialias switch (include/lgm_render.h LGM_RENDER_ANTIALIAS) without a GPU: the dense restatement
tests/render_aa_ref.py is pinned to the frozen oracle with the switch off, the CPU render path is checked against
the restatement with it on, and the factor itself against its closed form and at its clamp."""
import numpy as np
import pytest
import torch

from lgm_amd import cpu as lcpu
from lgm_amd.cameras import orbit_cameras
from lgm_amd.gs import rasterize
from tests import render_aa_ref as R
from tests.render_cases import TAN, rel_l2, scene, upstream

H, W = 40, 56
GROUPS = {"mean": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11), "rgb": slice(11, 14)}


@pytest.fixture(scope="module")
def small():
    g, cv, cvp = scene(N=300, V=2)
    return (g, cv, cvp) + upstream(1, 2, H, W)


def test_restatement_equals_the_oracle_with_the_switch_off(oracle_mod, small):
    """fp64 against the oracle's fp64 build: image, depth, alpha <= 1e-9 rel L2, every gradient group <= 1e-7."""
    g, cv, cvp, d_img, d_dep, d_alp, bg = small
    ref = oracle_mod.render(g.numpy(), cv.numpy(), cvp.numpy(), TAN, H, W, bg.numpy(), f64=True,
                            d_image=d_img.numpy(), d_depth=d_dep.numpy(), d_alpha=d_alp.numpy())
    out = R.render(g, cv, cvp, TAN, H, W, bg, antialias=False, d_image=d_img, d_depth=d_dep, d_alpha=d_alp)
    for k in ("image", "depth", "alpha"):
        e = rel_l2(out[k], ref[k])
        print(k, e)
        assert e <= 1e-9, (k, e)
    for name, sl in GROUPS.items():
        e = rel_l2(out["d_gaussians"][..., sl], ref["d_gaussians"][..., sl])
        print("d_" + name, e)
        assert e <= 1e-7, (name, e)


def test_cpu_path_with_the_switch_on(small):
    g, cv, cvp, _, _, _, bg = small
    ref = R.render(g, cv, cvp, TAN, H, W, bg, antialias=True)
    plain = R.render(g, cv, cvp, TAN, H, W, bg, antialias=False)
    assert rel_l2(ref["image"], plain["image"]) >= 1e-2  # (the scene feels the switch)
    out = lcpu.render_cpu(g, cv, cvp, bg, TAN, TAN, H, W, antialias=True)
    for k, o in zip(("image", "depth", "alpha"), out):
        e = rel_l2(o.numpy(), ref[k])
        print(k, e)
        assert e <= 1e-4, (k, e)
    # the public entry point takes CPU tensors there, with autograd through the factor
    gg = g.clone().requires_grad_(True)
    img, _, alp = rasterize(gg, cv, cvp, bg, TAN, TAN, H, W, antialias=True)
    assert torch.equal(img, out[0])
    (img.sum() + alp.sum()).backward()
    assert torch.isfinite(gg.grad).all() and float(gg.grad[..., 4:7].abs().max()) > 0


def test_cpu_path_with_the_switch_off_is_unchanged(small):
    g, cv, cvp, _, _, _, bg = small
    a = lcpu.render_cpu(g, cv, cvp, bg, TAN, TAN, H, W)
    b = lcpu.render_cpu(g, cv, cvp, bg, TAN, TAN, H, W, antialias=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _on_axis(scales, opacity=0.9):
    """One Gaussian at the origin, on the optical axis of orbit camera 0, with identity rotation."""
    cv, cvp, _ = orbit_cameras(1)
    g = torch.zeros(1, 1, 14)
    g[0, 0, 3] = opacity
    g[0, 0, 4:7] = torch.as_tensor(scales, dtype=torch.float32)
    g[0, 0, 7] = 1.0
    g[0, 0, 11:14] = 1.0
    z = float(cv[0, 3, 2])  # the origin's view-space depth
    return g, cv[None], cvp[None], z


@pytest.mark.parametrize("var", [0.04, 1.0, 25.0])
def test_factor_of_an_isotropic_gaussian(var):
    """Pixel-space variance sigma^2 on the optical axis: s = sigma^2 / (sigma^2 + 0.3) within 1e-6 relative -- in the
    restatement (both dtypes) and in the CPU path's preprocess."""
    fx = W / (2.0 * TAN)
    g, cv, cvp, z = _on_axis([1.0, 1.0, 1.0])
    g[0, 0, 4:7] = np.sqrt(var) * z / fx
    want = var / (var + 0.3)
    for dt in (torch.float64, torch.float32):
        s = float(R.render(g, cv, cvp, TAN, W, W, torch.zeros(3), dtype=dt, antialias=True)["s"][0, 0, 0])
        assert abs(s / want - 1) <= 1e-6, (dt, s, want)
    # the CPU path's compensated opacity over the opacity (the rendered alpha = 1 - T rounds at 6e-8 absolute: too
    # coarse a reading of a 1e-6 bar)
    pre = lcpu._preprocess(g[0], cv[0, 0], cvp[0, 0], TAN, TAN, W, W, 1.0, True)
    s32 = float(pre["opacity"][0].double() / g[0, 0, 3].double())
    print(var, want, s32)
    assert bool(pre["vis"][0]) and abs(s32 / want - 1) <= 1e-6
    # and it reaches the image: the peak alpha scales by s
    on = lcpu.render_cpu(g, cv, cvp, torch.zeros(3), TAN, TAN, W, W, antialias=True)[2]
    off = lcpu.render_cpu(g, cv, cvp, torch.zeros(3), TAN, TAN, W, W)[2]
    if float(off.max()) < 0.98:
        assert abs(float(on.max() / off.max()) / want - 1) <= 1e-4


def test_factor_clamp_of_an_edge_on_needle():
    """A disc seen edge-on has det0 / det <= 2.5e-5: s is the floor's root, 0.005, and carries no gradient."""
    g, cv, cvp, _ = _on_axis([0.1, 1e-6, 0.1])
    info = R.render(g, cv, cvp, TAN, W, W, torch.zeros(3), antialias=True)
    assert abs(float(info["s"][0, 0, 0]) - 0.005) <= 1e-9
    # the restatement's factor: constant under the floor
    a0, b, c0 = (torch.tensor([v], dtype=torch.float64, requires_grad=True) for v in (16.0, 0.0, 1e-7))
    s = R.aa_factor(a0, b, c0)
    s.sum().backward()
    assert float(s.detach()) == float(np.sqrt(R.AA_FLOOR)) and float(a0.grad) == 0 and float(c0.grad) == 0 and float(b.grad) == 0
    # the CPU path: o^ = 0.005 o exactly (fp32), and only the opacity itself receives a gradient from it
    gg = g[0].clone().requires_grad_(True)
    pre = lcpu._preprocess(gg, cv[0, 0], cvp[0, 0], TAN, TAN, W, W, 1.0, True)
    assert bool(pre["vis"][0])
    s32 = np.sqrt(np.float32(2.5e-5))
    assert float(pre["opacity"][0].detach()) == float(np.float32(0.9) * s32)
    pre["opacity"].sum().backward()
    assert float(gg.grad[0, 3]) == float(s32)
    assert float(gg.grad[0, :3].abs().max()) == 0 and float(gg.grad[0, 4:11].abs().max()) == 0


def test_option_bit_and_defaults():
    """The bit is 32 in the header and in _native, and every default is off."""
    import inspect
    import os
    import re

    from lgm_amd import GaussianRenderer, Options, _native
    from lgm_amd import gs as lgs
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgm_render.h")).read()
    assert re.search(r"^#define LGM_RENDER_ANTIALIAS 32$", hdr, re.M) and _native.RENDER_ANTIALIAS == 32
    assert Options().antialias is False
    for fn, default in ((lgs.rasterize, False), (lgs.forward_state, False), (lcpu.render_cpu, False),
                        (GaussianRenderer.render, None)):
        assert inspect.signature(fn).parameters["antialias"].default is default
