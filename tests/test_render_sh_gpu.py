"""Spherical-harmonics colour (include/lgm_render.h LGM_RENDER_SH_MASK) on the GPU, against the fp64 dense
restatement tests/render_sh_ref.py (pinned to the plain render and to the basis' orthonormality by
tests/test_render_sh_cpu.py).

Bars: forward outputs 1e-4 rel L2 (the project's forward bar); gradients per parameter group
render_cases.grad_bar(e32) = max(1e-4, 1.25 x e32), e32 the fp32 restatement's own error against fp64 on the same
inputs; everything said to be equal is equal bit for bit. The scene is the antialias tests' (scene(N=1000, V=2, seed=3,
scale_mul=2.0) at 40 x 56), its rest coefficients drawn here (render_sh_ref.lift: N(0, 0.6^2)); it is sensitive to them
by the reference alone, asserted in test_forward: the reference image is >= 1e-2 rel L2 from the DC-only one and
between 5 % and 50 % of the visible colours sit at the clamp.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lgm_amd import _native as nat
from lgm_amd import gs as lgs
from lgm_amd import sh as lsh
from lgm_amd._native import ptr
from lgm_amd.cameras import orbit_cameras
from lgm_amd.gs import forward_state, rasterize
from tests import render_sh_ref as S
from tests.alloc_guard import guarded
from tests.render_cases import PRECISION, TAN, grad_bar, rel_l2, scene, upstream

pytestmark = pytest.mark.gpu

H, W = 40, 56  # not multiples of the 16-pixel tile
GROUPS = {"mean": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11),
          "sh_dc": slice(11, 14), "sh_rest": slice(14, None)}
E_WORKSPACE = -2  # include/lgm_common.h LGM_E_WORKSPACE


def _case(g, cv, cvp, h, w, grads=True, **kw):
    d_img, d_dep, d_alp, bg = upstream(1, cv.shape[1], h, w)
    z = {"g": g, "cv": cv, "cvp": cvp, "bg": bg, "grads": (d_img, d_dep, d_alp)}
    gk = dict(d_image=d_img, d_depth=d_dep, d_alpha=d_alp) if grads else {}
    z["ref"] = S.render(g, cv, cvp, TAN, h, w, bg, **gk, **kw)
    if grads:
        z["r32"] = S.render(g, cv, cvp, TAN, h, w, bg, dtype=torch.float32, **gk, **kw)
    return z


@functools.lru_cache(maxsize=None)
def main_case(d):
    """The main scene at degree d with its references, computed once and left unchanged."""
    g14, cv, cvp = scene(N=1000, V=2, seed=3, shrink=1.0, scale_mul=2.0)
    return _case(S.lift(g14, d), cv, cvp, H, W)


def _run(cuda, z, h=H, w=W, grads=True, **kw):
    gd = z["g"].to(cuda).requires_grad_(grads)
    img, dep, alp = rasterize(gd, z["cv"].to(cuda), z["cvp"].to(cuda), z["bg"].to(cuda), TAN, TAN, h, w, **kw)
    out = {"image": img.detach().cpu().numpy(), "depth": dep.detach().cpu().numpy(),
           "alpha": alp.detach().cpu().numpy()}
    if grads:
        d_img, d_dep, d_alp = (t.to(cuda) for t in z["grads"])
        loss = (img * d_img).sum() + (dep * d_dep).sum() + (alp * d_alp).sum()
        loss.backward(retain_graph=True)
        out["d_gaussians"] = gd.grad.cpu().numpy().copy()
        out["loss"], out["gd"] = loss, gd
    torch.cuda.synchronize()
    return out


def _check_forward(out, z, tag):
    for k in ("image", "depth", "alpha"):
        e = rel_l2(out[k], z["ref"][k])
        print(tag, k, f"{e:.3e}")
        assert e <= 1e-4, (tag, k, e)


def _check_grads(out, z, tag):
    truth = z["ref"]["d_gaussians"]
    assert out["d_gaussians"].shape == truth.shape
    bad = []
    for name, sl in GROUPS.items():
        e_gpu = rel_l2(out["d_gaussians"][..., sl], truth[..., sl])
        e32 = rel_l2(z["r32"]["d_gaussians"][..., sl], truth[..., sl])
        bar = grad_bar(e32)
        print(f"{tag} d_{name}: GPU vs fp64 {e_gpu:.3e}, fp32 restatement vs fp64 {e32:.3e}, bar {bar:.3e}")
        PRECISION.append({"test": tag, "group": name, "e_gpu": e_gpu, "e_o32": e32, "bar": bar})
        if not e_gpu < bar:
            bad.append((name, e_gpu, bar))
    assert not bad, bad


@pytest.mark.parametrize("d", [1, 2, 3])
def test_forward(cuda, d):
    z = main_case(d)
    g = z["g"]
    dc_only = S.render(torch.cat([g[..., :14], torch.zeros_like(g[..., 14:])], -1), z["cv"], z["cvp"], TAN, H, W, z["bg"])
    diff, frac = rel_l2(z["ref"]["image"], dc_only["image"]), S.clamped_fraction(z["ref"])
    print(f"degree {d}: reference with rest vs DC only {diff:.3e}, clamped colours {frac:.3f}")
    assert diff >= 1e-2 and 0.05 <= frac <= 0.5  # sensitive by the reference alone
    out = _run(cuda, z, grads=False)
    _check_forward(out, z, f"sh{d}")
    assert np.array_equal(_run(cuda, z, grads=False, sh_degree=d)["image"], out["image"])


@pytest.mark.parametrize("det", [False, True], ids=["float", "deterministic"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_gradients(cuda, d, det):
    _check_grads(_run(cuda, main_case(d), deterministic=det), main_case(d), f"sh{d}-{'det' if det else 'float'}")


def test_deterministic_is_bitwise_reproducible(cuda):
    z = main_case(3)
    a, b = _run(cuda, z, deterministic=True), _run(cuda, z, deterministic=True)
    for k in ("image", "depth", "alpha", "d_gaussians"):
        assert np.array_equal(a[k], b[k]), k
    a["gd"].grad = None
    a["loss"].backward()  # a second backward of the same forward (LGM_RENDER_BACKWARD_AGAIN)
    assert np.array_equal(a["gd"].grad.cpu().numpy(), a["d_gaussians"])
    assert np.isfinite(a["d_gaussians"]).all()


def test_second_backward_in_float_mode(cuda):
    """The per-view colour partials are cleared with the rest: a repeated backward does not add to the first."""
    a = _run(cuda, main_case(3), deterministic=False)
    a["gd"].grad = None
    a["loss"].backward()
    again = a["gd"].grad.cpu().numpy()
    for name, sl in GROUPS.items():
        assert rel_l2(again[..., sl], a["d_gaussians"][..., sl]) <= 1e-5, name


def test_binning_does_not_see_the_colours(cuda):
    z = main_case(3)
    cv, cvp = z["cv"].to(cuda), z["cvp"].to(cuda)
    g3 = z["g"].to(cuda)
    g0 = lsh.sh_to_rgb(g3).contiguous()
    a = forward_state(g3, cv, cvp, TAN, TAN, H, W, lists=True)
    b = forward_state(g0, cv, cvp, TAN, TAN, H, W, lists=True)
    assert np.array_equal(a["radii"], b["radii"]) and np.array_equal(a["tile_counts"], b["tile_counts"])
    assert (a["K_binned"], a["K_reference"]) == (b["K_binned"], b["K_reference"]) and a["K_binned"] > 0
    for v in range(2):
        assert np.array_equal(a["ids"][0][v], b["ids"][0][v])
    # lgm_render_count_pairs takes the 14-wide copy of the rows: the same counts
    assert lgs.count_pairs(g3, cv, cvp, TAN, TAN, H, W) == lgs.count_pairs(g0, cv, cvp, TAN, TAN, H, W) == \
        (a["K_binned"], a["K_reference"])


@pytest.mark.parametrize("det", [False, True], ids=["float", "deterministic"])
def test_an_invisible_view_contributes_nothing(cuda, det):
    """V = 3, the third camera inside the cloud: the Gaussians behind its near cut get no colour and no gradient from
    it (their direction from that camera is as good as any other: a contribution would show in d_sh and d_mean)."""
    z = _invisible_case()
    vis = z["ref"]["vis"][0]
    cut = vis[0] & ~vis[2]
    print("visible per view", vis.sum(1), "visible in view 0 and cut in view 2:", int(cut.sum()))
    assert cut.sum() >= 100 and vis[2].sum() >= 100
    out = _run(cuda, z, deterministic=det)
    _check_forward(out, z, "sh3-invisible")
    _check_grads(out, z, f"sh3-invisible-{'det' if det else 'float'}")


@functools.lru_cache(maxsize=None)
def _invisible_case():
    g14, cv, cvp = scene(N=1000, V=2, seed=3, scale_mul=2.0)
    cv3, cvp3, _ = orbit_cameras(1, radius=0.25, azimuth_offset=40.0)
    return _case(S.lift(g14, 3), torch.cat([cv, cv3[None]], 1), torch.cat([cvp, cvp3[None]], 1), H, W)


def test_with_antialias(cuda):
    g14, cv, cvp = scene(N=1000, V=2, seed=3, scale_mul=2.0)
    z = _case(S.lift(g14, 3), cv, cvp, H, W, antialias=True)
    assert rel_l2(z["ref"]["image"], main_case(3)["ref"]["image"]) >= 1e-2  # (the scene feels both switches)
    out = _run(cuda, z, antialias=True, deterministic=True)
    _check_forward(out, z, "sh3-antialias")
    _check_grads(out, z, "sh3-antialias-det")


def test_with_clamp(cuda):
    g14, cv, cvp = scene(N=1000, V=2, seed=3, scale_mul=2.0)
    z = _case(S.lift(g14, 3), cv, cvp, H, W, clamp=True)
    unclamped = main_case(3)["ref"]["image"]
    assert float(((unclamped < 0) | (unclamped > 1)).mean()) >= 0.01  # (the clamp is active)
    out = _run(cuda, z, clamp=True)
    _check_forward(out, z, "sh3-clamp")
    _check_grads(out, z, "sh3-clamp-float")


def test_fused_loss(cuda):
    """rasterize(..., gt_images, gt_masks) on SH rows against rasterize plus torch's MSE terms on the same input."""
    Sz, V = 32, 3
    g14, cv, cvp = scene(N=500, V=V, seed=11, scale_mul=2.0)
    g0 = S.lift(g14, 2)
    gen = torch.Generator().manual_seed(12)
    gt = torch.rand(1, V, 3, Sz, Sz, generator=gen).to(cuda)
    mask = (torch.rand(1, V, 1, Sz, Sz, generator=gen) > 0.5).float().to(cuda)
    bg = torch.tensor([0.3, 0.6, 0.9], device=cuda)
    res = {}
    for fused in (True, False):
        g = g0.to(cuda).requires_grad_(True)
        kw = dict(gt_images=gt, gt_masks=mask) if fused else {}
        out = rasterize(g, cv.to(cuda), cvp.to(cuda), bg, TAN, TAN, Sz, Sz, clamp=True, **kw)
        if fused:
            loss4 = out[3]
            loss = loss4[0]
        else:
            gt_c = gt * mask + bg.view(1, 1, 3, 1, 1) * (1 - mask)
            mi, ma = F.mse_loss(out[0], gt_c), F.mse_loss(out[2], mask)
            loss, loss4 = mi + ma, torch.stack([mi + ma, mi, ma, -10 * torch.log10(mi)])
        loss.backward()
        res[fused] = (loss4.detach().cpu().numpy(), out[0].detach().cpu().numpy(), g.grad.cpu().numpy())
    dc = rasterize(lsh.sh_to_rgb(g0).to(cuda), cv.to(cuda), cvp.to(cuda), bg, TAN, TAN, Sz, Sz, clamp=True)[0]
    assert rel_l2(res[True][1], dc.cpu().numpy()) >= 1e-2  # the fused entry points honour the bits
    assert np.array_equal(res[True][1], res[False][1])
    assert np.allclose(res[True][0], res[False][0], rtol=1e-5, atol=0)
    for name, sl in GROUPS.items():
        e = rel_l2(res[True][2][..., sl], res[False][2][..., sl])
        print(name, f"{e:.3e}")
        assert e <= 1e-4, (name, e)


def test_packed_mode(cuda, monkeypatch):
    """No slot workspace allowed: the capacity counted from the 14-wide copy of the rows; packed equals slot."""
    z = main_case(3)
    a = _run(cuda, z, deterministic=True)
    monkeypatch.setattr(lgs, "_WS_BUDGET", 0)
    b = _run(cuda, z, deterministic=True)
    for k in ("image", "depth", "alpha", "d_gaussians"):
        assert np.array_equal(a[k], b[k]), k


def test_workspace(cuda):
    z = main_case(3)
    L = nat.lib()
    g, cv, cvp, bg = (z[k].to(cuda).contiguous() for k in ("g", "cv", "cvp", "bg"))
    B, N, V = 1, g.shape[1], 2
    sizes = {}
    for det in (0, nat.RENDER_DETERMINISTIC):
        for aa in (0, nat.RENDER_ANTIALIAS):
            o = det | aa
            base = L.lgm_render_workspace_size_opts(B, V, N, H, W, 0, o)
            if o == 0:
                assert base == L.lgm_render_workspace_size(B, V, N, H, W, 0)
            per = [L.lgm_render_workspace_size_opts(B, V, N, H, W, 0, o | (d << nat.RENDER_SH_SHIFT)) for d in (1, 2, 3)]
            # the regions do not depend on the degree: colours, masks, partials and 14-wide copies
            assert per[0] == per[1] == per[2] > base, (o, base, per)
            sizes[o] = (base, per[0])
    # a forward handed the smaller workspace: LGM_E_WORKSPACE and nothing launched
    small = sizes[0][0]
    ws = torch.empty(small, dtype=torch.uint8, device=cuda)
    outs = [torch.full((B, V, c, H, W), -7.0, device=cuda) for c in (3, 1, 1)]
    prof = nat.KernelProfiler()
    try:
        with prof:
            rc = L.lgm_render_forward(B, V, N, H, W, ptr(g), ptr(cv), ptr(cvp), ptr(bg), TAN, TAN, 1.0, ptr(outs[0]),
                                      ptr(outs[1]), ptr(outs[2]), None, ptr(ws), small, 0, None,
                                      3 << nat.RENDER_SH_SHIFT, nat.stream_of(cuda), nat.diag())
        torch.cuda.synchronize()
        assert rc == E_WORKSPACE and b"workspace" in L.lgm_last_error()
        assert prof.summary() == {}
    finally:
        prof.close()
    for o in outs:
        assert bool((o == -7.0).all())
    with pytest.raises(nat.NativeError):
        nat.call("lgm_render_backward", cuda, B, V, N, H, W, ptr(g), ptr(cv), ptr(cvp), ptr(bg), TAN, TAN, 1.0,
                 ptr(outs[0]), None, None, ptr(torch.empty_like(g)), None, ptr(ws), small, 0, 3 << nat.RENDER_SH_SHIFT)


@pytest.mark.parametrize("det", [False, True], ids=["float", "deterministic"])
def test_poisoned_allocations(cuda, det):
    """Degree-3 forward + backward with every allocation (the workspace included) filled with 0x00 and with 0xFF and
    red-zoned: outputs invariant (bitwise in deterministic mode), every red zone intact."""
    z = main_case(3)
    outs = []
    for fill in (0x00, 0xFF):
        with guarded(fill) as gd:
            outs.append(_run(cuda, z, deterministic=det))
        print(f"fill 0x{fill:02X}: {gd.n_allocations} allocations, {gd.zones_checked} red zones checked, "
              f"{len(gd.violations)} violated")
        assert gd.n_allocations >= 1
        gd.assert_clean()
    for k in ("image", "depth", "alpha"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.isfinite(outs[1]["d_gaussians"]).all()
    if det:
        assert np.array_equal(outs[0]["d_gaussians"], outs[1]["d_gaussians"])
    else:  # two orders of the same atomic sums
        for name, sl in GROUPS.items():
            assert rel_l2(outs[1]["d_gaussians"][..., sl], outs[0]["d_gaussians"][..., sl]) <= 1e-5, name
    _check_grads(outs[1], z, f"sh3-poisoned-{'det' if det else 'float'}")
