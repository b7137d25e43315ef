"""The antialias switch (include/lgm_render.h LGM_RENDER_ANTIALIAS) on the GPU, against the fp64 dense restatement
tests/render_aa_ref.py (pinned to the frozen oracle with the switch off by tests/test_render_antialias_cpu.py).

Bars: forward outputs 1e-4 rel L2 (the project's forward bar); gradients per parameter group
render_cases.grad_bar(e32) = max(1e-4, 1.25 x e32), e32 the fp32 restatement's own error against fp64 on the same
inputs; everything said to be equal is equal bit for bit. The scene is chosen sensitive to the switch by the
reference alone (asserted in test_forward): scene(N=1000, V=2, seed=3, scale_mul=2.0) at 40 x 56 has 77 % of its
visible records at s < 0.8 and the reference's two images 7.4e-2 apart.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lgm_amd import GaussianRenderer, Options
from lgm_amd import _native as nat
from lgm_amd import gs as lgs
from lgm_amd._native import ptr
from lgm_amd.cameras import orbit_cameras
from lgm_amd.gs import forward_state, rasterize
from tests import render_aa_ref as R
from tests.render_cases import PRECISION, TAN, grad_bar, rel_l2, scene, upstream

pytestmark = pytest.mark.gpu

H, W = 40, 56  # not multiples of the 16-pixel tile
GROUPS = {"mean": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11), "rgb": slice(11, 14)}


def _references(g, cv, cvp, h, w, grads, bg):
    kw = dict(d_image=grads[0], d_depth=grads[1], d_alpha=grads[2])
    return {"ref": R.render(g, cv, cvp, TAN, h, w, bg, antialias=True, **kw),
            "r32": R.render(g, cv, cvp, TAN, h, w, bg, dtype=torch.float32, antialias=True, **kw)}


@pytest.fixture(scope="module")
def case():
    """The main scene with its references, computed once and left unchanged."""
    g, cv, cvp = scene(N=1000, V=2, seed=3, shrink=1.0, scale_mul=2.0)
    d_img, d_dep, d_alp, bg = upstream(1, 2, H, W)
    z = {"g": g, "cv": cv, "cvp": cvp, "bg": bg, "grads": (d_img, d_dep, d_alp)}
    z.update(_references(g, cv, cvp, H, W, z["grads"], bg))
    z["plain"] = R.render(g, cv, cvp, TAN, H, W, bg, antialias=False)
    return z


def _run(cuda, z, h=H, w=W, grads=True, antialias=True, **kw):
    gd = z["g"].to(cuda).requires_grad_(grads)
    img, dep, alp = rasterize(gd, z["cv"].to(cuda), z["cvp"].to(cuda), z["bg"].to(cuda), TAN, TAN, h, w,
                              antialias=antialias, **kw)
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


def _check_grads(out, z, tag):
    truth = z["ref"]["d_gaussians"]
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


def test_forward(cuda, case):
    ref, plain = case["ref"], case["plain"]
    vis = ref["vis"]
    frac = float((ref["s"][vis] < 0.8).mean())
    diff = rel_l2(ref["image"], plain["image"])
    print(f"visible records {int(vis.sum())}, s < 0.8 in {frac:.3f}, reference on vs off {diff:.3e}")
    assert frac >= 0.25 and diff >= 1e-2  # sensitive by the reference alone
    out = _run(cuda, case, grads=False)
    for k in ("image", "depth", "alpha"):
        e = rel_l2(out[k], ref[k])
        print(k, f"{e:.3e}")
        assert e <= 1e-4, (k, e)


def test_flag_is_used(cuda, case):
    on, off = _run(cuda, case, grads=False), _run(cuda, case, grads=False, antialias=False)
    assert rel_l2(on["image"], off["image"]) >= 1e-2
    assert rel_l2(off["image"], case["plain"]["image"]) <= 1e-4


@pytest.mark.parametrize("det", [False, True], ids=["float", "deterministic"])
def test_gradients(cuda, case, det):
    _check_grads(_run(cuda, case, deterministic=det), case, f"antialias-{'det' if det else 'float'}")


def test_deterministic_is_bitwise_reproducible(cuda, case):
    a, b = _run(cuda, case, deterministic=True), _run(cuda, case, deterministic=True)
    for k in ("image", "depth", "alpha", "d_gaussians"):
        assert np.array_equal(a[k], b[k]), k
    a["gd"].grad = None
    a["loss"].backward()  # a second backward of the same forward (LGM_RENDER_BACKWARD_AGAIN)
    assert np.array_equal(a["gd"].grad.cpu().numpy(), a["d_gaussians"])
    assert np.isfinite(a["d_gaussians"]).all()


def test_second_backward_in_float_mode(cuda, case):
    """The per-view opacity partial is cleared with the rest: a repeated backward does not add to the first."""
    a = _run(cuda, case, deterministic=False)
    a["gd"].grad = None
    a["loss"].backward()
    again = a["gd"].grad.cpu().numpy()
    for name, sl in GROUPS.items():
        assert rel_l2(again[..., sl], a["d_gaussians"][..., sl]) <= 1e-5, name


def _lists(fs, v):
    counts = fs["tile_counts"][0, v]
    return np.split(fs["ids"][0][v], np.cumsum(counts)[:-1])


def _is_subsequence(sub, full):
    it = iter(full.tolist())
    return all(x in it for x in sub.tolist())


def test_tile_lists(cuda, case):
    g, cv, cvp = (case[k].to(cuda) for k in ("g", "cv", "cvp"))
    st = {(aa, nc): forward_state(g, cv, cvp, TAN, TAN, H, W, lists=True, no_cull=nc, antialias=aa)
          for aa in (False, True) for nc in (False, True)}
    on, off = st[(True, True)], st[(False, True)]
    assert np.array_equal(on["radii"], off["radii"]) and np.array_equal(on["tile_counts"], off["tile_counts"])
    assert np.array_equal(st[(True, False)]["radii"], off["radii"])
    for v in range(2):
        assert np.array_equal(on["ids"][0][v], off["ids"][0][v])
        for t, (sub, full) in enumerate(zip(_lists(st[(True, False)], v), _lists(on, v))):
            assert _is_subsequence(sub, full), (v, t)
    # the compensated opacity can only cull more (include/lgm_render.h: the packed capacity rests on it)
    assert st[(True, False)]["K_binned"] <= st[(False, False)]["K_binned"] <= off["K_binned"]
    print("binned pairs: antialias", st[(True, False)]["K_binned"], "plain", st[(False, False)]["K_binned"])


def test_culling_is_output_preserving(cuda, case):
    for det in (False, True):
        a, b = _run(cuda, case, deterministic=det), _run(cuda, case, deterministic=det, no_cull=True)
        for k in ("image", "depth", "alpha"):
            assert np.array_equal(a[k], b[k]), k
        if det:
            assert np.array_equal(a["d_gaussians"], b["d_gaussians"])
        else:  # two orders of the same atomic sums
            for name, sl in GROUPS.items():
                assert rel_l2(a["d_gaussians"][..., sl], b["d_gaussians"][..., sl]) <= 1e-5, name


def _record_errors(cuda, case):
    g, cv, cvp = (case[k].to(cuda) for k in ("g", "cv", "cvp"))
    fs = forward_state(g, cv, cvp, TAN, TAN, H, W, records=True, antialias=True)
    vis = (fs["rects"][..., 0] & 0xffff) != (fs["rects"][..., 1] & 0xffff)
    assert np.array_equal(vis, case["ref"]["vis"])
    ref = case["ref"]
    err = np.abs(fs["Q"][..., 1].astype(np.float64)[vis] - np.log2(ref["opacity"][vis]))
    e32 = np.abs(np.log2(case["r32"]["opacity"][vis].astype(np.float64)) - np.log2(ref["opacity"][vis]))
    return err, e32, ref["cond"][vis], ref["s"][vis]


def test_records_hold_the_compensated_opacity(cuda, case):
    """lgm_render_records' L against log2(o s_ref) within 2e-6 on the visible records (measured 6.1e-7).

    What the bar asks of the code: det0 = a0 c0 - b^2 cancels for an elongated splat (a0 c0 / det0 reaches 500 on this
    scene), so a factor formed in fp32 is up to 3.6e-5 away on 40 of the 1,929 records -- the fp32 restatement
    itself 9.8e-5 -- whereas the factor pass evaluates it in fp64 (render_bin.hip k_aa_factor)."""
    err, e32, cond, _ = _record_errors(cuda, case)
    print("max |L - log2(o s_ref)|", float(err.max()), "records over 2e-6:", int((err > 2e-6).sum()), "of", err.size,
          "; fp32 restatement: max", float(e32.max()), "over 2e-6:", int((e32 > 2e-6).sum()),
          "; largest a0 c0 / det0", float(cond[np.isfinite(cond)].max()))
    assert float(err.max()) <= 2e-6


def test_records_within_the_rounding_of_the_formula(cuda, case):
    """The same records against a bound that follows the fp32 formula's own rounding: a0, b, c0 each come out of four
    stages of fp32 sums of products (J, T = W J, Sigma T, T . Sigma T), ~10 units of 2^-24 relative each; det0 = a0
    c0 - b^2 then carries ~40 x 2^-24 a0 c0, i.e. 40 x 2^-24 x cond relative in r (cond = a0 c0 / det0), and L = log2(o)
    + log2(r) / 2 moves by that over 2 ln 2: 29 x 2^-24 x cond, on top of the 2e-6 of a well-conditioned record. A
    factor that is ignored, or formed from a - 0.3, is orders of magnitude outside it; the fp64 factor pass is at 0.14
    of it, its fp32 predecessor was at 0.29."""
    err, _, cond, s = _record_errors(cuda, case)
    assert float((s < 0.8).mean()) >= 0.25
    open_ = s > 0.00501  # (under the floor L is log2(0.005 o): no amplification)
    bound = 2e-6 + np.where(open_, 29 * 2.0 ** -24 * np.where(np.isfinite(cond), cond, 0), 0)
    worst = float((err / bound).max())
    print("largest error over its bound:", worst)
    assert worst <= 1


def _forward_abi(cuda, z, cap, options):
    """lgm_render_forward called directly: (image, depth, alpha, stats) with the given pair capacity."""
    g, cv, cvp, bg = (z[k].to(cuda).contiguous() for k in ("g", "cv", "cvp", "bg"))
    B, N, V = g.shape[0], g.shape[1], cv.shape[1]
    ws, ws_bytes = nat.workspace("lgm_render_workspace_size_opts", cuda, B, V, N, H, W, cap, options)
    out = [torch.empty(B, V, c, H, W, device=cuda) for c in (3, 1, 1)]
    stats = torch.zeros(2, dtype=torch.int64, device=cuda)
    nat.call("lgm_render_forward", cuda, B, V, N, H, W, ptr(g), ptr(cv), ptr(cvp), ptr(bg), TAN, TAN, 1.0,
             ptr(out[0]), ptr(out[1]), ptr(out[2]), None, ptr(ws), ws_bytes, cap, ptr(stats), options)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], stats.tolist()


def test_packed_mode(cuda, case, monkeypatch):
    """Capacity from count_pairs (which knows no options) holds an antialiased forward; packed equals slot."""
    count = lgs.count_pairs(case["g"].to(cuda), case["cv"].to(cuda), case["cvp"].to(cuda), TAN, TAN, H, W)[0]
    packed, stats = _forward_abi(cuda, case, count, nat.RENDER_ANTIALIAS)
    slot, stats_slot = _forward_abi(cuda, case, 0, nat.RENDER_ANTIALIAS)
    print("count_pairs", count, "antialiased forward binned", stats[0])
    assert 0 < stats[0] <= count and stats == stats_slot
    for p, s in zip(packed, slot):
        assert np.array_equal(p, s)
    # and through rasterize: no slot workspace allowed -> counted capacity, forward and backward
    a = _run(cuda, case, deterministic=True)
    monkeypatch.setattr(lgs, "_WS_BUDGET", 0)
    b = _run(cuda, case, deterministic=True)
    for k in ("image", "depth", "alpha", "d_gaussians"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["image"], packed[0])


def test_fused_loss(cuda):
    """render(..., gt_images, gt_masks, antialias=True) against the unfused render plus torch's MSE terms."""
    S, V = 32, 3
    g0, cv, cvp = scene(N=500, V=V, seed=11, scale_mul=2.0)
    gen = torch.Generator().manual_seed(12)
    gt = torch.rand(1, V, 3, S, S, generator=gen).to(cuda)
    mask = (torch.rand(1, V, 1, S, S, generator=gen) > 0.5).float().to(cuda)
    bg = torch.tensor([0.3, 0.6, 0.9], device=cuda)
    r = GaussianRenderer(Options(output_size=S))
    cp = torch.zeros(1, V, 3, device=cuda)
    res = {}
    for fused in (True, False):
        g = g0.to(cuda).requires_grad_(True)
        kw = dict(gt_images=gt, gt_masks=mask) if fused else {}
        out = r.render(g, cv.to(cuda), cvp.to(cuda), cp, bg_color=bg, antialias=True, **kw)
        if fused:
            loss = out["loss_mse"]
        else:
            gt_c = gt * mask + bg.view(1, 1, 3, 1, 1) * (1 - mask)
            loss = F.mse_loss(out["image"], gt_c) + F.mse_loss(out["alpha"], mask)
        loss.backward()
        res[fused] = (float(loss.detach()), out["image"].detach().cpu().numpy(), g.grad.cpu().numpy())
    plain = r.render(g0.to(cuda), cv.to(cuda), cvp.to(cuda), cp, bg_color=bg)["image"].cpu().numpy()
    assert rel_l2(res[True][1], plain) >= 1e-2  # the fused entry points honour the bit
    assert np.array_equal(res[True][1], res[False][1])
    assert abs(res[True][0] / res[False][0] - 1) <= 1e-5
    for name, sl in GROUPS.items():
        e = rel_l2(res[True][2][..., sl], res[False][2][..., sl])
        print(name, f"{e:.3e}")
        assert e <= 1e-4, (name, e)
    # Options.antialias is what render reads when the argument is left out
    r2 = GaussianRenderer(Options(output_size=S, antialias=True))
    img = r2.render(g0.to(cuda), cv.to(cuda), cvp.to(cuda), cp, bg_color=bg)["image"].cpu().numpy()
    assert np.array_equal(img, res[False][1])


@pytest.mark.parametrize("det", [False, True], ids=["float", "deterministic"])
def test_more_views_than_the_lds_staging_holds(cuda, det):
    """V = 33 > 32: k_preproc_bwd without the LDS-staged matrices (the main scene runs the staged one)."""
    h = w = 16
    g, cv, cvp = scene(N=64, V=33, seed=5, scale_mul=2.0)
    d_img, d_dep, d_alp, bg = upstream(1, 33, h, w)
    z = {"g": g, "cv": cv, "cvp": cvp, "bg": bg, "grads": (d_img, d_dep, d_alp)}
    z.update(_references(g, cv, cvp, h, w, z["grads"], bg))
    out = _run(cuda, z, h, w, deterministic=det)
    for k in ("image", "depth", "alpha"):
        assert rel_l2(out[k], z["ref"][k]) <= 1e-4, k
    _check_grads(out, z, f"antialias-33-views-{'det' if det else 'float'}")


def _single(scales, opacity, rgb=(1.0, 0.5, 0.25)):
    cv, cvp, _ = orbit_cameras(1)
    g = torch.zeros(1, 1, 14)
    g[0, 0, 3] = opacity
    g[0, 0, 4:7] = torch.as_tensor(scales, dtype=torch.float32)
    g[0, 0, 7] = 1.0
    g[0, 0, 11:14] = torch.tensor(rgb)
    return g, cv[None], cvp[None], float(cv[0, 3, 2])


@pytest.mark.parametrize("det", [False, True], ids=["float", "deterministic"])
def test_edge_cases(cuda, det):
    S = 32
    fx = S / (2.0 * TAN)
    bg = torch.tensor([0.1, 0.2, 0.3])
    grads = upstream(1, 1, S, S)[:3]
    # (1) an edge-on disc, det0 / det <= 2.5e-5 (s = 0.005), next to ordinary Gaussians, one of them with an opacity
    # that the compensation brings under 1/255: everything finite, and equal to the reference
    g, cv, cvp, z = _single([0.1, 1e-6, 0.1], 0.9)
    g2 = scene(N=40, V=1, seed=2, scale_mul=2.0)[0]
    g2[0, 0, 3] = 0.004
    gg = torch.cat([g, g2], 1)
    zc = {"g": gg, "cv": cv, "cvp": cvp, "bg": bg, "grads": grads}
    ref = R.render(gg, cv, cvp, TAN, S, S, bg, antialias=True, d_image=grads[0], d_depth=grads[1], d_alpha=grads[2])
    assert ref["vis"][0, 0, 0] and abs(float(ref["s"][0, 0, 0]) - 0.005) <= 1e-9
    assert ref["vis"][0, 0, 1] and ref["opacity"][0, 0, 1] <= 1 / 255 < 0.004
    out = _run(cuda, zc, S, S, deterministic=det)
    for k in ("image", "depth", "alpha", "d_gaussians"):
        assert np.isfinite(out[k]).all(), k
    for k in ("image", "depth", "alpha"):
        assert rel_l2(out[k], ref[k]) <= 1e-4, k
    assert rel_l2(out["d_gaussians"][..., 11:14], ref["d_gaussians"][..., 11:14]) <= 1e-4
    # (2) o > 1/255 >= o^: a sub-pixel Gaussian (sigma^2 = 0.04 px^2, s = 0.118) of opacity 0.02 is drawn without the
    # switch and contributes nothing with it -- the image is the background and its colour gradient is zero
    g, cv, cvp, z = _single([1.0, 1.0, 1.0], 0.02)
    g[0, 0, 4:7] = 0.2 * z / fx
    zc = {"g": g, "cv": cv, "cvp": cvp, "bg": bg, "grads": grads}
    off = _run(cuda, zc, S, S, antialias=False, deterministic=det)
    on = _run(cuda, zc, S, S, deterministic=det)
    assert float(off["alpha"].max()) > 1 / 255 and float(np.abs(off["d_gaussians"][..., 11:14]).max()) > 0
    assert float(on["alpha"].max()) == 0 and np.array_equal(on["image"][0, 0], np.broadcast_to(
        bg.numpy()[:, None, None], (3, S, S)))
    assert np.array_equal(on["d_gaussians"], np.zeros_like(on["d_gaussians"]))
