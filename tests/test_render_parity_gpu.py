"""GPU parity of the PRODUCTION render configuration and bit-exact integer parity of the binning.

Production configuration = what LGM (core/models.py:141-153) and bench.py call: GaussianRenderer.render (the
image clamped in-kernel as core/gs.py:87) and a backward of image and alpha only (d_depth is None, so
k_render_bwd<false> runs, the kernel the benchmark times). The oracle is given torch's clamp gradient explicitly:
d_image is masked where the fp64 forward's unclamped image lies outside [0, 1] (inclusive bounds, torch's
clamp backward); pixels within 1e-5 of a bound are given zero upstream gradient on both sides, so an fp32
rounding of the image across the bound cannot flip the mask between the two implementations.

Integer parity (bit-exact, no tolerance): per view the GPU's radii equal the oracle's, the reference pair count
K (upstream's num_rendered) equals the oracle's, and with exact culling disabled (LGM_RENDER_NO_CULL) every
tile's sorted id list and every pixel's n_contrib equal the oracle's. With culling on, every GPU tile list is the
oracle's list with the provably-skipped pairs removed, in the same order.

Tolerances for floats are those of tests/test_render_gpu.py (forward 1e-4 rel L2; gradients within
max(1e-4, 1.25 x the fp32 oracle's own error) of fp64; the GPU's distance to the fp32 oracle itself is
recorded beside it).
"""
import glob
import os

import numpy as np
import pytest
import torch

from lgm_amd import GaussianRenderer, Options, _native
from lgm_amd.gs import forward_state
from lgm_amd.synthetic import synthetic_gaussians, synthetic_upstream_grads
from lgm_amd.cameras import orbit_cameras
from tests.render_cases import PRECISION, TAN, grad_bar, rel_l2, scene, upstream

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
BWD_TOL = 1e-4
BOUND_EPS = 1e-5  # pixels this close to a clamp bound get zero upstream gradient on both sides
GROUPS = {"mean": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11), "rgb": slice(11, 14)}
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "render_*.npz")))


def _clamp_masked_grads(O, g, cv, cvp, H, W, bg, d_img, mod=1.0):
    """The upstream image gradient after torch's clamp(0, 1) backward, from the fp64 forward's unclamped image;
    near-bound pixels zeroed."""
    ref = O.render(g.numpy(), cv.numpy(), cvp.numpy(), TAN, H, W, bg.numpy(), scale_modifier=mod, f64=True)
    img = ref["image"]
    inside = (img >= 0.0) & (img <= 1.0)
    near = (np.abs(img) < BOUND_EPS) | (np.abs(img - 1.0) < BOUND_EPS)
    return torch.from_numpy((d_img.numpy() * (inside & ~near)).astype(np.float32)), \
        torch.from_numpy((~near).astype(np.float32))


def _production(cuda, g, cv, cvp, H, W, bg, d_img, d_alpha, keep, mod=1.0):
    """GaussianRenderer.render + backward of image and alpha (LGM's loss inputs) on the GPU."""
    opt = Options(output_size=H)
    r = GaussianRenderer(opt)
    gd = g.to(cuda).requires_grad_(True)
    cp = torch.zeros(cv.shape[0], cv.shape[1], 3, device=cuda)
    out = r.render(gd, cv.to(cuda), cvp.to(cuda), cp, bg_color=bg.to(cuda), scale_modifier=mod)
    assert set(out) >= {"image", "alpha"}
    # keep: near-bound pixels excluded from the loss (their clamp mask is rounding-ambiguous)
    torch.autograd.backward([out["image"], out["alpha"]], [d_img.to(cuda) * keep.to(cuda), d_alpha.to(cuda)])
    torch.cuda.synchronize()
    return {"image": out["image"].detach().cpu().numpy(), "alpha": out["alpha"].detach().cpu().numpy(),
            "d_gaussians": gd.grad.cpu().numpy()}


def _check(O, out, g, cv, cvp, H, W, bg, d_img_masked, d_alpha, mod=1.0, name=None):
    ref = O.render(g.numpy(), cv.numpy(), cvp.numpy(), TAN, H, W, bg.numpy(), scale_modifier=mod,
                   d_image=d_img_masked.numpy(), d_alpha=d_alpha.numpy())
    truth = O.render(g.numpy(), cv.numpy(), cvp.numpy(), TAN, H, W, bg.numpy(), scale_modifier=mod,
                     d_image=d_img_masked.numpy(), d_alpha=d_alpha.numpy(), f64=True)["d_gaussians"]
    e = rel_l2(out["image"], np.clip(ref["image"], 0.0, 1.0))
    assert e < FWD_TOL, f"image: rel L2 {e:.3e}"
    e = rel_l2(out["alpha"], ref["alpha"])
    assert e < FWD_TOL, f"alpha: rel L2 {e:.3e}"
    rec = {}
    for grp, sl in GROUPS.items():
        e_gpu = rel_l2(out["d_gaussians"][..., sl], truth[..., sl])
        e_o32 = rel_l2(ref["d_gaussians"][..., sl], truth[..., sl])
        rec[grp] = {"gpu": e_gpu, "fp32_oracle": e_o32, "bar": grad_bar(e_o32, BWD_TOL),
                    "gpu_vs_fp32_oracle": rel_l2(out["d_gaussians"][..., sl], ref["d_gaussians"][..., sl])}
    if name:
        PRECISION.append({"test": name, "groups": rec})
    for grp, r in rec.items():
        assert r["gpu"] < r["bar"], f"d_{grp}: GPU vs fp64 {r['gpu']:.3e}, fp32 oracle {r['fp32_oracle']:.3e}"


PROD_CASES = [
    # B, N, V, H, mod, elevation, stretch colours outside [0, 1] (exercises the clamp)
    (1, 300, 2, 64, 1.0, 0.0, False),
    (2, 2000, 3, 64, 1.0, 15.0, False),
    (1, 3000, 2, 48, 0.7, -20.0, True),
    (2, 1500, 2, 128, 1.3, 20.0, True),
    (1, 8000, 4, 128, 1.0, -15.0, True),
]


@pytest.mark.parametrize("B,N,V,H,mod,elev,stretch", PROD_CASES)
def test_production_render_parity(cuda, oracle_mod, B, N, V, H, mod, elev, stretch):
    g, cv, cvp = scene(B=B, N=N, V=V, seed=N + V + 3, elevation=elev)
    if stretch:
        g[..., 11:14] = g[..., 11:14] * 2.2 - 0.6
    d_img, _, d_alpha, bg = upstream(B, V, H, H, seed=N)
    d_m, keep = _clamp_masked_grads(oracle_mod, g, cv, cvp, H, H, bg, d_img, mod)
    out = _production(cuda, g, cv, cvp, H, H, bg, d_img, d_alpha, keep, mod)
    _check(oracle_mod, out, g, cv, cvp, H, H, bg, d_m, d_alpha, mod)


def test_production_cfg3_bench_inputs(cuda, oracle_mod):
    """BASELINE config 3 with bench.py's exact inputs: scene seed 1 (rank 0), upstream gradients seed 1001."""
    g = synthetic_gaussians(1, 100_000, seed=1)
    cv, cvp, _ = orbit_cameras(6)
    cv, cvp = cv[None], cvp[None]
    d_img, _, d_alpha, bg = synthetic_upstream_grads(1, 6, 256, 256, seed=1001)
    d_m, keep = _clamp_masked_grads(oracle_mod, g, cv, cvp, 256, 256, bg, d_img)
    out = _production(cuda, g, cv, cvp, 256, 256, bg, d_img, d_alpha, keep)
    _check(oracle_mod, out, g, cv, cvp, 256, 256, bg, d_m, d_alpha, name="cfg3 bench inputs (production path)")


def test_production_cfg4_512(cuda, oracle_mod):
    """BASELINE config 4's render: N = 6 x 160^2 = 153,600 Gaussians at 512^2 (1,024 tiles per view). The batched
    call renders 4 of the 20 orbit views (the oracle's fp64 check bounds the test's run time); production path."""
    g = synthetic_gaussians(1, 153_600, seed=4)
    cv, cvp, _ = orbit_cameras(20)
    sel = [0, 3, 11, 17]
    cv, cvp = cv[None, sel], cvp[None, sel]
    d_img, _, d_alpha, bg = synthetic_upstream_grads(1, len(sel), 512, 512, seed=44)
    d_m, keep = _clamp_masked_grads(oracle_mod, g, cv, cvp, 512, 512, bg, d_img)
    out = _production(cuda, g, cv, cvp, 512, 512, bg, d_img, d_alpha, keep)
    _check(oracle_mod, out, g, cv, cvp, 512, 512, bg, d_m, d_alpha, name="cfg4 512^2, 4 views (production path)")


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[7:-4])
def test_golden_fixture(cuda, oracle_mod, path):
    """Each committed fixture (tests/golden/render_*.npz, elevated cameras included): forward vs its stored
    outputs, gradients (with its stored d_depth) vs its stored fp32 oracle gradient within max(1e-4, 1.25 x that
    gradient's own error against a live fp64 evaluation)."""
    from lgm_amd.gs import rasterize
    z = np.load(path)
    g = torch.from_numpy(z["gaussians"])
    H, W = int(z["H"]), int(z["W"])
    tan, mod = float(z["tanfov"]), float(z["scale_modifier"])
    gd = g.to(cuda).requires_grad_(True)
    img, dep, alp = rasterize(gd, torch.from_numpy(z["cam_view"]).to(cuda), torch.from_numpy(z["cam_view_proj"]).to(cuda),
                              torch.from_numpy(z["bg"]).to(cuda), tan, tan, H, W, mod)
    loss = (img * torch.from_numpy(z["d_image"]).to(cuda)).sum() + (dep * torch.from_numpy(z["d_depth"]).to(cuda)).sum() \
        + (alp * torch.from_numpy(z["d_alpha"]).to(cuda)).sum()
    loss.backward()
    torch.cuda.synchronize()
    for k, t in (("image", img), ("depth", dep), ("alpha", alp)):
        e = rel_l2(t.detach().cpu().numpy(), z[k])
        assert e < FWD_TOL, f"{k}: rel L2 {e:.3e}"
    truth = oracle_mod.render(z["gaussians"], z["cam_view"], z["cam_view_proj"], tan, H, W, z["bg"], mod,
                              d_image=z["d_image"], d_depth=z["d_depth"], d_alpha=z["d_alpha"], f64=True)["d_gaussians"]
    dg = gd.grad.cpu().numpy()
    for name, sl in GROUPS.items():
        e_gpu = rel_l2(dg[..., sl], truth[..., sl])
        e_fix = rel_l2(z["d_gaussians"][..., sl], truth[..., sl])
        assert e_gpu < grad_bar(e_fix, BWD_TOL), f"d_{name}: {e_gpu:.3e} vs fixture {e_fix:.3e}"


# ---------------------------------------------------------------------------------------------- integer parity
INT_CASES = {
    "cfg2": dict(N=50_000, V=1, H=256, seed=0, elevation=0.0),
    "cfg3": dict(N=100_000, V=6, H=256, seed=1, elevation=0.0),
    "elevated": dict(N=20_000, V=3, H=128, seed=5, elevation=20.0),
    "ragged": dict(N=7_000, V=2, H=72, seed=6, elevation=-15.0),
}


def _ties_scene():
    g, cv, cvp = scene(N=3000, V=1, seed=3000)
    g[..., 2] = 0.0  # a flat layer facing the azimuth-0 camera: every depth equal, order decided by id
    g[..., 0:2] *= 0.6
    return g, cv, cvp


def _case(name):
    if name == "ties":
        g, cv, cvp = _ties_scene()
        return g, cv, cvp, 48
    c = INT_CASES[name]
    g, cv, cvp = scene(N=c["N"], V=c["V"], seed=c["seed"], elevation=c["elevation"])
    return g, cv, cvp, c["H"]


@pytest.mark.parametrize("name", list(INT_CASES) + ["ties"])
def test_integer_parity_radii_and_K(cuda, oracle_mod, name):
    g, cv, cvp, H = _case(name)
    st = forward_state(g.to(cuda), cv.to(cuda), cvp.to(cuda), TAN, TAN, H, H)
    V = cv.shape[1]
    K_sum = 0
    for v in range(V):
        pre = oracle_mod.preprocess(g[0].numpy(), cv[0, v].numpy(), cvp[0, v].numpy(), TAN, H, H)
        bad = np.nonzero(st["radii"][0, v] != pre["radii"])[0]
        assert bad.size == 0, f"view {v}: {bad.size} radii differ, e.g. ids {bad[:8]}"
        K_sum += pre["K"]
    assert st["K_reference"] == K_sum, (st["K_reference"], K_sum)
    assert st["K_binned"] == int(st["tile_counts"].sum())


@pytest.mark.parametrize("name", list(INT_CASES) + ["ties"])
def test_integer_parity_tile_lists(cuda, oracle_mod, name):
    """NO_CULL: the GPU's tile lists and n_contrib ARE the oracle's (upstream's 3-sigma rects). Culled (the
    product default): each GPU list is an in-order subsequence of the oracle's."""
    g, cv, cvp, H = _case(name)
    V = cv.shape[1]
    full = forward_state(g.to(cuda), cv.to(cuda), cvp.to(cuda), TAN, TAN, H, H, lists=True, no_cull=True)
    culled = forward_state(g.to(cuda), cv.to(cuda), cvp.to(cuda), TAN, TAN, H, H, lists=True)
    T = full["tile_counts"].shape[-1]
    nc_mismatch = 0
    for v in range(V):
        ts, ids = oracle_mod.tile_lists(g[0].numpy(), cv[0, v].numpy(), cvp[0, v].numpy(), TAN, H, H)
        counts = np.diff(ts)
        assert np.array_equal(full["tile_counts"][0, v], counts), f"view {v}: tile counts differ"
        assert np.array_equal(full["ids"][0][v], ids), f"view {v}: sorted tile lists differ"
        # culled lists: in-order subsequences of the full ones
        cc = culled["tile_counts"][0, v]
        assert np.all(cc <= counts)
        off_c = np.concatenate([[0], np.cumsum(cc)])
        for t in range(T):
            sub = culled["ids"][0][v][off_c[t]:off_c[t + 1]]
            lst = ids[ts[t]:ts[t + 1]]
            idx = {int(x): k for k, x in enumerate(lst)}
            ks = np.array([idx.get(int(x), -1) for x in sub])
            assert np.all(ks >= 0) and np.all(np.diff(ks) > 0), f"view {v} tile {t}: not an in-order subsequence"
        nc, _, _ = oracle_mod.forward_state(g[0].numpy(), cv[0, v].numpy(), cvp[0, v].numpy(), TAN, H, H)
        nc_mismatch += int((full["n_contrib"][0, v] != nc).sum())
    # n_contrib depends on the 1/255 and T < 1e-4 decisions, i.e. on exp(): the GPU evaluates
    # v_exp_f32(A' dx^2 + B' dx dy + C' dy^2 + log2(opacity)) on the pre-scaled records (render_common.h), the
    # oracle opacity * libm expf(power). The two agree to ~1e-6 relative in alpha, so a decision flips only where
    # alpha lands within ~1e-6 of 1/255 (or T of 1e-4): measured 0-4 pixels of 2k-393k.
    npix = V * H * H
    print(f"{name}: n_contrib differs at {nc_mismatch} of {npix} pixels")
    assert nc_mismatch <= max(4, npix // 50_000), f"{nc_mismatch} of {npix} pixels differ in n_contrib"


def test_exact_count_path_matches_slot_path_512(cuda, monkeypatch):
    """The packed workspace (exact pair count first, one host sync; taken when the slot workspace exceeds the
    budget) gives the slot path's results bit for bit, at cfg4's 512^2 (1,024 tiles per view) with 5 of the 20
    views: the forward always, the gradients in deterministic mode (order-independent fixed-point accumulation, so
    only the tile-list addressing differs between the two runs). (A float-atomic comparison of the two is a draw
    of the accumulation order: ill-conditioned rotation gradients of needle-like Gaussians then differ by up to
    ~1e-3 relative between ANY two runs, slot or packed.)"""
    from lgm_amd import gs as lgs
    g = synthetic_gaussians(1, 153_600, seed=4)
    cv, cvp, _ = orbit_cameras(20)
    cv, cvp = cv[None, 0:20:4].contiguous(), cvp[None, 0:20:4].contiguous()
    V = cv.shape[1]
    d_img, _, d_alpha, bg = synthetic_upstream_grads(1, V, 512, 512, seed=45)
    keep = torch.ones(1)
    monkeypatch.setenv("LGM_AMD_DETERMINISTIC", "1")
    outs = []
    for budget in (None, 0):
        monkeypatch.setattr(lgs, "_WS_BUDGET", budget)
        outs.append(_production(cuda, g, cv, cvp, 512, 512, bg, d_img, d_alpha, keep))
    slot, packed = outs
    for k in ("image", "alpha", "d_gaussians"):
        assert np.array_equal(slot[k], packed[k]), k
    monkeypatch.setenv("LGM_AMD_DETERMINISTIC", "0")
    monkeypatch.setattr(lgs, "_WS_BUDGET", 0)  # the packed path with float atomics: same forward, bit for bit
    fl = _production(cuda, g, cv, cvp, 512, 512, bg, d_img, d_alpha, keep)
    for k in ("image", "alpha"):
        assert np.array_equal(slot[k], fl[k]), k
    # the float-atomic path's own spread at this scale (recorded): two float runs (packed, slot)
    # against each other and against the order-independent deterministic gradients
    monkeypatch.setattr(lgs, "_WS_BUDGET", None)
    fl2 = _production(cuda, g, cv, cvp, 512, 512, bg, d_img, d_alpha, keep)
    rec = {}
    for grp, sl in GROUPS.items():
        rec[grp] = {"float_packed_vs_float_slot": rel_l2(fl["d_gaussians"][..., sl], fl2["d_gaussians"][..., sl]),
                    "float_vs_deterministic": rel_l2(fl2["d_gaussians"][..., sl], slot["d_gaussians"][..., sl])}
    PRECISION.append({"test": "cfg4 512^2, 5 views: float-atomic accumulation-order spread", "groups": rec})
    # with the fp64 side accumulators for needle-like records the default float path sits at the flat 1e-4 bar
    # (measured r03/s5: rot 5.5e-6 packed vs slot, 6.1e-5 vs deterministic; round 2 had 8.5e-4)
    for grp, r in rec.items():
        for k, v in r.items():
            assert v <= BWD_TOL, f"d_{grp} {k}: {v:.3e} > {BWD_TOL:.0e}"


def test_deterministic_backward(cuda, oracle_mod):
    """LGM_RENDER_DETERMINISTIC (int64 fixed-point accumulators): two backwards of the same inputs are bitwise
    equal, and within the gradient bar of the fp64 oracle (cfg3 with bench.py's inputs, production path)."""
    from lgm_amd.gs import rasterize
    g = synthetic_gaussians(1, 100_000, seed=1)
    cv, cvp, _ = orbit_cameras(6)
    cv, cvp = cv[None], cvp[None]
    d_img, _, d_alpha, bg = synthetic_upstream_grads(1, 6, 256, 256, seed=1001)
    d_m, keep = _clamp_masked_grads(oracle_mod, g, cv, cvp, 256, 256, bg, d_img)
    tan = TAN
    grads = []
    for _ in range(2):
        gd = g.to(cuda).requires_grad_(True)
        img, _, alp = rasterize(gd, cv.to(cuda), cvp.to(cuda), bg.to(cuda), tan, tan, 256, 256, clamp=True,
                                deterministic=True)
        torch.autograd.backward([img, alp], [d_img.to(cuda) * keep.to(cuda), d_alpha.to(cuda)])
        grads.append(gd.grad.clone())
    torch.cuda.synchronize()
    assert torch.equal(grads[0], grads[1])
    out = {"image": img.detach().cpu().numpy(), "alpha": alp.detach().cpu().numpy(),
           "d_gaussians": grads[0].cpu().numpy()}
    _check(oracle_mod, out, g, cv, cvp, 256, 256, bg, d_m, d_alpha, name="cfg3 bench inputs (deterministic mode)")


@pytest.mark.parametrize("det", [True, False])
def test_needles_512_vs_fp32_oracle(cuda, oracle_mod, det):
    """cfg4's 512^2 (153,600 Gaussians, 5 of the 20 views), whose mean / scale / rotation gradient errors are carried
    by a few needle-like footprints (conic condition 1e3-2e4: the cov2D inverse amplifies any rounding of their conic
    gradients). The backward's moment MFMAs split w / u into round-to-nearest bf16 hi + lo parts (unbiased, <= 2^-17
    per product; the truncated split sat near 2x the oracle's error here, profiles/r03/diag_float_spread):
    both accumulation modes at or below the fp32 oracle's own error vs fp64 in those groups (measured 0.36-0.44x in
    both: the float mode's needle conic partials are summed in fp64), the other groups within the usual bar."""
    g = synthetic_gaussians(1, 153_600, seed=4)
    cv, cvp, _ = orbit_cameras(20)
    cv, cvp = cv[None, 0:20:4].contiguous(), cvp[None, 0:20:4].contiguous()
    V = cv.shape[1]
    d_img, _, d_alpha, bg = synthetic_upstream_grads(1, V, 512, 512, seed=45)
    d_m, keep = _clamp_masked_grads(oracle_mod, g, cv, cvp, 512, 512, bg, d_img)
    os.environ["LGM_AMD_DETERMINISTIC"] = "1" if det else "0"
    try:
        out = _production(cuda, g, cv, cvp, 512, 512, bg, d_img, d_alpha, keep)
    finally:
        os.environ.pop("LGM_AMD_DETERMINISTIC", None)
    ref = oracle_mod.render(g.numpy(), cv.numpy(), cvp.numpy(), TAN, 512, 512, bg.numpy(), d_image=d_m.numpy(),
                            d_alpha=d_alpha.numpy())
    truth = oracle_mod.render(g.numpy(), cv.numpy(), cvp.numpy(), TAN, 512, 512, bg.numpy(), d_image=d_m.numpy(),
                              d_alpha=d_alpha.numpy(), f64=True)["d_gaussians"]
    rec = {}
    for grp, sl in GROUPS.items():
        e_gpu = rel_l2(out["d_gaussians"][..., sl], truth[..., sl])
        e_o32 = rel_l2(ref["d_gaussians"][..., sl], truth[..., sl])
        rec[grp] = {"gpu": e_gpu, "fp32_oracle": e_o32, "bar": e_o32 if grp in ("mean", "scale", "rot")
                    else grad_bar(e_o32, BWD_TOL),
                    "gpu_vs_fp32_oracle": rel_l2(out["d_gaussians"][..., sl], ref["d_gaussians"][..., sl])}
    PRECISION.append({"test": f"cfg4 512^2, 5 views, needle-dominated ({'deterministic' if det else 'float'} mode)",
                      "groups": rec})
    for grp, r in rec.items():
        assert r["gpu"] <= r["bar"], f"d_{grp}: GPU vs fp64 {r['gpu']:.3e}, fp32 oracle {r['fp32_oracle']:.3e}"


# ------------------------------------------------------------------------------------------- headline workload
def test_headline_pool_batched_equals_per_scene(cuda, oracle_mod):
    """bench.py's headline workload itself: the 8-scene scaling pool (seed 2, 100k Gaussians x 6 views
    x 256^2 per scene, upstream gradients seed 1002) rendered as ONE batched call, as at N = 1, equals the same
    scenes rendered one per call, as each rank renders its shard at N = 8: forward bit for bit, and in
    deterministic mode (order-independent fixed-point accumulation) the gradients bit for bit too. Scene 0 of the
    pool is checked against the oracle on the production path (clamp, image + alpha backward)."""
    from lgm_amd.gs import rasterize
    B, N, V, R = 8, 100_000, 6, 256
    pool = synthetic_gaussians(B, N, seed=2)
    cv, cvp, _ = orbit_cameras(V)
    d_img, _, d_alpha, bg = synthetic_upstream_grads(B, V, R, R, seed=1002)

    def run(g, c, cp, di, da):
        gd = g.to(cuda).requires_grad_(True)
        img, _, alp = rasterize(gd, c.to(cuda), cp.to(cuda), bg.to(cuda), TAN, TAN, R, R, clamp=True,
                                deterministic=True)
        torch.autograd.backward([img, alp], [di.to(cuda), da.to(cuda)])
        return img.detach(), alp.detach(), gd.grad

    cvb = cv[None].expand(B, -1, -1, -1).contiguous()
    cvpb = cvp[None].expand(B, -1, -1, -1).contiguous()
    img_b, alp_b, grad_b = run(pool, cvb, cvpb, d_img, d_alpha)
    for s in range(B):
        img_s, alp_s, grad_s = run(pool[s:s + 1], cv[None], cvp[None], d_img[s:s + 1], d_alpha[s:s + 1])
        assert torch.equal(img_b[s:s + 1], img_s), f"scene {s}: image differs batched vs alone"
        assert torch.equal(alp_b[s:s + 1], alp_s), f"scene {s}: alpha differs batched vs alone"
        assert torch.equal(grad_b[s:s + 1], grad_s), f"scene {s}: gradient differs batched vs alone"
    # scene 0 on the production (non-deterministic, float-atomic) path vs the oracle
    g0, c0, cp0 = pool[0:1], cv[None], cvp[None]
    d_m, keep = _clamp_masked_grads(oracle_mod, g0, c0, cp0, R, R, bg, d_img[0:1])
    out = _production(cuda, g0, c0, cp0, R, R, bg, d_img[0:1], d_alpha[0:1], keep)
    _check(oracle_mod, out, g0, c0, cp0, R, R, bg, d_m, d_alpha[0:1], name="pool scene 0 (production path)")


@pytest.mark.parametrize("H,W,N,seed", [(256, 256, 50_000, 3), (136, 200, 20_000, 4)])
def test_small_launch_form_bitwise(cuda, H, W, N, seed):
    """Launches of at most 256 tiles (one 256^2 view: BASELINE config 2) take k_render_fwd's small-launch form (8
    entries per step at 2 waves per SIMD), larger launches the 4-entry form at 7. The same (scene, view) rendered alone
    (256 / 117 tiles) and as every scene of a 6-scene batch (1,536 / 702 tiles): image, depth, alpha, n_contrib and
    final T bitwise equal, the backward's gradients bitwise equal in deterministic mode (so the forward left the same
    checkpoints and list bounds), and with the fused loss the same image."""
    from lgm_amd.gs import rasterize
    g = synthetic_gaussians(1, N, seed=seed)
    cv, cvp, _ = orbit_cameras(1)
    d_img, _, d_alpha, bg = synthetic_upstream_grads(1, 1, H, W, seed=seed + 100)
    d_dep = torch.randn(1, 1, 1, H, W, generator=torch.Generator().manual_seed(seed + 200))
    gen = torch.Generator().manual_seed(seed + 300)
    gt_img, gt_mask = torch.rand(1, 1, 3, H, W, generator=gen), (torch.rand(1, 1, 1, H, W, generator=gen) > 0.3).float()

    def rep(t, B):
        return t.expand(B, *t.shape[1:]).contiguous().to(cuda)

    def run(B):
        gd = rep(g, B).requires_grad_(True)
        img, dep, alp = rasterize(gd, rep(cv[None], B), rep(cvp[None], B), bg.to(cuda), TAN, TAN, H, W, clamp=True,
                                  deterministic=True)
        torch.autograd.backward([img, dep, alp], [rep(d_img, B), rep(d_dep, B), rep(d_alpha, B)])
        nc, ft = (forward_state(rep(g, B), rep(cv[None], B), rep(cvp[None], B), TAN, TAN, H, W)[k]
                  for k in ("n_contrib", "final_T"))
        with torch.no_grad():
            li = rasterize(rep(g, B), rep(cv[None], B), rep(cvp[None], B), bg.to(cuda), TAN, TAN, H, W, clamp=True,
                           gt_images=rep(gt_img, B), gt_masks=rep(gt_mask, B))
        torch.cuda.synchronize()
        return [img.detach(), dep.detach(), alp.detach(), gd.grad, torch.as_tensor(nc), torch.as_tensor(ft), li[0],
                li[3]]

    alone, batched = run(1), run(6)
    names = ["image", "depth", "alpha", "gradient", "n_contrib", "final_T", "image (fused loss)"]
    for s in range(6):
        for nm, a, b in zip(names, alone, batched):
            assert torch.equal(a[0].cpu(), b[s].cpu()), f"{H}x{W} scene {s}: {nm} differs small vs batched form"
    # the fused loss terms: one view vs six copies of it (sums in a different order: float tolerance)
    assert torch.allclose(alone[7].cpu(), batched[7].cpu(), rtol=1e-5, atol=0)


def test_two_chunk_items_float_path_vs_oracle(cuda, oracle_mod):
    """Launches of >= CK_LONG_TILES (4,096) tiles split the backward into work items of two forward chunks
    (render_common.h ck_shift_for; the 8-scene pool takes it). The production float path on such a launch -- the pool's
    scene 0 repeated three times, 4,608 tiles -- against the oracle for every copy (deterministic mode, which has no
    checkpoint items, cannot cover it)."""
    B, N, V, R = 3, 100_000, 6, 256
    g0 = synthetic_gaussians(1, N, seed=2)
    cv, cvp, _ = orbit_cameras(V)
    c0, cp0 = cv[None], cvp[None]
    d_img, _, d_alpha, bg = synthetic_upstream_grads(1, V, R, R, seed=1002)
    assert B * V * (R // 16) ** 2 >= 4096
    d_m, keep = _clamp_masked_grads(oracle_mod, g0, c0, cp0, R, R, bg, d_img)

    def rep(t):
        return t.expand(B, *t.shape[1:]).contiguous()

    out = _production(cuda, rep(g0), rep(c0), rep(cp0), R, R, bg, rep(d_img), rep(d_alpha), rep(keep))
    _check(oracle_mod, {k: v[0:1] for k, v in out.items()}, g0, c0, cp0, R, R, bg, d_m, d_alpha,
           name="two-chunk items, copy 0")
    for s in range(1, B):  # the other copies: the same forward bit for bit, the float-atomic gradients within 1e-5
        assert np.array_equal(out["image"][s], out["image"][0]) and np.array_equal(out["alpha"][s], out["alpha"][0])
        e = rel_l2(out["d_gaussians"][s], out["d_gaussians"][0])
        assert e < 1e-5, f"copy {s}: gradient rel L2 {e:.3e} vs copy 0"


def test_deterministic_checkpoint_split_independent_of_batch(cuda):
    """Deterministic mode on a scene whose tiles walk many chunks (72^2, long lists). The mode takes no backward
    checkpoints -- one work item per tile walks the whole list, so no split can depend on the launch's size or on
    which tiles won a shared pool -- and its int64 sums commute: scene 0's gradients are bitwise the same rendered
    alone and inside a batch of three (different work order, different timing), and the same again on a second run."""
    from lgm_amd.gs import rasterize
    g, cv, cvp = scene(B=3, N=7000, V=2, seed=6, elevation=-15.0)
    d_img, _, d_alpha, bg = upstream(3, 2, 72, 72, seed=8)

    def run(sl):
        gd = g[sl].to(cuda).requires_grad_(True)
        img, _, alp = rasterize(gd, cv[sl].to(cuda), cvp[sl].to(cuda), bg.to(cuda), TAN, TAN, 72, 72, clamp=True,
                                deterministic=True)
        torch.autograd.backward([img, alp], [d_img[sl].to(cuda), d_alpha[sl].to(cuda)])
        torch.cuda.synchronize()
        return gd.grad.cpu()

    alone = run(slice(0, 1))
    batched = run(slice(0, 3))
    assert torch.equal(alone[0], batched[0])
    assert torch.equal(run(slice(0, 1)), alone)
