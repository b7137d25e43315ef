"""k_render_bwd takes each chunk's quadrant masks from the forward (one byte per list position, kept in the dead half
of the tile's pair range) instead of testing every entry again. What that could break, each on the smallest scene
that reaches it:
  - lists of many 64-entry chunks with checkpoint items (a mask byte per position, across chunk and item boundaries);
  - launches of >= 4,096 tiles, whose work items span two forward chunks;
  - batched vs alone and a second backward of the same forward (the masks live in the saved workspace);
  - short and empty tiles, packed tile ranges (the masks' offset is 4 n past the tile's own base);
  - a poisoned, red-zoned workspace (the backward reads no byte the forward did not write).
Gradients against the fp64 oracle at the usual bar (tests/render_cases.grad_bar: 1.25 x the fp32 oracle's own error,
1e-4 always accepted); the deterministic mode's bitwise.

The scenes: most Gaussians drawn into a small central cluster with opacity <= 0.02, so the central tiles' lists run
to a thousand entries without saturating a pixel (every chunk is composited and walked back), plus a sparse halo of
40 ordinary Gaussians for short and empty tiles."""
import numpy as np
import pytest
import torch

from lgm_amd import gs as lgs
from lgm_amd.gs import forward_state, rasterize
from tests.alloc_guard import guarded
from tests.render_cases import PRECISION, TAN, grad_bar, rel_l2, scene, upstream

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
GROUPS = {"mean": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11), "rgb": slice(11, 14)}
HALO = 40


def _clustered(B, N, V, H, seed, shrink):
    g, cv, cvp = scene(B=B, N=N, V=V, seed=seed, elevation=10.0)
    g[:, HALO:, 0:3] *= shrink
    g[:, HALO:, 3] = g[:, HALO:, 3].clamp(max=0.02)
    d_img, _, d_alpha, bg = upstream(B, V, H, H, seed=seed + 1)
    # deterministic mode scales its fixed point by the power of two of the CALL's largest upstream gradient: one
    # pinned value per scene gives a scene rendered alone the scale it has inside the batch (the N(0, 1) maxima
    # straddle 4.0: 3.97 in scene 0 of "long64", 4.09 in scene 1)
    d_img[:, 0, 0, 0, 0] = 5.0
    return {"g": g, "cv": cv, "cvp": cvp, "H": H, "bg": bg, "d_img": d_img, "d_alpha": d_alpha}


_CASES = {
    "long64": lambda: _clustered(2, 4000, 2, 64, 11, 0.3),     # 16 tiles per view, the central four very long
    "ragged128": lambda: _clustered(2, 4000, 2, 128, 11, 0.3),  # 64 tiles per view: long, short and empty ones
    "wide256": lambda: _clustered(1, 3000, 6, 256, 12, 0.1),    # one scene of the >= 4,096-tile launch
}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _CASES[name]()
    return _cache[name]


def oracle_of(O, name):
    """(fp32 oracle outputs, fp64 gradients) of a case, computed once."""
    z = case(name)
    if "ref" not in z:
        a = (z["g"].numpy(), z["cv"].numpy(), z["cvp"].numpy(), TAN, z["H"], z["H"], z["bg"].numpy())
        kw = {"d_image": z["d_img"].numpy(), "d_alpha": z["d_alpha"].numpy()}
        z["ref"] = O.render(*a, **kw)
        z["truth"] = O.render(*a, f64=True, **kw)["d_gaussians"]
    return z["ref"], z["truth"]


def run(cuda, z, det, sl=slice(None), copies=1, backwards=1):
    """Forward + backward(s) of image and alpha; `copies` repeats the scenes along the batch."""
    def dev(t):
        t = t[sl]
        return t.repeat(copies, *([1] * (t.dim() - 1))).to(cuda)
    gd = dev(z["g"]).requires_grad_(True)
    img, _, alp = rasterize(gd, dev(z["cv"]), dev(z["cvp"]), z["bg"].to(cuda), TAN, TAN, z["H"], z["H"],
                            deterministic=det)
    grads = [torch.autograd.grad([img, alp], gd, [dev(z["d_img"]), dev(z["d_alpha"])],
                                 retain_graph=k + 1 < backwards)[0].cpu().numpy() for k in range(backwards)]
    torch.cuda.synchronize()
    return {"image": img.detach().cpu().numpy(), "alpha": alp.detach().cpu().numpy(), "d_gaussians": grads[0],
            "d_gaussians_again": grads[-1]}


def check(O, name, out, label, sl=slice(None)):
    ref, truth = oracle_of(O, name)
    for k in ("image", "alpha"):
        e = rel_l2(out[k], ref[k][sl])
        assert e < FWD_TOL, f"{label} {k}: rel L2 {e:.3e}"
    rec = {}
    for grp, cs in GROUPS.items():
        e_gpu = rel_l2(out["d_gaussians"][..., cs], truth[sl][..., cs])
        e_o32 = rel_l2(ref["d_gaussians"][sl][..., cs], truth[sl][..., cs])
        rec[grp] = {"gpu": e_gpu, "fp32_oracle": e_o32, "bar": grad_bar(e_o32)}
        print(f"{label} d_{grp}: GPU vs fp64 {e_gpu:.3e}, fp32 oracle {e_o32:.3e}, bar {rec[grp]['bar']:.3e}")
    PRECISION.append({"test": label, "groups": rec})
    for grp, r in rec.items():
        assert r["gpu"] < r["bar"], f"{label} d_{grp}: GPU vs fp64 {r['gpu']:.3e}, fp32 oracle {r['fp32_oracle']:.3e}"


def tile_state(cuda, z, copies=1):
    g, cv, cvp = (z[k].repeat(copies, *([1] * (z[k].dim() - 1))).to(cuda) for k in ("g", "cv", "cvp"))
    st = forward_state(g, cv, cvp, TAN, TAN, z["H"], z["H"], lists=True)
    return st["tile_counts"], st["n_contrib"]


@pytest.mark.parametrize("det", [False, True], ids=["float", "deterministic"])
def test_multi_chunk_lists_and_checkpoints(cuda, oracle_mod, det):
    """64^2, 2 x 2 views: the longest list exceeds 600 entries and is composited beyond its second 256-entry chunk
    (several 64-entry chunks per work item, and in float mode a checkpoint item per 256-entry boundary)."""
    z = case("long64")
    counts, n_contrib = tile_state(cuda, z)
    print("longest list", counts.max(), "deepest contributor", n_contrib.max())
    assert counts.max() > 600
    assert n_contrib.max() > 512
    check(oracle_mod, "long64", run(cuda, z, det), f"masks long64 ({'deterministic' if det else 'float'})")


def test_two_chunk_items(cuda, oracle_mod):
    """3 x 6 views at 256^2 = 4,608 tiles: the launch form whose backward work items span two forward chunks (512
    positions), float mode (the deterministic one takes no checkpoint items). Every copy against the oracle."""
    z = case("wide256")
    assert 3 * 6 * (256 // 16) ** 2 >= 4096
    counts, n_contrib = tile_state(cuda, z, copies=3)
    print("longest list", counts.max(), "deepest contributor", n_contrib.max())
    assert counts.max() > 512
    assert n_contrib.max() > 512
    out = run(cuda, z, False, copies=3)
    for s in range(3):
        check(oracle_mod, "wide256", {k: v[s:s + 1] for k, v in out.items()}, f"masks two-chunk items, copy {s}")


def test_batched_equals_alone(cuda):
    z = case("long64")
    both = run(cuda, z, True)
    for s in range(2):
        alone = run(cuda, z, True, sl=slice(s, s + 1))
        for k in ("image", "alpha", "d_gaussians"):
            assert np.array_equal(both[k][s:s + 1], alone[k]), f"scene {s}: {k} differs batched vs alone"


def test_second_backward_finds_the_masks(cuda):
    out = run(cuda, case("long64"), True, backwards=2)
    assert np.array_equal(out["d_gaussians"], out["d_gaussians_again"])
    assert np.abs(out["d_gaussians"]).max() > 0


def test_short_and_empty_tiles_slot_and_packed(cuda, oracle_mod, monkeypatch):
    """128^2: lists of over 600 entries next to tiles of fewer than 64 entries and empty ones, in the slot workspace
    and in the packed one (exact pair count, tile ranges back to back: a mask byte written past a tile's own range
    would land in its neighbour's ids)."""
    z = case("ragged128")
    counts, _ = tile_state(cuda, z)
    print("tile counts: max", counts.max(), "empty", int((counts == 0).sum()), "1..63",
          int(((counts > 0) & (counts < 64)).sum()))
    assert counts.max() > 600 and (counts == 0).any() and ((counts > 0) & (counts < 64)).any()
    outs = {}
    for mode, budget in (("slot", None), ("packed", 0)):
        monkeypatch.setattr(lgs, "_WS_BUDGET", budget)
        outs[mode] = run(cuda, z, True)
        outs[mode + "_float"] = run(cuda, z, False)
    for k in ("image", "alpha", "d_gaussians"):
        assert np.array_equal(outs["slot"][k], outs["packed"][k]), k
    check(oracle_mod, "ragged128", outs["packed"], "masks ragged128 packed (deterministic)")
    check(oracle_mod, "ragged128", outs["packed_float"], "masks ragged128 packed (float)")
    check(oracle_mod, "ragged128", outs["slot_float"], "masks ragged128 slot (float)")


@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["zeros", "ones"])
def test_poisoned_workspace(cuda, fill):
    """Every allocation of the call (the workspace included) filled with `fill` and red-zoned: finite gradients,
    bitwise those of the plain run in deterministic mode, every red zone intact. A mask byte the forward had not
    written would read as no quadrant (0x00: a contributor dropped) or as all four."""
    z = case("long64")
    plain = run(cuda, z, True)
    with guarded(fill) as gd:
        out = run(cuda, z, True)
    print(f"fill 0x{fill:02X}: {gd.n_allocations} allocations, {gd.zones_checked} red zones checked, "
          f"{len(gd.violations)} violated")
    assert gd.n_allocations >= 1
    gd.assert_clean()
    assert np.isfinite(out["d_gaussians"]).all()
    for k in ("image", "alpha", "d_gaussians"):
        assert np.array_equal(out[k], plain[k]), k
