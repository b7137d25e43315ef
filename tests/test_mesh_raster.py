"""render_mesh, fit_texture and mesh_psnr (lgm_amd/meshraster.py) on the CPU: the dense torch path against the numpy
fp64 restatement of include/lgm_meshraster.h (tests/mesh_raster_ref.py), and the C ABI's error rows (nothing is
launched, so they need no GPU)."""
import numpy as np
import pytest
import torch

from lgm_amd import _native as nat
from tests import mesh_raster_ref as R

CPU = torch.device("cpu")


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_forward_against_fp64(name):
    R.check_forward(name, CPU)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_against_fp64(name):
    R.check_backward(name, CPU)


@pytest.mark.parametrize("name", ["boxes_33x47", "hand_colour_40x72", "hand_texture_64x64", "nets_texels4_48x80"])
def test_adjoint_identity(name):
    R.check_adjoint(name, CPU)


def test_hand_scene_faces():
    R.check_hand_scene(CPU)


def test_camera_convention_shared_with_the_gaussian_renderer():
    R.check_camera_convention(CPU)


def test_fit_texture():
    R.check_fit_texture(CPU)


def test_mesh_psnr_and_arguments():
    from lgm_amd import Options, fit_texture, mesh_psnr, render_mesh
    mesh, g = R.nets_mesh(2), R.nets_gaussians()
    cv, cvp = R.cameras([-23.0, 37.0], [11.0, 161.0])
    p = mesh_psnr(mesh, g, Options(), cv, cvp, 32, 32)
    assert np.isfinite(p) and 0 < p < 60
    out = render_mesh(mesh, cv, cvp, 32, 32)
    assert out["image"].shape == (2, 3, 32, 32) and out["face_id"].dtype == torch.int32
    with pytest.raises(ValueError):
        render_mesh(mesh, cv[0], cvp[0], 32, 32)
    with pytest.raises(ValueError):
        render_mesh(mesh, cv, cvp, 0, 32)
    with pytest.raises(ValueError):
        fit_texture(R.hand_scene(False), g, Options(), iters=1)  # no texture to fit
    from lgm_amd.mesh import gaussians_to_mesh
    with pytest.raises(ValueError):
        gaussians_to_mesh(g, resolution=24, fit_iters=2)  # needs texels


def test_empty_mesh_is_background():
    from lgm_amd.mesh import Mesh
    from lgm_amd.meshraster import render_mesh
    cv, cvp = R.cameras([10.0], [20.0])
    m = Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3))
    out = render_mesh(m, cv, cvp, 5, 7, R.BG)
    assert torch.equal(out["image"], torch.tensor(R.BG).view(1, 3, 1, 1).expand(1, 3, 5, 7))
    assert not out["alpha"].any() and not out["depth"].any() and (out["face_id"] == -1).all()


def error_rows():
    """(name, forward arguments) of every error row of include/lgm_meshraster.h. Pointers are a dummy address: an
    entry point that reports an error launches nothing and reads nothing."""
    P = 0x1000
    ok = dict(vertices=P, Nv=4, faces=P, Nf=2, uvs=P, Nu=4, face_uvs=P, texture=P, Ht=4, Wt=4, colors=None, cam_view=P,
              cam_view_proj=P, V=1, bg=P, H=8, W=8, image=P, alpha=P, depth=None, face_id=None, ws=P, ws_bytes=None)
    rows = [("null " + k, dict(ok, **{k: None})) for k in ("vertices", "faces", "uvs", "face_uvs", "cam_view",
                                                          "cam_view_proj", "bg", "image", "alpha", "ws")]
    rows.append(("null colors", dict(ok, texture=None, colors=None)))
    rows += [("Nv < 0", dict(ok, Nv=-1)), ("Nf < 0", dict(ok, Nf=-1)), ("Nu < 0", dict(ok, Nu=-1)),
             ("3 Nv >= 2^31", dict(ok, Nv=2 ** 31 // 3 + 1)), ("3 Nf >= 2^31", dict(ok, Nf=2 ** 31 // 3 + 1)),
             ("2 Nu >= 2^31", dict(ok, Nu=2 ** 30)), ("3 V H W >= 2^31", dict(ok, V=4, H=16384, W=16384)),
             ("V Nf >= 2^31", dict(ok, V=64, Nf=2 ** 25)), ("3 Ht Wt >= 2^31", dict(ok, Ht=32768, Wt=32768)),
             ("H < 1", dict(ok, H=0)), ("W < 1", dict(ok, W=0)), ("V < 1", dict(ok, V=0)), ("Ht < 1", dict(ok, Ht=0)),
             ("Wt < 1", dict(ok, Wt=0)), ("short workspace", dict(ok, ws_bytes=-1))]
    return rows


@pytest.mark.parametrize("name,a", error_rows(), ids=[r[0] for r in error_rows()])
def test_error_rows(name, a):
    L = nat.lib()
    size = L.lgm_meshraster_workspace_size(a["V"], a["Nv"], a["Nf"], a["H"], a["W"], a["Ht"], a["Wt"])
    ws_bytes = max(size - 1, 0) if a["ws_bytes"] == -1 else (size or 1 << 20)
    rc = L.lgm_meshraster_forward(a["vertices"], a["Nv"], a["faces"], a["Nf"], a["uvs"], a["Nu"], a["face_uvs"],
                                  a["texture"], a["Ht"], a["Wt"], a["colors"], a["cam_view"], a["cam_view_proj"], a["V"],
                                  a["bg"], a["H"], a["W"], a["image"], a["alpha"], a["depth"], a["face_id"], a["ws"],
                                  ws_bytes, None, None)
    assert rc < 0 and L.lgm_last_error(), name
    if name == "short workspace":
        assert rc == -2
    if name in ("null colors", "null vertices", "null cam_view", "null cam_view_proj", "null bg", "null image",
                "null alpha"):
        return
    # the backward's rows: the same sizes, its own pointers
    d_tex = 0x1000 if a["texture"] else None
    rc = L.lgm_meshraster_backward(a["Nv"], a["faces"], a["Nf"], a["uvs"], a["Nu"], a["face_uvs"], a["Ht"], a["Wt"],
                                   a["V"], a["H"], a["W"], 0x1000, d_tex, None if d_tex else 0x1000, a["ws"], ws_bytes,
                                   None, None)
    assert rc < 0 and L.lgm_last_error(), name


def test_backward_null_rows_and_sizes():
    L = nat.lib()
    size = L.lgm_meshraster_workspace_size(1, 4, 2, 8, 8, 4, 4)
    assert size > 0 and L.lgm_meshraster_workspace_size(1, 4, 2, 8, 8, 0, 0) > 0
    assert L.lgm_meshraster_workspace_size(0, 4, 2, 8, 8, 0, 0) == 0
    assert L.lgm_meshraster_workspace_size(1, 4, 2, 8, 8, 8, 8) > size  # the texture's accumulators
    P = 0x1000
    assert L.lgm_meshraster_backward(4, P, 2, P, 4, P, 4, 4, 1, 8, 8, None, P, None, P, size, None, None) < 0  # d_image
    assert L.lgm_meshraster_backward(4, P, 2, None, 0, None, 0, 0, 1, 8, 8, P, None, None, P, size, None, None) < 0
    # the fixed-point unit: V H W pixels of fewer than 2^(S + 1) units each stay below 2^62
    assert L.lgm_meshraster_unit_log2(8, 512, 512) == 40 and L.lgm_meshraster_unit_log2(1, 1, 1) == 61
    for V, H, W in ((1, 1, 1), (2, 40, 72), (3, 333, 77), (8, 512, 512), (1, 16384, 16384)):
        S = L.lgm_meshraster_unit_log2(V, H, W)
        assert V * H * W * 2 ** (S + 1) <= 2 ** 62 < V * H * W * 2 ** (S + 2), (V, H, W, S)
    assert L.lgm_meshraster_unit_log2(0, 8, 8) < 0
