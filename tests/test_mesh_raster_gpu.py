"""The mesh rasteriser's kernels (include/lgm_meshraster.h, lgm_amd/csrc/meshraster.hip) on the GPU: the cases of
tests/test_mesh_raster.py against the numpy fp64 restatement tests/mesh_raster_ref.py, and what only the kernels have:
the launched kernel set, error rows that launch nothing, the non-finite gradient rule."""
import numpy as np
import pytest
import torch

from lgm_amd import _native as nat
from tests import mesh_raster_ref as R

pytestmark = pytest.mark.gpu
FORWARD = {"k_mr_project", "k_mr_vis", "k_mr_vis_big", "k_mr_shade"}
BACKWARD = {"k_mr_absmax", "k_mr_scatter", "k_mr_convert"}


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_forward_against_fp64(cuda, name):
    R.check_forward(name, cuda)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_against_fp64(cuda, name):
    R.check_backward(name, cuda)


@pytest.mark.parametrize("name", ["boxes_33x47", "hand_colour_40x72", "hand_texture_64x64", "nets_texels4_48x80"])
def test_adjoint_identity(cuda, name):
    R.check_adjoint(name, cuda)


def test_hand_scene_faces(cuda):
    R.check_hand_scene(cuda)


def test_camera_convention_shared_with_the_gaussian_renderer(cuda):
    R.check_camera_convention(cuda)


def test_fit_texture(cuda):
    R.check_fit_texture(cuda)


def test_kernels_agree_with_the_torch_path(cuda):
    """The torch path evaluates the header's fp32 operations in the kernels' order: on the non-ambiguous pixels the
    two draw the same faces, and where they do the images agree to the tolerance of the fp64 comparison."""
    from lgm_amd.meshraster import render_mesh
    for name in ("boxes_33x47", "nets_texels2_64x64"):
        mesh, cv, cvp, H, W, r64, _, _ = R.case(name)
        a = render_mesh(mesh, cv, cvp, H, W, R.BG)
        b = render_mesh(R.on(mesh, cuda), cv.to(cuda), cvp.to(cuda), H, W, R.BG)
        ok = torch.from_numpy(~r64["ambiguous"])
        assert torch.equal(a["face_id"][ok], b["face_id"].cpu()[ok])
        e_img, _ = R.self_difference(name)
        diff = (a["image"] - b["image"].cpu()).abs().amax(dim=1)[ok].max()
        print(f"{name}: kernels against the torch path {float(diff):.3e}")
        assert float(diff) <= 2 * e_img


def test_launched_kernels_and_errors_launch_nothing(cuda):
    from lgm_amd.meshraster import render_mesh
    mesh, cv, cvp, H, W, _, _, _ = R.case("hand_texture_40x72")
    m = R.on(mesh, cuda)
    prof = nat.KernelProfiler()
    try:
        with prof:
            p = m.texture.clone().requires_grad_(True)
            out = render_mesh(R.with_param(m, p), cv.to(cuda), cvp.to(cuda), H, W, R.BG)
            assert set(prof.summary()) == FORWARD
            out["image"].sum().backward()
            assert set(prof.summary()) == FORWARD | BACKWARD
            prof.reset()
            L = nat.lib()
            V, Nv, Nf, Nu = cv.shape[0], m.vertices.shape[0], m.faces.shape[0], m.uvs.shape[0]
            Ht, Wt = m.texture.shape[:2]
            ws, ws_bytes = nat.workspace("lgm_meshraster_workspace_size", cuda, V, Nv, Nf, H, W, Ht, Wt)
            image = torch.full((V, 3, H, W), 7.0, device=cuda)
            alpha = torch.full((V, 1, H, W), 7.0, device=cuda)
            args = [nat.ptr(m.vertices), Nv, nat.ptr(m.faces), Nf, nat.ptr(m.uvs), Nu, nat.ptr(m.face_uvs),
                    nat.ptr(m.texture), Ht, Wt, None, nat.ptr(cv.to(cuda)), nat.ptr(cvp.to(cuda)), V,
                    nat.ptr(torch.zeros(3, device=cuda)), H, W, nat.ptr(image), nat.ptr(alpha), None, None, nat.ptr(ws),
                    ws_bytes]
            for i, bad in ((22, ws_bytes - 1), (15, 0), (13, 0), (8, 0), (1, -1), (21, None), (17, None)):
                a = list(args)
                a[i] = bad
                with pytest.raises(nat.NativeError):
                    nat.call("lgm_meshraster_forward", cuda, *a)
            torch.cuda.synchronize()
            assert prof.summary() == {}, prof.summary()
            assert bool((image == 7).all()) and bool((alpha == 7).all())
    finally:
        prof.close()


def test_empty_mesh_is_background(cuda):
    from lgm_amd.mesh import Mesh
    from lgm_amd.meshraster import render_mesh
    cv, cvp = R.cameras([10.0], [20.0])
    m = Mesh(torch.zeros(0, 3, device=cuda), torch.zeros(0, 3, dtype=torch.int32, device=cuda),
             torch.zeros(0, 3, device=cuda))
    out = render_mesh(m, cv.to(cuda), cvp.to(cuda), 5, 7, R.BG)
    assert torch.equal(out["image"].cpu(), torch.tensor(R.BG).view(1, 3, 1, 1).expand(1, 3, 5, 7))
    assert not out["alpha"].any() and not out["depth"].any() and bool((out["face_id"] == -1).all())


def test_gradient_of_zero_and_of_non_finite(cuda):
    """amax == 0: zeros; an Inf or NaN anywhere in d_image: every element NaN (the header's rule)."""
    from lgm_amd.meshraster import render_mesh
    mesh, cv, cvp, H, W, _, _, _ = R.case("hand_colour_40x72")
    m = R.on(mesh, cuda)
    p = m.colors.clone().requires_grad_(True)
    image = render_mesh(R.with_param(m, p), cv.to(cuda), cvp.to(cuda), H, W, R.BG)["image"]
    g, = torch.autograd.grad(image, p, torch.zeros_like(image), retain_graph=True)
    assert bool((g == 0).all())
    d = torch.ones_like(image)
    d[1, 2, 3, 4] = float("inf")
    g, = torch.autograd.grad(image, p, d, retain_graph=True)
    assert bool(torch.isnan(g).all())
    g, = torch.autograd.grad(image, p, torch.ones_like(image))  # and the workspace is still good for a third
    assert bool(torch.isfinite(g).all()) and float(g.sum()) > 0


def test_mesh_psnr_and_save_mesh_fit(cuda, tmp_path):
    from lgm_amd import GaussianRenderer, Options, mesh_psnr
    g = R.nets_gaussians().to(cuda)
    opt = Options(output_size=64)
    cv, cvp = R.cameras([-23.0, 37.0], [11.0, 161.0])
    path = str(tmp_path / "fit.obj")
    mesh = GaussianRenderer(opt).save_mesh(g[None], path, resolution=24, texels=2, fit_iters=3, fit_resolution=64)
    assert mesh.fit["iters"] == 3 and (tmp_path / "fit.png").exists() and (tmp_path / "fit.mtl").exists()
    p = mesh_psnr(mesh, g, opt, cv.to(cuda), cvp.to(cuda), 64, 64)
    assert np.isfinite(p) and 0 < p < 60


def test_optional_outputs_may_be_null(cuda):
    """depth and face_id NULL: the image and alpha are those of a call that asks for everything."""
    from lgm_amd.meshraster import render_mesh
    mesh, cv, cvp, H, W, _, _, _ = R.case("hand_texture_40x72")
    m = R.on(mesh, cuda)
    cvd, cvpd, bg = cv.to(cuda), cvp.to(cuda), torch.tensor(R.BG, device=cuda)
    want = render_mesh(m, cvd, cvpd, H, W, R.BG)
    V, Nv, Nf, Nu = cv.shape[0], m.vertices.shape[0], m.faces.shape[0], m.uvs.shape[0]
    Ht, Wt = m.texture.shape[:2]
    ws, ws_bytes = nat.workspace("lgm_meshraster_workspace_size", cuda, V, Nv, Nf, H, W, Ht, Wt)
    image = torch.empty(V, 3, H, W, device=cuda)
    alpha = torch.empty(V, 1, H, W, device=cuda)
    nat.call("lgm_meshraster_forward", cuda, nat.ptr(m.vertices), Nv, nat.ptr(m.faces), Nf, nat.ptr(m.uvs), Nu,
             nat.ptr(m.face_uvs), nat.ptr(m.texture), Ht, Wt, None, nat.ptr(cvd), nat.ptr(cvpd), V, nat.ptr(bg), H, W,
             nat.ptr(image), nat.ptr(alpha), None, None, nat.ptr(ws), ws_bytes)
    assert torch.equal(image, want["image"]) and torch.equal(alpha, want["alpha"])
