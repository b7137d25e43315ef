"""The CPU path of the textured mesh export (lgm_amd.mesh: sample_field, mesh_atlas, bake_texture) against the numpy
restatement tests/mesh_texture_ref.py with the bars of the GPU file, and the writers: the textured OBJ with its .mtl and
.png, the untextured OBJ unchanged, save_mesh passing `texels` through."""
import os

import numpy as np
import pytest
import torch

import lgm_amd
from lgm_amd import mesh as M
from tests import mesh_ref as R
from tests import mesh_texture_ref as TR

CASES = sorted(TR.sample_cases())
TEXELS = (2, 4, 5)
_MESHES = {}


def cpu_mesh(name):
    """The CPU path's own mesh of an atlas case (computed once; the tests leave it unchanged)."""
    if name not in _MESHES:
        if name == "sphere":
            g, G, iso = R.one_gaussian(), (24, 24, 24), 0.3
        else:
            seed, N, G = R.E2E[name]
            g, iso = R.random_gaussians(seed, N), R.ISO
        gt = torch.from_numpy(g)
        _MESHES[name] = (g, G, M.gaussians_to_mesh(gt, G, iso))
    return _MESHES[name]


@pytest.mark.parametrize("name", CASES)
def test_sample_against_fp64(name):
    g, G, mod, pts = TR.sample_cases()[name]
    sigma, rgb = M.sample_field(torch.from_numpy(g), torch.from_numpy(pts), G, scale_modifier=mod)
    assert sigma.shape == (len(pts),) and rgb.shape == (len(pts), 3) and sigma.dtype == torch.float32
    TR.check_sample(sigma.numpy(), rgb.numpy(), TR.sample_reference(name), name)
    s2, none = M.sample_field(torch.from_numpy(g), torch.from_numpy(pts), G, scale_modifier=mod, colors=False)
    assert none is None and torch.equal(s2, sigma)


def test_sample_gap_between_bricks():
    """A cut that ends between node 7 and node 8 of a 24^3 grid: the density pass's lists would miss the first point."""
    g, G, pts = TR.GAP
    sigma, rgb = M.sample_field(torch.from_numpy(g), torch.from_numpy(pts), G)
    ref = TR.sample(g, pts, G)
    assert abs(ref[0][0] - 5.63e-4) < 1e-5 and ref[0][1] == 0
    TR.check_sample(sigma.numpy(), rgb.numpy(), ref, "gap")
    assert sigma[1] == 0 and sigma[0] > 5e-4


def test_sample_special_points_and_shapes():
    g, G, mod = R.density_cases()["ragged"]
    sp = TR.special_points(G)
    pts = np.concatenate(list(sp.values()))
    ref = TR.sample(g, pts, G)
    inside = dict(zip(sp, np.split(ref[3], np.cumsum([len(v) for v in sp.values()])[:-1])))
    assert inside["nodes"].all() and inside["inward"].all() and not inside["outward"].any() and not inside["bad"].any()
    sigma, rgb = M.sample_field(torch.from_numpy(g), torch.from_numpy(pts), G)
    TR.check_sample(sigma.numpy(), rgb.numpy(), ref, "special")
    # leading shapes are kept
    s2, c2 = M.sample_field(torch.from_numpy(g), torch.from_numpy(pts[:24].reshape(2, 3, 4, 3)), G)
    assert s2.shape == (2, 3, 4) and c2.shape == (2, 3, 4, 3) and torch.equal(s2.reshape(-1), sigma[:24])
    with pytest.raises(ValueError):
        M.sample_field(torch.from_numpy(g), torch.zeros(5, 2), G)


@pytest.mark.parametrize("name", ("ragged", "cube32", "sphere"))
def test_atlas_and_bake(name):
    g, G, mesh = cpu_mesh(name)
    V, F = mesh.vertices.numpy(), mesh.faces.numpy()
    assert len(F) // 2 == {"ragged": 448, "cube32": 946, "sphere": 192}[name]
    for T in TEXELS:
        points, uvs, face_uvs, shape = M.mesh_atlas(mesh, T)
        assert TR.check_atlas(points.numpy(), uvs.numpy(), face_uvs.numpy(), V, F, T) == shape
        baked = M.bake_texture(mesh, torch.from_numpy(g), T, resolution=G)
        assert baked.vertices is mesh.vertices and baked.faces is mesh.faces and baked.colors is mesh.colors
        assert torch.equal(baked.uvs, uvs.reshape(-1, 2)) and torch.equal(baked.face_uvs, face_uvs)
        TR.check_texture(baked.texture.numpy(), points.numpy(), TR.sample(g, points.numpy(), G), T, shape[0], shape[1])
        if name == "sphere":
            blocks = baked.texture.reshape(shape[1], T, shape[0], T, 3).permute(0, 2, 1, 3, 4).reshape(-1, T, T, 3)
            assert (blocks[:len(F) // 2] - torch.tensor([0.8, 0.4, 0.1])).abs().max() <= 1e-6


def test_bake_rejects_other_meshes_and_bakes_an_empty_one():
    g, G, mesh = cpu_mesh("sphere")
    gt = torch.from_numpy(g)
    F = mesh.faces
    broken = F.clone()
    broken[5, 0] = (broken[5, 0] + 1) % mesh.vertices.shape[0]  # faces 4 and 5 no longer start at the same q0
    diagonal = F.clone()
    diagonal[5, 1] = diagonal[5, 2] = diagonal[5, 0]  # ... no longer share the q0-q2 diagonal
    out_of_range = F.clone()
    out_of_range[7, 2] = mesh.vertices.shape[0]
    negative = F.clone()
    negative[0, 0] = -1
    for faces in (F[:-1], broken, diagonal, out_of_range, negative):
        with pytest.raises(ValueError):
            M.bake_texture(M.Mesh(mesh.vertices, faces, mesh.colors), gt, 4, resolution=G)
    with pytest.raises(ValueError):
        M.bake_texture(mesh, gt, 1, resolution=G)
    with pytest.raises(ValueError):
        M.atlas_shape(4097 * 4097, 4)  # 16,388 texels a side
    empty = M.gaussians_to_mesh(torch.zeros(0, 14), G, texels=4)
    assert empty.faces.shape[0] == 0 and empty.uvs.shape == (0, 2) and empty.face_uvs.shape == (0, 3)
    assert empty.texture.shape == (4, 4, 3) and not empty.texture.any()


def test_gaussians_to_mesh_texels():
    """texels=None is the path without a texture; an int bakes from the pruned Gaussians the density used."""
    seed, N, G = R.E2E["ragged"]
    g = R.random_gaussians(seed, N)
    g[:5, 3] = 0.004  # pruned by min_opacity = 0.005, though above the field's cutoff
    gt = torch.from_numpy(g)
    plain = M.gaussians_to_mesh(gt, G, R.ISO)
    none = M.gaussians_to_mesh(gt, G, R.ISO, texels=None)
    assert plain.texture is None and plain.uvs is None and plain.face_uvs is None and none.texture is None
    assert torch.equal(none.vertices, plain.vertices) and torch.equal(none.faces, plain.faces)
    assert torch.equal(none.colors, plain.colors)
    baked = M.gaussians_to_mesh(gt, G, R.ISO, texels=4)
    assert torch.equal(baked.vertices, plain.vertices) and torch.equal(baked.faces, plain.faces)
    assert torch.equal(baked.colors, plain.colors)
    again = M.bake_texture(plain, gt[5:], 4, resolution=G)
    assert torch.equal(baked.texture, again.texture) and torch.equal(baked.uvs, again.uvs)
    assert lgm_amd.bake_texture is M.bake_texture and lgm_amd.sample_field is M.sample_field


def _parse_obj(path):
    v, vt, f, ft, other = [], [], [], [], []
    for line in open(path):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vt":
            vt.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            f.append([int(x.split("/")[0]) - 1 for x in w[1:]])
            ft.append([int(x.split("/")[1]) - 1 for x in w[1:]])
        else:
            other.append(w)
    return np.array(v), np.array(vt), np.array(f), np.array(ft), other


def test_textured_obj_mtl_png(tmp_path):
    from PIL import Image
    g, G, mesh = cpu_mesh("ragged")
    baked = M.bake_texture(mesh, torch.from_numpy(g), 4, resolution=G)
    path = str(tmp_path / "object.obj")
    baked.save_obj(path)
    v, vt, f, ft, other = _parse_obj(path)
    assert v.shape == (mesh.vertices.shape[0], 3) and (v.astype(np.float32) == mesh.vertices.numpy()).all()
    assert vt.shape == (2 * mesh.faces.shape[0], 2) and (vt.astype(np.float32) == baked.uvs.numpy()).all()
    assert (f == mesh.faces.numpy()).all() and (ft == baked.face_uvs.numpy()).all()
    assert ["mtllib", "object.mtl"] in other and any(w[0] == "usemtl" for w in other)
    mtl = [line.split() for line in open(tmp_path / "object.mtl")]
    assert ["map_Kd", "object.png"] in mtl
    assert [w for w in other if w[0] == "usemtl"][0][1] == [w for w in mtl if w[0] == "newmtl"][0][1]
    png = np.asarray(Image.open(tmp_path / "object.png"))
    H, W = baked.texture.shape[:2]
    want = np.round(np.clip(baked.texture.numpy(), 0.0, 1.0) * 255.0).astype(np.uint8)
    assert png.shape == (H, W, 3) and png.dtype == np.uint8 and (png == want).all()
    # the PLY writer ignores the texture
    baked.save_ply(str(tmp_path / "a.ply"))
    mesh.save_ply(str(tmp_path / "b.ply"))
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["a.ply", "b.ply", "object.mtl", "object.obj", "object.png"]


def test_untextured_obj_is_unchanged(tmp_path):
    """Byte for byte what save_obj wrote before textures existed: `v x y z r g b` with repr floats, `f a b c`."""
    g, G, mesh = cpu_mesh("sphere")
    path = str(tmp_path / "plain.obj")
    mesh.save_obj(path)
    v, f, c = mesh.vertices.numpy(), mesh.faces.numpy(), np.clip(mesh.colors.numpy(), 0.0, 1.0)
    want = f"# {len(v)} vertices, {len(f)} faces\n"
    want += "".join("v " + " ".join(repr(float(x)) for x in list(a) + list(b)) + "\n" for a, b in zip(v, c))
    want += "".join(f"f {a + 1} {b + 1} {c_ + 1}\n" for a, b, c_ in f.tolist())
    assert open(path).read() == want
    M.Mesh(mesh.vertices, mesh.faces).save_obj(path)
    want = f"# {len(v)} vertices, {len(f)} faces\n"
    want += "".join("v " + " ".join(repr(float(x)) for x in a) + "\n" for a in v)
    want += "".join(f"f {a + 1} {b + 1} {c_ + 1}\n" for a, b, c_ in f.tolist())
    assert open(path).read() == want
    assert os.listdir(tmp_path) == ["plain.obj"]


def test_save_mesh_passes_texels(tmp_path):
    from lgm_amd import GaussianRenderer, Options
    seed, N, G = R.E2E["ragged"]
    gt = torch.from_numpy(R.random_gaussians(seed, N))[None]
    r = GaussianRenderer(Options(output_size=64))
    plain = r.save_mesh(gt, str(tmp_path / "plain.obj"), resolution=G)
    baked = r.save_mesh(gt, str(tmp_path / "tex.obj"), resolution=G, texels=2)
    assert plain.texture is None and baked.texture is not None and baked.texture.shape[2] == 3
    assert torch.equal(plain.faces, baked.faces)
    assert sorted(os.listdir(tmp_path)) == ["plain.obj", "tex.mtl", "tex.obj", "tex.png"]
    assert "vt " in open(tmp_path / "tex.obj").read() and "vt " not in open(tmp_path / "plain.obj").read()
