"""lgm_amd.mesh on CPU tensors (the torch forms of include/lgm_mesh.h) against the numpy restatement tests/mesh_ref.py
with the bars of the GPU file, the OBJ and PLY writers, and GaussianRenderer.save_mesh. No GPU here."""
import numpy as np
import pytest
import torch

from lgm_amd import mesh as M
from lgm_amd.ply import read_mesh_ply
from tests import mesh_ref as R

E2E, ISO, e2e_reference = R.E2E, R.ISO, R.e2e_reference


@pytest.mark.parametrize("name", sorted(R.density_cases()))
def test_density_torch_against_fp64(name):
    g, G, mod = R.density_cases()[name]
    sigma, rgb = M.density_grid(torch.from_numpy(g), G, scale_modifier=mod)
    assert sigma.shape == G and rgb.shape == G + (3,) and sigma.dtype == torch.float32
    R.check_density(sigma.numpy(), rgb.numpy(), name)
    s2, none = M.density_grid(torch.from_numpy(g), G, scale_modifier=mod, colors=False)
    assert none is None and torch.equal(s2, sigma)


@pytest.mark.parametrize("name", sorted(R.hand_grids()))
def test_extraction_torch_on_hand_grids(name):
    sigma, rgb = R.hand_grids()[name]
    m = M.extract_surface(torch.from_numpy(sigma), torch.from_numpy(rgb), ISO)
    R.check_extraction(m.vertices.numpy(), m.colors.numpy(), m.faces.numpy(), sigma, rgb, ISO)
    if name == "single":
        assert m.vertices.shape[0] == 8 and m.faces.shape[0] == 12  # a cube: 6 quads, 12 triangles
    if name == "all_outside":
        assert m.vertices.shape[0] == 0 and m.faces.shape[0] == 0
    if name == "checkerboard":  # every cell with an inside corner off the forced layer is active: all but 4 corner cells
        assert m.vertices.shape[0] == 6 * 5 * 4 - 4
    m2 = M.extract_surface(torch.from_numpy(sigma), None, ISO)
    assert m2.colors is None and torch.equal(m2.faces, m.faces) and torch.equal(m2.vertices, m.vertices)


@pytest.mark.parametrize("name", sorted(E2E))
def test_end_to_end_torch(name):
    g, G, margin, v64, c64, f64, d32 = e2e_reference(name)
    assert margin > 1e-3, margin  # the precondition: no classification can flip
    m = M.gaussians_to_mesh(torch.from_numpy(g)[None], G, ISO)
    assert (m.faces.numpy().astype(np.int64) == f64).all()
    dist = float(np.abs(m.vertices.numpy().astype(np.float64) - v64).max())
    print(name, "fp32 restatement", d32, "torch path", dist)
    assert dist <= max(2 * d32, 1e-6 * 2.0)
    assert np.abs(m.colors.numpy() - c64).max() <= 1e-5
    R.check_invariants(m.vertices.numpy(), m.faces.numpy())


def test_known_sphere_torch():
    m = M.gaussians_to_mesh(torch.from_numpy(R.one_gaussian()), 24, iso=0.3)
    R.check_sphere(m.vertices.numpy(), m.faces.numpy(), m.colors.numpy())


def test_obj_and_ply_round_trip(tmp_path):
    sigma, rgb = R.hand_grids()["block_at_boundary"]
    m = M.extract_surface(torch.from_numpy(sigma), torch.from_numpy(rgb), ISO)
    obj, ply = str(tmp_path / "m.obj"), str(tmp_path / "m.ply")
    m.save_obj(obj)
    m.save_ply(ply)
    vs, fs = [], []
    for line in open(obj):
        tok = line.split()
        if tok and tok[0] == "v":
            assert len(tok) == 7
            vs.append([float(t) for t in tok[1:]])
        elif tok and tok[0] == "f":
            fs.append([int(t) - 1 for t in tok[1:]])
    vs = np.array(vs)
    assert np.array_equal(vs[:, :3].astype(np.float32), m.vertices.numpy())  # repr() round-trips a float
    assert np.array_equal(vs[:, 3:].astype(np.float32), m.colors.numpy().clip(0, 1))
    assert np.array_equal(np.array(fs), m.faces.numpy())
    v, f, c = read_mesh_ply(ply)
    assert np.array_equal(v, m.vertices.numpy()) and np.array_equal(f, m.faces.numpy())
    assert np.array_equal(c, np.rint(m.colors.numpy().astype(np.float64) * 255).astype(np.uint8))
    M.Mesh(m.vertices, m.faces, None).save_ply(ply)
    v, f, c = read_mesh_ply(ply)
    assert c is None and np.array_equal(f, m.faces.numpy())


def test_save_mesh(tmp_path):
    from lgm_amd import GaussianRenderer, preset
    gs = GaussianRenderer(preset("small"))
    g = torch.from_numpy(R.random_gaussians(0))[None]
    mesh = gs.save_mesh(g, str(tmp_path / "object.obj"), resolution=(20, 12, 9))
    ref = M.gaussians_to_mesh(g, (20, 12, 9))
    assert torch.equal(mesh.faces, ref.faces) and torch.equal(mesh.vertices, ref.vertices)
    assert sum(line.startswith("f ") for line in open(tmp_path / "object.obj")) == mesh.faces.shape[0] > 0
    gs.save_mesh(g, str(tmp_path / "object.ply"), resolution=(20, 12, 9))
    assert np.array_equal(read_mesh_ply(str(tmp_path / "object.ply"))[1], mesh.faces.numpy())
    with pytest.raises(AssertionError):
        gs.save_mesh(torch.cat([g, g]), str(tmp_path / "two.obj"))
    # min_opacity prunes as save_ply does: dropping everything leaves an empty mesh
    assert M.gaussians_to_mesh(g, (20, 12, 9), min_opacity=2.0).faces.shape[0] == 0


def test_argument_checks():
    g = torch.from_numpy(R.random_gaussians(0))
    with pytest.raises(ValueError):
        M.density_grid(g, (2, 8, 8))
    with pytest.raises(ValueError):
        M.density_grid(g[:, :13], 8)
    with pytest.raises(ValueError):
        M.density_grid(g, 8, cutoff=0.0)
    with pytest.raises(ValueError):
        M.extract_surface(torch.zeros(4, 4, 4), iso=0.0)
    with pytest.raises(ValueError):
        M.extract_surface(torch.zeros(4, 4, 4), torch.zeros(4, 4, 4, 2))
