"""The sampling and atlas kernels (include/lgm_mesh.h, lgm_amd/csrc/mesh.hip) and bake_texture on the GPU against the
numpy restatement tests/mesh_texture_ref.py: the field at points against fp64 with the density pass's bars, the atlas
bitwise against its fp32 restatement, the baked texture against the fp64 field at the GPU's own atlas points, and the
error paths (nothing launched)."""
import numpy as np
import pytest
import torch

from lgm_amd import _native as nat
from lgm_amd import mesh as M
from tests import mesh_ref as R
from tests import mesh_texture_ref as TR

pytestmark = pytest.mark.gpu

KERNELS_SAMPLE = {"k_mesh_sample_bin_count", "k_mesh_scan_reduce", "k_mesh_scan_top", "k_mesh_scan_add",
                  "k_mesh_bin_fill", "k_mesh_point_count", "k_mesh_point_fill", "k_mesh_sample"}
TEXELS = (2, 4, 5)
_SAMPLES, _MESHES = {}, {}


def gpu_sample(name, dev):
    """The GPU's samples of a case (computed once; the tests leave them unchanged)."""
    if name not in _SAMPLES:
        g, G, mod, pts = TR.sample_cases()[name]
        _SAMPLES[name] = M.sample_field(torch.from_numpy(g).to(dev), torch.from_numpy(pts).to(dev), G, scale_modifier=mod)
    return _SAMPLES[name]


def gpu_mesh(name, dev):
    """The GPU's own mesh of an atlas case (computed once; the tests leave it unchanged)."""
    if name not in _MESHES:
        if name == "sphere":
            g, G, iso = R.one_gaussian(), (24, 24, 24), 0.3
        else:
            seed, N, G = R.E2E[name]
            g, iso = R.random_gaussians(seed, N), R.ISO
        _MESHES[name] = (g, G, M.gaussians_to_mesh(torch.from_numpy(g).to(dev), G, iso))
    return _MESHES[name]


@pytest.mark.parametrize("name", sorted(TR.sample_cases()))
def test_sample_against_fp64(cuda, name):
    """Every density case at 6,000 uniform points (`over_cap`, the walk-all path, at 1,500; `chunks` with 1,000 more in
    its first brick: several point batches on one workgroup against a five-chunk list)."""
    g, G, mod, pts = TR.sample_cases()[name]
    sigma, rgb = gpu_sample(name, cuda)
    assert sigma.shape == (len(pts),) and rgb.shape == (len(pts), 3)
    TR.check_sample(sigma.cpu().numpy(), rgb.cpu().numpy(), TR.sample_reference(name), name)
    # two calls are bitwise equal, and sigma does not depend on whether rgb is asked for (rgb = NULL)
    gt, pt = torch.from_numpy(g).to(cuda), torch.from_numpy(pts).to(cuda)
    s2, c2 = M.sample_field(gt, pt, G, scale_modifier=mod)
    assert torch.equal(s2, sigma) and torch.equal(c2, rgb)
    s3, none = M.sample_field(gt, pt, G, scale_modifier=mod, colors=False)
    assert none is None and torch.equal(s3, sigma)


def test_sample_independent_of_the_acceleration_grid(cuda):
    """`ragged` (20, 12, 9) and `rand32` (32, 32, 32) are the same Gaussians and the same points: both meet the bars
    (checked above), so they differ by at most twice the bars (brick origins differ: not bitwise)."""
    (sa, ca), (sb, cb) = gpu_sample("ragged", cuda), gpu_sample("rand32", cuda)
    ref_s, _, border, _ = TR.sample_reference("ragged")
    assert (TR.sample_reference("rand32")[0] == ref_s).all()
    bar = 2 * (1e-5 * ref_s + 1e-6 + R.EPS * np.maximum(border, TR.sample_reference("rand32")[2]))
    assert (np.abs(sa.cpu().numpy().astype(np.float64) - sb.cpu().numpy()) <= bar).all()
    assert np.abs(ca.cpu().numpy() - cb.cpu().numpy())[ref_s > 1e-3].max() <= 2e-5


def test_sample_gap_between_bricks(cuda):
    """A cut that ends between node 7 (x = -0.3913) and node 8 (-0.3043) of a 24^3 grid: in the density pass's lists
    the Gaussian is in brick 1 only, and a sampler reading them returns 0 at (-0.34, 0, 0), which lies in brick 0."""
    g, G, pts = TR.GAP
    sigma, rgb = M.sample_field(torch.from_numpy(g).to(cuda), torch.from_numpy(pts).to(cuda), G)
    ref = TR.sample(g, pts, G)
    assert abs(ref[0][0] - 5.63e-4) < 1e-5 and ref[0][1] == 0
    TR.check_sample(sigma.cpu().numpy(), rgb.cpu().numpy(), ref, "gap")
    assert sigma[1] == 0 and sigma[0] > 5e-4


def test_sample_special_points(cuda):
    """Points on nodes, on brick faces and one ulp either side, on the box faces lo - h / 2 and lo + (G - 1/2) h and one
    ulp either side, and NaN / inf points: the ones that are not sampled give exactly 0, and the others are what they
    are without them."""
    g, G, mod = R.density_cases()["ragged"]
    sp = TR.special_points(G)
    pts = np.concatenate(list(sp.values()))
    ref = TR.sample(g, pts, G)
    inside = dict(zip(sp, np.split(ref[3], np.cumsum([len(v) for v in sp.values()])[:-1])))
    assert inside["nodes"].all() and inside["inward"].all() and not inside["outward"].any() and not inside["bad"].any()
    gt = torch.from_numpy(g).to(cuda)
    sigma, rgb = M.sample_field(gt, torch.from_numpy(pts).to(cuda), G)
    TR.check_sample(sigma.cpu().numpy(), rgb.cpu().numpy(), ref, "special")
    assert (sigma.cpu().numpy()[~ref[3]] == 0).all() and (rgb.cpu().numpy()[~ref[3]] == 0).all()
    keep = torch.from_numpy(ref[3]).to(cuda)
    s2, c2 = M.sample_field(gt, torch.from_numpy(pts).to(cuda)[keep], G)
    assert torch.equal(s2, sigma[keep]) and torch.equal(c2, rgb[keep])
    # leading shapes are kept
    s4, c4 = M.sample_field(gt, torch.from_numpy(pts[:24].reshape(2, 3, 4, 3)).to(cuda), G)
    assert s4.shape == (2, 3, 4) and c4.shape == (2, 3, 4, 3) and torch.equal(s4.reshape(-1), sigma[:24])


def _sample_args(cuda, name="ragged", M_=64):
    g, G, _ = R.density_cases()[name]
    gt = torch.from_numpy(g).to(cuda)
    pts = torch.from_numpy(TR.uniform_points(M_)).to(cuda)
    L, (_, lo, h) = nat.lib(), M.grid_params(G)
    ws = torch.empty(L.lgm_mesh_sample_workspace_size(len(g), 0, *G, 0), dtype=torch.uint8, device=cuda)
    npairs = torch.zeros(1, dtype=torch.int64, device=cuda)
    assert L.lgm_mesh_sample_count(nat.ptr(gt), len(g), 1.0, *G, M._c3(lo), M._c3(h), 1e-4, nat.ptr(ws), ws.numel(),
                                   nat.ptr(npairs), nat.stream_of(cuda), None) == 0
    return L, gt, pts, G, lo, h, int(npairs.item())


def test_sample_short_capacity_poisons(cuda):
    """A list capacity below the counted pairs: nothing out of bounds, every output NaN (include/lgm_mesh.h), the points
    that are not sampled too."""
    L, gt, pts, G, lo, h, total = _sample_args(cuda)
    pts[3, 0] = 7.0  # (outside the box)
    cap = total - 1
    assert cap > 0
    ws = torch.empty(L.lgm_mesh_sample_workspace_size(len(gt), len(pts), *G, cap), dtype=torch.uint8, device=cuda)
    guard = torch.zeros(64, dtype=torch.uint8, device=cuda)  # (allocated right after: stays zero)
    sigma, rgb = torch.zeros(len(pts), device=cuda), torch.zeros(len(pts), 3, device=cuda)
    st = nat.stream_of(cuda)

    def run(capacity):
        return L.lgm_mesh_sample(nat.ptr(gt), len(gt), 1.0, *G, M._c3(lo), M._c3(h), 1e-4, capacity, nat.ptr(pts),
                                 len(pts), nat.ptr(sigma), nat.ptr(rgb), nat.ptr(ws), ws.numel(), st, None)

    assert run(cap) == 0
    assert torch.isnan(sigma).all() and torch.isnan(rgb).all() and not guard.any()
    # the count is more than the density pass's: the boxes cover the gaps between the bricks' nodes
    npairs = torch.zeros(1, dtype=torch.int64, device=cuda)
    ws0 = torch.empty(L.lgm_mesh_density_workspace_size(len(gt), *G, 0), dtype=torch.uint8, device=cuda)
    assert L.lgm_mesh_density_count(nat.ptr(gt), len(gt), 1.0, *G, M._c3(lo), M._c3(h), 1e-4, nat.ptr(ws0), ws0.numel(),
                                    nat.ptr(npairs), st, None) == 0
    assert total >= int(npairs.item())


def test_sample_kernel_names(cuda):
    g, G, mod, pts = TR.sample_cases()["ragged"]
    gt, pt = torch.from_numpy(g).to(cuda), torch.from_numpy(pts).to(cuda)
    prof = nat.KernelProfiler()
    with prof:
        M.sample_field(gt, pt, G)
    names = prof.summary()
    assert set(names) == KERNELS_SAMPLE
    assert names["k_mesh_sample"][0] == 1 and names["k_mesh_sample_bin_count"][0] == 2  # (the count call, then the pass)
    assert names["k_mesh_scan_top"][0] == 3 and names["k_mesh_point_count"][0] == 1
    prof.reset()
    _, _, mesh = gpu_mesh("ragged", cuda)
    with prof:
        M.mesh_atlas(mesh, 4)
    assert set(prof.summary()) == {"k_mesh_atlas"}
    prof.close()


def test_error_paths_launch_nothing(cuda):
    L, gt, pts, G, lo, h, total = _sample_args(cuda)
    N, Mp = len(gt), len(pts)
    lo_c, h_c, st = M._c3(lo), M._c3(h), nat.stream_of(cuda)
    need = L.lgm_mesh_sample_workspace_size(N, Mp, *G, total)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    npairs = torch.zeros(1, dtype=torch.int64, device=cuda)
    sigma, rgb = torch.zeros(Mp, device=cuda), torch.zeros(Mp, 3, device=cuda)
    nan, inf = float("nan"), float("inf")
    bad_h, bad_lo = M._c3(np.array([h[0], nan, h[2]])), M._c3([0, inf, 0])
    P = nat.ptr

    def count(g_=P(gt), N_=N, mod=1.0, G_=G, lo_=lo_c, h_=h_c, cut=1e-4, ws_=P(ws), wsb=ws.numel(), np_=P(npairs)):
        return L.lgm_mesh_sample_count(g_, N_, mod, *G_, lo_, h_, cut, ws_, wsb, np_, st, nat.diag())

    def samp(g_=P(gt), N_=N, mod=1.0, G_=G, lo_=lo_c, h_=h_c, cut=1e-4, cap=total, p_=P(pts), M_=Mp, s_=P(sigma),
             c_=P(rgb), ws_=P(ws), wsb=ws.numel()):
        return L.lgm_mesh_sample(g_, N_, mod, *G_, lo_, h_, cut, cap, p_, M_, s_, c_, ws_, wsb, st, nat.diag())

    V = torch.zeros(8, 3, device=cuda)
    F = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=cuda)
    pt_out, uv_out = torch.zeros(1, 4, 4, 3, device=cuda), torch.zeros(1, 4, 2, device=cuda)
    fu_out = torch.zeros(2, 3, dtype=torch.int32, device=cuda)

    def atlas(v_=P(V), nv=8, f_=P(F), nf=2, T=4, cols=1, rows=1, p_=P(pt_out), u_=P(uv_out), fu_=P(fu_out)):
        return L.lgm_mesh_atlas(v_, nv, f_, nf, T, cols, rows, p_, u_, fu_, st, nat.diag())

    bad = [lambda: count(g_=None), lambda: count(G_=(2, 12, 9)), lambda: count(h_=bad_h), lambda: count(lo_=bad_lo),
           lambda: count(cut=0.0), lambda: count(mod=inf), lambda: count(ws_=None), lambda: count(wsb=64),
           lambda: count(np_=None), lambda: count(N_=-1), lambda: count(N_=2 ** 31),
           lambda: samp(g_=None), lambda: samp(G_=(20, 12, 2)), lambda: samp(cap=-1), lambda: samp(cap=2 ** 31),
           lambda: samp(cut=nan), lambda: samp(h_=None), lambda: samp(wsb=need - 1), lambda: samp(ws_=None),
           lambda: samp(M_=-1), lambda: samp(M_=(2 ** 31 + 2) // 3), lambda: samp(p_=None), lambda: samp(s_=None),
           lambda: atlas(nv=-1), lambda: atlas(nf=-2), lambda: atlas(nf=1), lambda: atlas(T=1), lambda: atlas(cols=0),
           lambda: atlas(rows=0), lambda: atlas(nf=4), lambda: atlas(T=4, cols=4097), lambda: atlas(T=4, rows=4097),
           lambda: atlas(v_=None), lambda: atlas(f_=None), lambda: atlas(p_=None), lambda: atlas(u_=None),
           lambda: atlas(fu_=None), lambda: atlas(nv=2 ** 30)]
    prof = nat.KernelProfiler()
    with prof:
        for i, call in enumerate(bad):
            assert call() < 0 and L.lgm_last_error(), i
    assert prof.summary() == {}
    assert not sigma.any() and not rgb.any() and not pt_out.any() and not fu_out.any()
    assert L.lgm_mesh_sample_workspace_size(N, -1, *G, 0) == 0 and L.lgm_mesh_sample_workspace_size(N, 4, 2, 9, 9, 0) == 0
    assert L.lgm_mesh_sample_workspace_size(N, (2 ** 31 + 2) // 3, *G, 0) == 0
    # the same calls with nothing wrong go through (N = 0 and M = 0 with null pointers included)
    with prof:
        assert count() == 0 and samp() == 0 and samp(c_=None) == 0 and samp(g_=None, N_=0) == 0
        assert samp(p_=None, M_=0, s_=None, c_=None) == 0
        assert atlas() == 0 and atlas(v_=None, nv=0, f_=None, nf=0, p_=None, u_=None, fu_=None) == 0
    assert prof.summary()["k_mesh_sample"][0] == 3 and prof.summary()["k_mesh_atlas"][0] == 1
    prof.close()
    assert not sigma.any()  # (N = 0 came last: a zero field)
    with pytest.raises(nat.NativeError):
        nat.check(samp(M_=-1), "lgm_mesh_sample")


@pytest.mark.parametrize("name", ("ragged", "cube32", "sphere"))
def test_atlas_and_bake(cuda, name):
    """The atlas of the GPU's own mesh, bitwise against the fp32 restatement, and the baked texture against the fp64
    field at the GPU's own atlas points (every texel: sigma >= 0.05 there, so the rgb bar applies to all)."""
    g, G, mesh = gpu_mesh(name, cuda)
    gt = torch.from_numpy(g).to(cuda)
    V, F = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    assert len(F) // 2 == {"ragged": 448, "cube32": 946, "sphere": 192}[name]
    for T in TEXELS:
        points, uvs, face_uvs, shape = M.mesh_atlas(mesh, T)
        assert TR.check_atlas(points.cpu().numpy(), uvs.cpu().numpy(), face_uvs.cpu().numpy(), V, F, T) == shape
        baked = M.bake_texture(mesh, gt, T, resolution=G)
        assert baked.vertices is mesh.vertices and baked.faces is mesh.faces and baked.colors is mesh.colors
        assert torch.equal(baked.uvs, uvs.reshape(-1, 2)) and torch.equal(baked.face_uvs, face_uvs)
        ref = TR.sample(g, points.cpu().numpy(), G)
        TR.check_texture(baked.texture.cpu().numpy(), points.cpu().numpy(), ref, T, shape[0], shape[1])
        again = M.bake_texture(mesh, gt, T, resolution=G)  # two bakes: bitwise equal
        assert torch.equal(again.texture, baked.texture) and torch.equal(again.uvs, baked.uvs)
        if name == "sphere":
            blocks = baked.texture.reshape(shape[1], T, shape[0], T, 3).permute(0, 2, 1, 3, 4).reshape(-1, T, T, 3)
            assert (blocks[:len(F) // 2].cpu() - torch.tensor([0.8, 0.4, 0.1])).abs().max() <= 1e-6


def test_bake_rejects_other_meshes_and_bakes_an_empty_one(cuda):
    g, G, mesh = gpu_mesh("sphere", cuda)
    gt = torch.from_numpy(g).to(cuda)
    F = mesh.faces
    broken = F.clone()
    broken[5, 0] = (broken[5, 0] + 1) % mesh.vertices.shape[0]  # faces 4 and 5 no longer start at the same q0
    diagonal = F.clone()
    diagonal[5, 1] = diagonal[5, 2] = diagonal[5, 0]  # ... no longer share the q0-q2 diagonal
    out_of_range = F.clone()
    out_of_range[7, 2] = mesh.vertices.shape[0]
    for faces in (F[:-1], broken, diagonal, out_of_range):
        with pytest.raises(ValueError):
            M.bake_texture(M.Mesh(mesh.vertices, faces, mesh.colors), gt, 4, resolution=G)
    empty = M.gaussians_to_mesh(torch.zeros(0, 14, device=cuda), G, texels=4)
    assert empty.faces.shape[0] == 0 and empty.uvs.shape == (0, 2) and empty.face_uvs.shape == (0, 3)
    assert empty.texture.shape == (4, 4, 3) and not empty.texture.any()


def test_gaussians_to_mesh_texels(cuda):
    """texels=None is the path without a texture; an int bakes from the pruned Gaussians the density used."""
    seed, N, G = R.E2E["ragged"]
    g = R.random_gaussians(seed, N)
    g[:5, 3] = 0.004  # pruned by min_opacity = 0.005, though above the field's cutoff
    gt = torch.from_numpy(g).to(cuda)
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
