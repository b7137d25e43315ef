"""The mesh kernels (include/lgm_mesh.h, lgm_amd/csrc/mesh.hip) on the GPU against the numpy restatement
tests/mesh_ref.py: the density pass against fp64, the extraction against the restatement on the same fp32 grid, the
whole path against the fp64 mesh, the mesh invariants, a known sphere, and the error paths (nothing launched)."""
import numpy as np
import pytest
import torch

from lgm_amd import _native as nat
from lgm_amd import mesh as M
from tests import mesh_ref as R

pytestmark = pytest.mark.gpu
E2E, ISO, e2e_reference = R.E2E, R.ISO, R.e2e_reference

KERNELS_DENSITY = {"k_mesh_bin_count", "k_mesh_scan_reduce", "k_mesh_scan_top", "k_mesh_scan_add", "k_mesh_bin_fill",
                   "k_mesh_density"}
KERNELS_EXTRACT = {"k_mesh_classify", "k_mesh_scan_reduce", "k_mesh_scan_top", "k_mesh_scan_add", "k_mesh_emit"}
_GRIDS = {}


def gpu_density(name, dev):
    """The GPU's density grid of a case (computed once; the tests leave it unchanged)."""
    if name not in _GRIDS:
        g, G, mod = R.density_cases()[name]
        sigma = torch.full(G, float("nan"), device=dev)
        rgb = torch.full(G + (3,), float("nan"), device=dev)
        M.density_grid(torch.from_numpy(g).to(dev), G, scale_modifier=mod, out=(sigma, rgb))
        _GRIDS[name] = (sigma, rgb)
    return _GRIDS[name]


@pytest.mark.parametrize("name", sorted(R.density_cases()))
def test_density_against_fp64(cuda, name):
    g, G, mod = R.density_cases()[name]
    sigma, rgb = gpu_density(name, cuda)  # (into buffers pre-filled with NaN)
    R.check_density(sigma.cpu().numpy(), rgb.cpu().numpy(), name)
    # two calls are bitwise equal, and sigma does not depend on whether rgb is asked for (rgb = NULL)
    s2, c2 = M.density_grid(torch.from_numpy(g).to(cuda), G, scale_modifier=mod)
    assert torch.equal(s2, sigma) and torch.equal(c2, rgb)
    s3, none = M.density_grid(torch.from_numpy(g).to(cuda), G, scale_modifier=mod, colors=False)
    assert none is None and torch.equal(s3, sigma)


def test_density_skipped_rows_change_nothing(cuda):
    """The rows the kernel must skip (o <= eps, NaN, zero scale, zero quaternion) leave the grid of the others."""
    g, G, mod = R.density_cases()["edge"]
    sigma, rgb = gpu_density("edge", cuda)
    s2, c2 = M.density_grid(torch.from_numpy(g[:16]).to(cuda), G)
    assert torch.equal(s2, sigma) and torch.equal(c2, rgb)


def test_density_short_capacity_poisons(cuda):
    """A list capacity below the counted pairs: nothing out of bounds, every output NaN (include/lgm_mesh.h)."""
    g, G, _ = R.density_cases()["ragged"]
    gt = torch.from_numpy(g).to(cuda)
    L, (_, lo, h) = nat.lib(), M.grid_params(G)
    ws = torch.empty(L.lgm_mesh_density_workspace_size(len(g), *G, 0), dtype=torch.uint8, device=cuda)
    npairs = torch.zeros(1, dtype=torch.int64, device=cuda)
    st = nat.stream_of(cuda)
    assert L.lgm_mesh_density_count(nat.ptr(gt), len(g), 1.0, *G, M._c3(lo), M._c3(h), 1e-4, nat.ptr(ws), ws.numel(),
                                    nat.ptr(npairs), st, None) == 0
    cap = int(npairs.item()) - 1
    assert cap > 0
    ws = torch.empty(L.lgm_mesh_density_workspace_size(len(g), *G, cap), dtype=torch.uint8, device=cuda)
    guard = torch.zeros(64, dtype=torch.uint8, device=cuda)  # (allocated right after: stays zero)
    sigma, rgb = torch.zeros(G, device=cuda), torch.zeros(G + (3,), device=cuda)
    assert L.lgm_mesh_density(nat.ptr(gt), len(g), 1.0, *G, M._c3(lo), M._c3(h), 1e-4, cap, nat.ptr(sigma), nat.ptr(rgb),
                              nat.ptr(ws), ws.numel(), st, None) == 0
    assert torch.isnan(sigma).all() and torch.isnan(rgb).all() and not guard.any()


EXTRACT_ON = ("ragged", "rand32", "chunks", "needle", "edge", "half", "tiny", "empty")


@pytest.mark.parametrize("name", EXTRACT_ON)
def test_extraction_on_density_grids(cuda, name):
    sigma, rgb = gpu_density(name, cuda)
    m = M.extract_surface(sigma, rgb, ISO)
    R.check_extraction(m.vertices.cpu().numpy(), m.colors.cpu().numpy(), m.faces.cpu().numpy(), sigma.cpu().numpy(),
                       rgb.cpu().numpy(), ISO)
    if name in ("ragged", "rand32"):
        assert m.faces.shape[0] > 0
    m2 = M.extract_surface(sigma, rgb, ISO)  # two calls: bitwise equal
    assert torch.equal(m2.vertices, m.vertices) and torch.equal(m2.colors, m.colors) and torch.equal(m2.faces, m.faces)


@pytest.mark.parametrize("name", sorted(R.hand_grids()))
def test_extraction_on_hand_grids(cuda, name):
    sigma, rgb = R.hand_grids()[name]
    m = M.extract_surface(torch.from_numpy(sigma).to(cuda), torch.from_numpy(rgb).to(cuda), ISO)
    R.check_extraction(m.vertices.cpu().numpy(), m.colors.cpu().numpy(), m.faces.cpu().numpy(), sigma, rgb, ISO)
    if name == "single":
        assert m.vertices.shape[0] == 8 and m.faces.shape[0] == 12  # a cube: 6 quads, 12 triangles
    if name == "all_outside":
        assert m.vertices.shape[0] == 0 and m.faces.shape[0] == 0
    if name == "all_inside":  # the boundary shell only: a box two nodes in from every face
        assert m.faces.shape[0] > 0 and R.invariants(m.vertices.cpu().numpy(), m.faces.cpu().numpy())[1]
    m2 = M.extract_surface(torch.from_numpy(sigma).to(cuda), None, ISO)  # rgb = NULL
    assert m2.colors is None and torch.equal(m2.faces, m.faces) and torch.equal(m2.vertices, m.vertices)


def test_extraction_scans_span_tiles(cuda):
    """48^3 = 110,592 nodes: the scans run over 54 tiles of 2048 entries, so the tile offsets matter."""
    rng = np.random.default_rng(5)
    sigma = torch.from_numpy(rng.uniform(0, 1, (48, 48, 48)).astype(np.float32)).to(cuda)
    m = M.extract_surface(sigma, None, ISO)
    cpu = M.extract_surface(sigma.cpu(), None, ISO)  # (the torch path was held to the restatement in the CPU file)
    assert torch.equal(m.faces.cpu(), cpu.faces)
    assert (m.vertices.cpu() - cpu.vertices).abs().max() <= 2e-6
    R.check_invariants(m.vertices.cpu().numpy(), m.faces.cpu().numpy())


def _emit_args(cuda, sigma, rgb, G):
    L, (_, lo, h) = nat.lib(), M.grid_params(G)
    ws = torch.empty(L.lgm_mesh_extract_workspace_size(*G), dtype=torch.uint8, device=cuda)
    counts = torch.zeros(2, dtype=torch.int64, device=cuda)
    assert L.lgm_mesh_count(nat.ptr(sigma), *G, ISO, nat.ptr(ws), ws.numel(), nat.ptr(counts), nat.stream_of(cuda),
                            None) == 0
    nv, nf = counts.tolist()
    return L, lo, h, ws, nv, nf


def test_emit_capacity_one_short(cuda):
    sigma, rgb = gpu_density("ragged", cuda)
    G = tuple(sigma.shape)
    L, lo, h, ws, nv, nf = _emit_args(cuda, sigma, rgb, G)
    assert nv > 0 and nf > 0
    V, C = torch.zeros(nv, 3, device=cuda), torch.zeros(nv, 3, device=cuda)
    F = torch.zeros(nf, 3, dtype=torch.int32, device=cuda)
    prof = nat.KernelProfiler()
    for cap_v, cap_f in ((nv - 1, nf), (nv, nf - 1)):
        with prof:
            rc = L.lgm_mesh_emit(nat.ptr(sigma), nat.ptr(rgb), *G, M._c3(lo), M._c3(h), ISO, nat.ptr(ws), ws.numel(),
                                 nv, nf, nat.ptr(V), nat.ptr(C), nat.ptr(F), cap_v, cap_f, nat.stream_of(cuda),
                                 nat.diag())
        assert rc < 0 and b"capacity" in L.lgm_last_error()
    assert prof.summary() == {}  # nothing launched
    assert not V.any() and not F.any()
    prof.close()


@pytest.mark.parametrize("name", sorted(E2E))
def test_end_to_end_against_fp64(cuda, name):
    """gaussians_to_mesh against the fp64 restatement. Under the precondition (every node's |sigma - iso| > 1e-3 iso in
    fp64) no classification can flip, so the faces are the restatement's exactly; the vertices are held to twice the
    distance of the restatement's own fp32 run from fp64 (or 1e-6 of the box extent)."""
    g, G, margin, v64, c64, f64, d32 = e2e_reference(name)
    assert margin > 1e-3, margin
    m = M.gaussians_to_mesh(torch.from_numpy(g).to(cuda)[None], G, ISO)
    assert (m.faces.cpu().numpy().astype(np.int64) == f64).all()
    dist = float(np.abs(m.vertices.cpu().numpy().astype(np.float64) - v64).max())
    print(name, "fp32 restatement", d32, "gpu", dist, "bar", max(2 * d32, 2e-6))
    R.check_invariants(m.vertices.cpu().numpy(), m.faces.cpu().numpy())
    assert dist <= max(2 * d32, 1e-6 * 2.0)


def test_known_sphere_and_ellipsoid(cuda):
    m = M.gaussians_to_mesh(torch.from_numpy(R.one_gaussian()).to(cuda), 24, iso=0.3)
    R.check_sphere(m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.colors.cpu().numpy())
    # the same Gaussian rotated and scaled to an ellipsoid, against the restatement on the GPU's grid
    g = R.one_gaussian(0.9, (0.3, 0.15, 0.08), (0.7, -0.4, 0.5, 0.3), (0.05, -0.1, 0.02))
    sigma, rgb = M.density_grid(torch.from_numpy(g).to(cuda), 24)
    ref_s, ref_c, border = R.density(g, (24, 24, 24))
    assert (np.abs(sigma.cpu().numpy() - ref_s) <= 1e-5 * ref_s + 1e-6 + R.EPS * border).all()
    m = M.extract_surface(sigma, rgb, 0.3)
    R.check_extraction(m.vertices.cpu().numpy(), m.colors.cpu().numpy(), m.faces.cpu().numpy(), sigma.cpu().numpy(),
                       rgb.cpu().numpy(), 0.3)
    closed, twice, euler, vol, _ = R.invariants(m.vertices.cpu().numpy(), m.faces.cpu().numpy())
    assert closed and twice and euler == 2
    # the enclosed volume: that of the ellipsoid d2 = 2 ln 3, within the grid's resolution
    exact = 4.0 / 3.0 * np.pi * 0.3 * 0.15 * 0.08 * (2 * np.log(3.0)) ** 1.5
    assert abs(vol - exact) <= 0.25 * exact


def test_kernel_names(cuda):
    g, G, _ = R.density_cases()["ragged"]
    prof = nat.KernelProfiler()
    with prof:
        sigma, rgb = M.density_grid(torch.from_numpy(g).to(cuda), G)
    names = prof.summary()
    assert set(names) == KERNELS_DENSITY
    assert names["k_mesh_density"][0] == 1 and names["k_mesh_bin_count"][0] == 2  # (the count call, then the pass)
    prof.reset()
    with prof:
        M.extract_surface(sigma, rgb, ISO)
    names = prof.summary()
    assert set(names) == KERNELS_EXTRACT and names["k_mesh_scan_top"][0] == 2 and names["k_mesh_emit"][0] == 1
    prof.close()


def test_error_paths_launch_nothing(cuda):
    L = nat.lib()
    G = (8, 9, 10)
    _, lo, h = M.grid_params(G)
    lo_c, h_c, st = M._c3(lo), M._c3(h), nat.stream_of(cuda)
    g = torch.from_numpy(R.random_gaussians(0, 4)).to(cuda)
    ws = torch.empty(L.lgm_mesh_density_workspace_size(4, *G, 4096) + L.lgm_mesh_extract_workspace_size(*G),
                     dtype=torch.uint8, device=cuda)
    npairs = torch.zeros(2, dtype=torch.int64, device=cuda)
    sigma, rgb = torch.zeros(G, device=cuda), torch.zeros(G + (3,), device=cuda)
    V, F = torch.zeros(16, 3, device=cuda), torch.zeros(16, 3, dtype=torch.int32, device=cuda)
    nan, inf = float("nan"), float("inf")
    bad_h, neg_h, bad_lo = M._c3(np.array([h[0], nan, h[2]])), M._c3(np.array([h[0], h[1], -h[2]])), M._c3([0, inf, 0])
    P = nat.ptr

    def count(g_=P(g), N=4, mod=1.0, G_=G, lo_=lo_c, h_=h_c, cut=1e-4, ws_=P(ws), wsb=ws.numel(), np_=P(npairs)):
        return L.lgm_mesh_density_count(g_, N, mod, *G_, lo_, h_, cut, ws_, wsb, np_, st, nat.diag())

    def dens(g_=P(g), N=4, mod=1.0, G_=G, lo_=lo_c, h_=h_c, cut=1e-4, cap=4096, s_=P(sigma), c_=P(rgb), ws_=P(ws),
             wsb=ws.numel()):
        return L.lgm_mesh_density(g_, N, mod, *G_, lo_, h_, cut, cap, s_, c_, ws_, wsb, st, nat.diag())

    def cnt(s_=P(sigma), G_=G, iso=0.5, ws_=P(ws), wsb=ws.numel(), c_=P(npairs)):
        return L.lgm_mesh_count(s_, *G_, iso, ws_, wsb, c_, st, nat.diag())

    def emit(s_=P(sigma), c_=P(rgb), G_=G, lo_=lo_c, h_=h_c, iso=0.5, ws_=P(ws), wsb=ws.numel(), nv=4, nf=4, v_=P(V),
             col_=P(V), f_=P(F), cv=16, cf=16):
        return L.lgm_mesh_emit(s_, c_, *G_, lo_, h_, iso, ws_, wsb, nv, nf, v_, col_, f_, cv, cf, st, nat.diag())

    bad = [lambda: count(g_=None), lambda: count(G_=(2, 9, 10)), lambda: count(G_=(2048, 2048, 512)),
           lambda: count(h_=bad_h), lambda: count(h_=neg_h), lambda: count(lo_=bad_lo), lambda: count(h_=None),
           lambda: count(cut=0.0), lambda: count(cut=nan), lambda: count(mod=inf), lambda: count(ws_=None),
           lambda: count(wsb=64), lambda: count(np_=None), lambda: count(N=-1), lambda: count(N=2 ** 31),
           lambda: dens(g_=None), lambda: dens(G_=(8, 9, 2)), lambda: dens(s_=None), lambda: dens(cap=-1),
           lambda: dens(cap=2 ** 31), lambda: dens(cut=-1.0), lambda: dens(h_=bad_h),
           lambda: dens(wsb=L.lgm_mesh_density_workspace_size(4, *G, 4096) - 1), lambda: dens(ws_=None),
           lambda: cnt(s_=None), lambda: cnt(G_=(8, 2, 10)), lambda: cnt(iso=0.0), lambda: cnt(iso=nan),
           lambda: cnt(iso=-0.5), lambda: cnt(ws_=None), lambda: cnt(wsb=L.lgm_mesh_extract_workspace_size(*G) - 1),
           lambda: cnt(c_=None),
           lambda: emit(s_=None), lambda: emit(G_=(1, 9, 10)), lambda: emit(lo_=None), lambda: emit(h_=neg_h),
           lambda: emit(iso=inf), lambda: emit(ws_=None), lambda: emit(wsb=16), lambda: emit(nv=-1), lambda: emit(nf=-1),
           lambda: emit(v_=None), lambda: emit(col_=None), lambda: emit(f_=None), lambda: emit(cv=3), lambda: emit(cf=3),
           lambda: emit(nv=2 ** 30, cv=2 ** 30), lambda: emit(nf=2 ** 30, cf=2 ** 30)]
    prof = nat.KernelProfiler()
    with prof:
        for i, call in enumerate(bad):
            assert call() < 0 and L.lgm_last_error(), i
    assert prof.summary() == {}
    assert not sigma.any() and not V.any() and not F.any()
    assert L.lgm_mesh_density_workspace_size(4, 2, 9, 10, 0) == 0 and L.lgm_mesh_extract_workspace_size(8, 9, 2) == 0
    # the same calls with nothing wrong go through (N = 0 with a null g included)
    with prof:
        assert count() == 0 and dens() == 0 and cnt() == 0 and dens(g_=None, N=0) == 0
        assert emit(nv=0, nf=0, v_=None, col_=None, f_=None, cv=0, cf=0) == 0
    assert "k_mesh_density" in prof.summary() and "k_mesh_emit" not in prof.summary()
    prof.close()
    with pytest.raises(nat.NativeError):
        nat.check(count(cut=0.0), "lgm_mesh_density_count")
