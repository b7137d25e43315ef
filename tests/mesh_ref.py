"""An independent numpy restatement of include/lgm_mesh.h for the mesh tests: the density pass in fp64 (with the
per-node count of borderline terms), the extraction pass with plain loops in fp32 or fp64, the mesh invariants, and
the seeded inputs the CPU and GPU test files share. Nothing here imports lgm_amd."""
import collections
import functools

import numpy as np

EPS = 1e-4


def grid(G, bound=1.0):
    """lo, h as the fp32 numbers the kernels are given: node (i, j, k) = lo + (i, j, k) h."""
    lo = np.full(3, -bound, np.float32)
    h = np.array([np.float32(2.0 * bound / (n - 1)) for n in G], np.float32)
    return lo, h


def rotation(q):
    r, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def density(g, G, bound=1.0, mod=1.0, eps=EPS):
    """fp64: sigma [G], rgb [G, 3], border [G] = the number of terms with |d2 - rho2| < 1e-4 rho2 at the node."""
    lo, h = grid(G, bound)
    eps = float(np.float32(eps))
    ax = [lo[a].astype(np.float64) + np.arange(G[a], dtype=np.float64) * np.float64(h[a]) for a in range(3)]
    X = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    sw, swc, border = np.zeros(len(X)), np.zeros((len(X), 3)), np.zeros(len(X), np.int64)
    for row in np.asarray(g, np.float32).astype(np.float64):
        mu, o, s, q, c = row[:3], row[3], row[4:7] * float(mod), row[7:11], row[11:14]
        if not np.isfinite(row).all() or not o > eps or not (s > 0).all() or not (q * q).sum() > 0:
            continue
        R = rotation(q)
        y = ((X - mu) @ R) / s  # diag(s)^-1 R^T (x - mu), row-wise
        d2 = (y * y).sum(1)
        rho2 = 2.0 * np.log(o / eps)
        m = d2 <= rho2
        w = o * np.exp(-0.5 * d2[m])
        sw[m] += w
        swc[m] += w[:, None] * c
        border += np.abs(d2 - rho2) < 1e-4 * rho2
    rgb = np.where(sw[:, None] > 0, swc / np.where(sw > 0, sw, 1.0)[:, None], 0.0)
    return sw.reshape(G), rgb.reshape(tuple(G) + (3,)), border.reshape(G)


EDGES = ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))


def extract(sigma, rgb, iso, bound=1.0, dtype=np.float32):
    """Surface nets with plain loops, every operation in `dtype`: vertices [Nv, 3], colors [Nv, 3] (None without
    rgb), faces [Nf, 3] int."""
    dt = dtype
    G = sigma.shape
    lo, h = grid(G, bound)
    lo, h = lo.astype(dt), h.astype(dt)
    iso = dt(np.float32(iso))
    s = np.array(sigma, dtype=dt)
    s[~np.isfinite(s)] = 0
    s[0] = s[-1] = 0
    s[:, 0] = s[:, -1] = 0
    s[:, :, 0] = s[:, :, -1] = 0
    ins = (s >= iso).tolist()
    col = None if rgb is None else np.asarray(rgb, dtype=dt)
    vid, V, C = {}, [], []
    for i in range(G[0] - 1):
        for j in range(G[1] - 1):
            for k in range(G[2] - 1):
                corner = [(i + (c >> 2), j + ((c >> 1) & 1), k + (c & 1)) for c in range(8)]
                flags = [ins[a][b][c] for a, b, c in corner]
                if all(flags) or not any(flags):
                    continue
                p = [dt(0), dt(0), dt(0)]
                cc = [dt(0), dt(0), dt(0)]
                m = 0
                for a, b in EDGES:
                    if flags[a] == flags[b]:
                        continue
                    sa, sb = s[corner[a]], s[corner[b]]
                    t = (iso - sa) / (sb - sa)
                    for d in range(3):
                        off = dt(corner[a][d] - corner[0][d])
                        if corner[b][d] != corner[a][d]:
                            off = t
                        p[d] = p[d] + off
                    if col is not None:
                        rgb_in = col[corner[a] if flags[a] else corner[b]]
                        cc = [cc[d] + rgb_in[d] for d in range(3)]
                    m += 1
                vid[(i, j, k)] = len(V)
                cell = (i, j, k)
                V.append([lo[d] + (dt(cell[d]) + p[d] / dt(m)) * h[d] for d in range(3)])
                C.append([cc[d] / dt(m) for d in range(3)])
    F = []
    for i in range(G[0]):
        for j in range(G[1]):
            for k in range(G[2]):
                n = (i, j, k)
                for a in range(3):
                    if n[a] + 1 >= G[a]:
                        continue
                    up = tuple(n[d] + (d == a) for d in range(3))
                    i0, i1 = ins[i][j][k], ins[up[0]][up[1]][up[2]]
                    if i0 == i1:
                        continue
                    b, c = (a + 1) % 3, (a + 2) % 3
                    q = [vid[tuple(n[d] - (d == b) - (d == c) for d in range(3))],
                         vid[tuple(n[d] - (d == c) for d in range(3))], vid[n],
                         vid[tuple(n[d] - (d == b) for d in range(3))]]
                    F += [(q[0], q[1], q[2]), (q[0], q[2], q[3])] if i0 else [(q[0], q[2], q[1]), (q[0], q[3], q[2])]
    V = np.array(V, dtype=dt).reshape(-1, 3)
    C = None if col is None else np.array(C, dtype=dt).reshape(-1, 3)
    return V, C, np.array(F, dtype=np.int64).reshape(-1, 3)


def invariants(V, F):
    """(closed and consistently oriented: every directed edge as often as its reverse; every undirected edge used
    exactly twice; Euler characteristic V - E + F; signed volume; all indices < Nv)."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    d = collections.Counter()
    for f in F.tolist():
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            d[(a, b)] += 1
    closed = all(d[(b, a)] == c for (a, b), c in d.items())
    und = collections.Counter()
    for (a, b), c in d.items():
        und[(min(a, b), max(a, b))] += c
    twice = all(c == 2 for c in und.values())
    vol = float(np.einsum("ij,ij->i", V[F[:, 0]], np.cross(V[F[:, 1]], V[F[:, 2]])).sum() / 6) if len(F) else 0.0
    in_range = bool(len(F) == 0 or (F.min() >= 0 and F.max() < len(V)))
    return closed, twice, len(V) - len(und) + len(F), vol, in_range


# ------------------------------------------------------------------------------------------------- shared inputs
def random_gaussians(seed=0, N=200):
    """Positions in +-0.6, opacity in 0.05 - 1, log-uniform scales in 0.02 - 0.25, random quaternions, random rgb."""
    rng = np.random.default_rng(seed)
    g = np.zeros((N, 14))
    g[:, :3] = rng.uniform(-0.6, 0.6, (N, 3))
    g[:, 3] = rng.uniform(0.05, 1, N)
    g[:, 4:7] = np.exp(rng.uniform(np.log(0.02), np.log(0.25), (N, 3)))
    g[:, 7:11] = rng.normal(size=(N, 4))
    g[:, 11:14] = rng.uniform(0, 1, (N, 3))
    return g.astype(np.float32)


def one_gaussian(o=0.9, s=(0.2, 0.2, 0.2), q=(1, 0, 0, 0), mu=(0, 0, 0), rgb=(0.8, 0.4, 0.1)):
    g = np.zeros((1, 14), np.float32)
    g[0, :3], g[0, 3], g[0, 4:7], g[0, 7:11], g[0, 11:14] = mu, o, s, q, rgb
    return g


def density_cases():
    """name -> (gaussians [N, 14] float32, G, scale_modifier): the density cases both test files run."""
    rng = np.random.default_rng(7)
    base = random_gaussians(0)
    cases = {"rand32": (base, (32, 32, 32), 1.0), "ragged": (base, (20, 12, 9), 1.0), "tiny": (base, (3, 3, 3), 1.0),
             "half": (base, (20, 12, 9), 0.5)}
    # 320 small Gaussians inside the first brick of a 24^3 grid (nodes 0..7: x in [-1, -0.39]): five LDS chunks
    many = random_gaussians(1, 320)
    many[:, :3] = rng.uniform(-0.9, -0.5, (320, 3))
    many[:, 4:7] = np.exp(rng.uniform(np.log(0.03), np.log(0.1), (320, 3)))
    cases["chunks"] = (many, (24, 24, 24), 1.0)
    # a 100:1 needle at an oblique rotation, with a few ordinary Gaussians around it
    needle = np.concatenate([one_gaussian(0.8, (0.4, 0.004, 0.004), (0.9, 0.3, -0.2, 0.25), (0.1, -0.05, 0.02)),
                             random_gaussians(2, 8)])
    cases["needle"] = (needle, (32, 32, 32), 1.0)
    # wholly outside the box, straddling its faces, and the rows the kernel must skip
    edge = random_gaussians(3, 24)
    edge[:8, 0] = np.where(np.arange(8) % 2 == 0, 3.0, -3.0)  # outside
    edge[8:16, :3] = np.sign(edge[8:16, :3]) * rng.uniform(0.95, 1.05, (8, 3))  # straddling faces and corners
    edge[8:16, 4:7] = 0.2
    edge[16, 3] = 1e-4  # o <= eps
    edge[17, 3] = 5e-5
    edge[18, 5] = np.nan
    edge[19, 0] = np.inf
    edge[20, 4] = 0.0  # zero scale
    edge[21, 6] = -0.1
    edge[22, 7:11] = 0.0  # zero quaternion
    edge[23, 12] = np.nan
    cases["edge"] = (edge, (20, 12, 9), 1.0)
    # more Gaussians on a brick than the LDS sort holds (LGM_MESH_SORT_CAP = 4096): the kernel's other list path. The
    # grid is tiny, so the fp64 reference still takes a moment only
    wide = random_gaussians(4, 4200)
    wide[:, 4:7] = rng.uniform(1.0, 2.0, (4200, 3))  # (every cut lies outside the box: no borderline terms)
    cases["over_cap"] = (wide, (9, 10, 9), 1.0)
    cases["empty"] = (np.zeros((0, 14), np.float32), (20, 12, 9), 1.0)
    return cases


@functools.lru_cache(maxsize=None)
def density_reference(name):
    g, G, mod = density_cases()[name]
    return density(g, G, mod=mod)


def check_density(sigma, rgb, name):
    """The issue's bars against the fp64 reference; returns the measured figures (asserts after computing them)."""
    ref_s, ref_c, border = density_reference(name)
    share = float((border > 0).mean())
    err = np.abs(np.asarray(sigma, np.float64) - ref_s)
    bar = 1e-5 * ref_s + 1e-6 + EPS * border
    worst = float((err / bar).max())
    out = {"border_share": share, "sigma_err_over_bar": worst}
    assert share <= 0.01, out
    if rgb is not None:
        m = ref_s > 1e-3
        out["rgb_err"] = float(np.abs(np.asarray(rgb, np.float64) - ref_c)[m].max()) if m.any() else 0.0
    print(name, out)
    assert np.isfinite(np.asarray(sigma)).all()
    assert worst <= 1.0, out
    if rgb is not None:
        assert np.isfinite(np.asarray(rgb)).all()
        assert out["rgb_err"] <= 1e-5, out
    return out


def hand_grids():
    """name -> (sigma float32 [G], rgb float32 [G, 3]): the hand-made extraction grids."""
    rng = np.random.default_rng(11)
    out = {}

    def with_rgb(s):
        return s.astype(np.float32), rng.uniform(0, 1, s.shape + (3,)).astype(np.float32)

    s = np.zeros((5, 6, 7))
    s[2, 3, 3] = 1.0
    out["single"] = with_rgb(s)  # 8 vertices, 12 quads
    s = np.zeros((6, 5, 7))
    s[0:4, 0:3, 2:7] = rng.uniform(0.7, 2.0, (4, 3, 5))
    out["block_at_boundary"] = with_rgb(s)
    i, j, k = np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij")
    out["checkerboard"] = with_rgb(np.where((i + j + k) % 2 == 0, 0.9, 0.1) + rng.uniform(0, 0.05, (7, 6, 5)))
    out["all_outside"] = with_rgb(np.full((4, 5, 3), 0.1))
    out["all_inside"] = with_rgb(rng.uniform(0.6, 3.0, (5, 4, 6)))
    return out


def check_extraction(V, C, F, sigma, rgb, iso, bound=1.0):
    """The issue's bars for an extraction (V, C, F) of the fp32 grid against the fp32 restatement; returns the
    restatement."""
    rv, rc, rf = extract(sigma, rgb, iso, bound, np.float32)
    V, F = np.asarray(V), np.asarray(F)
    assert V.shape == rv.shape, (V.shape, rv.shape)  # Nv
    assert F.shape == rf.shape and (F.astype(np.int64) == rf).all()
    extent = 2.0 * bound
    if len(rv):
        dv = float(np.abs(V.astype(np.float64) - rv.astype(np.float64)).max())
        assert dv <= 1e-6 * extent, dv
        if rgb is not None:
            dc = float(np.abs(np.asarray(C, np.float64) - rc.astype(np.float64)).max())
            assert dc <= 1e-6, dc
    check_invariants(V, F)
    return rv, rc, rf


def check_invariants(V, F):
    closed, _, _, vol, in_range = invariants(V, F)
    assert closed and in_range
    assert len(F) == 0 or vol > 0, vol


E2E = {"ragged": (0, 200, (20, 12, 9)), "cube32": (5, 60, (32, 32, 32))}  # seed, N, grid: see test_end_to_end
ISO = 0.5


def e2e_reference(name):
    """The fp64 mesh of an end-to-end case and the distance of the restatement's own fp32 run from it."""
    if name not in _E2E_CACHE:
        seed, N, G = E2E[name]
        g = random_gaussians(seed, N)
        s64, c64, _ = density(g, G)
        margin = float(np.abs(s64 - ISO).min() / ISO)
        v64, col64, f64 = extract(s64, c64, ISO, dtype=np.float64)
        v32, _, f32 = extract(s64.astype(np.float32), c64.astype(np.float32), ISO, dtype=np.float32)
        assert (f32 == f64).all()
        _E2E_CACHE[name] = (g, G, margin, v64, col64, f64, float(np.abs(v32.astype(np.float64) - v64).max()))
    return _E2E_CACHE[name]


_E2E_CACHE = {}


def check_sphere(V, F, C):
    """One Gaussian, o = 0.9, s = 0.2 at the origin, iso = 0.3 on 24^3: a sphere of radius 0.2 sqrt(2 ln 3)."""
    closed, twice, euler, vol, in_range = invariants(V, F)
    assert closed and twice and in_range and euler == 2 and vol > 0
    radius, h = 0.2 * np.sqrt(2 * np.log(3.0)), 2.0 / 23
    assert np.abs(np.linalg.norm(np.asarray(V, np.float64), axis=1) - radius).max() <= np.sqrt(3.0) * h
    assert np.abs(np.asarray(C) - np.array([0.8, 0.4, 0.1], np.float32)).max() <= 1e-6
