"""An independent numpy restatement of include/lgm_mesh.h's sampling pass (fp64, with the per-point count of borderline
terms) and atlas (fp32, every operation rounded on its own), the bars of tests/mesh_ref.check_density for points, and the
seeded point sets the CPU and GPU texture tests share. Nothing here imports lgm_amd."""
import functools

import numpy as np

from tests.mesh_ref import EPS, density_cases, grid, one_gaussian, rotation


def sample(g, pts, G, bound=1.0, mod=1.0, eps=EPS):
    """fp64: sigma [M], rgb [M, 3], border [M] = the number of terms with |d2 - rho2| < 1e-4 rho2 at the point,
    inside [M] = the point is sampled (finite, lo - h / 2 <= p <= lo + (G - 1/2) h in fp64)."""
    lo, h = grid(G, bound)
    lo, h = lo.astype(np.float64), h.astype(np.float64)
    eps = float(np.float32(eps))
    P = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    top = np.array([n - 0.5 for n in G])
    with np.errstate(invalid="ignore"):
        inside = (np.isfinite(P) & (P >= lo - h / 2.0) & (P <= lo + top * h)).all(1)
    X = np.where(inside[:, None], P, 0.0)
    sw, swc, border = np.zeros(len(X)), np.zeros((len(X), 3)), np.zeros(len(X), np.int64)
    for row in np.asarray(g, np.float32).astype(np.float64):
        mu, o, s, q, c = row[:3], row[3], row[4:7] * float(mod), row[7:11], row[11:14]
        if not np.isfinite(row).all() or not o > eps or not (s > 0).all() or not (q * q).sum() > 0:
            continue
        y = ((X - mu) @ rotation(q)) / s
        d2 = (y * y).sum(1)
        rho2 = 2.0 * np.log(o / eps)
        m = (d2 <= rho2) & inside
        w = o * np.exp(-0.5 * d2[m])
        sw[m] += w
        swc[m] += w[:, None] * c
        border += (np.abs(d2 - rho2) < 1e-4 * rho2) & inside
    rgb = np.where(sw[:, None] > 0, swc / np.where(sw > 0, sw, 1.0)[:, None], 0.0)
    return sw, rgb, border, inside


def check_sample(sigma, rgb, ref, name=""):
    """tests/mesh_ref.check_density's bars for points against ref = sample(...); returns the measured figures (asserts
    after computing them). Points that are not sampled must be exactly 0."""
    ref_s, ref_c, border, inside = ref
    sigma = np.asarray(sigma)
    share = float((border > 0).mean()) if len(border) else 0.0
    err = np.abs(sigma.astype(np.float64) - ref_s)
    bar = 1e-5 * ref_s + 1e-6 + EPS * border
    worst = float((err / bar).max()) if len(err) else 0.0
    out = {"points": len(ref_s), "border_share": share, "sigma_err_over_bar": worst}
    if rgb is not None:
        m = ref_s > 1e-3
        out["rgb_err"] = float(np.abs(np.asarray(rgb, np.float64) - ref_c)[m].max()) if m.any() else 0.0
    print(name, out)
    assert share <= 0.01, out
    assert np.isfinite(sigma).all()
    assert worst <= 1.0, out
    assert (sigma[~inside] == 0).all()
    if rgb is not None:
        assert np.isfinite(np.asarray(rgb)).all()
        assert out["rgb_err"] <= 1e-5, out
        assert (np.asarray(rgb)[~inside] == 0).all()
    return out


# ------------------------------------------------------------------------------------------------- shared inputs
def uniform_points(M=6000):
    return np.random.default_rng(11).uniform(-1.0, 1.0, (M, 3)).astype(np.float32)


def sample_cases():
    """name -> (gaussians, G, scale_modifier, points): every density case with 6,000 uniform points (1,500 for the
    walk-all path); `chunks` with 1,000 more inside its first brick, so that one workgroup takes several batches."""
    out = {}
    for name, (g, G, mod) in density_cases().items():
        pts = uniform_points(1500 if name == "over_cap" else 6000)
        if name == "chunks":
            extra = np.random.default_rng(12).uniform(-1.0, -0.4, (1000, 3)).astype(np.float32)
            pts = np.concatenate([pts, extra])
        out[name] = (g, G, mod, pts)
    return out


@functools.lru_cache(maxsize=None)
def sample_reference(name):
    g, G, mod, pts = sample_cases()[name]
    return sample(g, pts, G, mod=mod)


GAP = (one_gaussian(0.9, (0.02343,) * 3, mu=(-0.25, 0.0, 0.0)), (24, 24, 24),
       np.array([[-0.34, 0, 0], [-0.36, 0, 0]], np.float32))


def special_points(G, bound=1.0):
    """Points of the grid's own geometry, as a dict of float32 arrays: nodes, brick faces (node coordinate 8) and one
    ulp either side, the box faces lo - h / 2 and lo + (G - 1/2) h rounded to fp32, one ulp inwards and one outwards
    of those, and points with a NaN or an infinity."""
    lo, h = grid(G, bound)
    lo64, h64 = lo.astype(np.float64), h.astype(np.float64)
    rng = np.random.default_rng(13)
    idx = np.stack([rng.integers(0, n, 64) for n in G], 1)
    nodes = (lo64 + idx * h64).astype(np.float32)
    face = nodes.copy()
    for k in range(len(face)):  # one coordinate onto a brick face
        a = k % 3
        if G[a] > 8:
            face[k, a] = np.float32(lo64[a] + 8 * h64[a])
    big = np.float32(np.inf)
    below, above = np.nextafter(face, -big), np.nextafter(face, big)
    box_lo, box_hi = (lo64 - h64 / 2.0).astype(np.float32), (lo64 + (np.array(G) - 0.5) * h64).astype(np.float32)
    on_box, inward, outward = [], [], []
    for a in range(3):
        for edge, sign in ((box_lo, -1.0), (box_hi, 1.0)):
            p = nodes[:8].copy()
            p[:, a] = edge[a]
            on_box.append(p)
            q = p.copy()
            q[:, a] = np.nextafter(edge[a], np.float32(-sign) * big)
            inward.append(q)
            q = p.copy()
            q[:, a] = np.nextafter(edge[a], np.float32(sign) * big)
            outward.append(q)
    bad = nodes[:6].copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, 1] = np.nan, np.inf, -np.inf, np.nan, np.inf
    bad[5] = np.nan
    return {"nodes": nodes, "face": face, "face_below": below, "face_above": above, "on_box": np.concatenate(on_box),
            "inward": np.concatenate(inward), "outward": np.concatenate(outward), "bad": bad}


# ------------------------------------------------------------------------------------------------- atlas
def atlas_shape(nq, T):
    cols = 1
    while cols * cols < nq:  # ceil(sqrt(nq)), at least 1
        cols += 1
    rows = max(1, -(-nq // cols))
    return cols, rows, cols * T, rows * T


def quads(F):
    """[nq, 4] (q0, q1, q2, q3) and outward [nq] of faces in pairs; raises AssertionError on anything else."""
    F = np.asarray(F, np.int64)
    assert len(F) % 2 == 0
    p = F.reshape(-1, 6)
    outward = p[:, 2] == p[:, 4]
    flipped = ~outward & (p[:, 1] == p[:, 5])
    assert (p[:, 0] == p[:, 3]).all() and (outward | flipped).all()
    q = np.where(outward[:, None], p[:, [0, 1, 2, 5]], p[:, [0, 2, 1, 4]])
    return q, outward


def atlas(V, F, T, cols, rows):
    """fp32, every operation rounded on its own: points [nq, T, T, 3] (texel (i, j) at [q, j, i]), uvs [nq, 4, 2],
    face_uvs [nf, 3]."""
    f32 = np.float32
    V = np.asarray(V, f32)
    q, outward = quads(F)
    nq = len(q)
    points = np.zeros((nq, T, T, 3), f32)
    one = f32(1)
    for j in range(T):
        for i in range(T):
            s, t = f32(i) / f32(T - 1), f32(j) / f32(T - 1)
            if s >= t:
                w0, w1, w2, mid = one - s, s - t, t, q[:, 1]
            else:
                w0, w1, w2, mid = one - t, t - s, s, q[:, 3]
            points[:, j, i] = (f32(w0) * V[q[:, 0]] + f32(w1) * V[mid]) + f32(w2) * V[q[:, 2]]
    n = np.arange(nq)
    x0, y0 = ((n % cols) * T).astype(f32), ((n // cols) * T).astype(f32)
    uvs = np.zeros((nq, 4, 2), f32)
    for k, (a, b) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
        x = (x0 + f32(0.5)) + f32(a * (T - 1))
        y = (y0 + f32(0.5)) + f32(b * (T - 1))
        uvs[:, k, 0] = x / f32(cols * T)
        uvs[:, k, 1] = one - y / f32(rows * T)
    corner = np.where(outward[:, None], np.array([[0, 1, 2, 0, 2, 3]]), np.array([[0, 2, 1, 0, 3, 2]]))
    face_uvs = (4 * n[:, None] + corner).reshape(-1, 3)
    assert points.dtype == f32 and uvs.dtype == f32
    return points, uvs, face_uvs


def check_atlas(points, uvs, face_uvs, V, F, T):
    """The atlas of (V, F) against the restatement and its own geometry; returns (cols, rows, W, H)."""
    V, F = np.asarray(V, np.float32), np.asarray(F, np.int64)
    nq = len(F) // 2
    cols, rows, W, H = atlas_shape(nq, T)
    rp, ru, rf = atlas(V, F, T, cols, rows)
    points, uvs, face_uvs = np.asarray(points), np.asarray(uvs).reshape(-1, 4, 2), np.asarray(face_uvs)
    assert points.shape == rp.shape and points.dtype == np.float32
    assert (points.view(np.uint32) == rp.view(np.uint32)).all()  # bitwise
    assert (uvs == ru).all() and (face_uvs.astype(np.int64) == rf).all()
    q, outward = quads(F)
    assert (points[:, 0, 0] == V[q[:, 0]]).all() and (points[:, T - 1, T - 1] == V[q[:, 2]]).all()
    assert (points[:, 0, T - 1] == V[q[:, 1]]).all() and (points[:, T - 1, 0] == V[q[:, 3]]).all()
    # the diagonal from the other formula: (1 - t) v0 + (t - s) v3 + s v2 with s = t
    f32 = np.float32
    for i in range(T):
        s = f32(i) / f32(T - 1)
        other = ((f32(1) - s) * V[q[:, 0]] + (s - s) * V[q[:, 3]]) + s * V[q[:, 2]]
        assert (points[:, i, i] == other).all()
    # every face corner's uv is the pixel centre of the texel that holds that vertex, inside the face's own block
    flat_uv = uvs.reshape(-1, 2)[face_uvs]  # [nf, 3, 2]
    px = flat_uv[..., 0].astype(np.float64) * W - 0.5
    py = (1.0 - flat_uv[..., 1].astype(np.float64)) * H - 0.5
    block = np.repeat(np.arange(nq), 2)[:, None]
    i, j = px - (block % cols) * T, py - (block // cols) * T
    assert np.abs(i - np.round(i)).max() <= 1e-2 and np.abs(j - np.round(j)).max() <= 1e-2
    i, j = np.round(i).astype(int), np.round(j).astype(int)
    assert ((i == 0) | (i == T - 1)).all() and ((j == 0) | (j == T - 1)).all()
    assert (points[block, j, i] == V[F]).all()
    # shared edges: the texels of an edge two quads share are the same 3D points, whichever way each quad runs along
    # it. A texel is a convex combination with three products and two sums, every one rounded (and its weights 1 - s,
    # s - t rounded too): within 8 ulp of the largest coordinate per evaluation, 16 for two
    tol = 16 * 2.0 ** -24 * float(np.abs(V).max()) if len(V) else 0.0
    sides = {}
    line = np.arange(T)
    for n_, (a, b, c, d) in enumerate(q.tolist()):
        for (u, v), pts_ in (((a, b), points[n_, 0, line]), ((b, c), points[n_, line, T - 1]),
                             ((d, c), points[n_, T - 1, line]), ((a, d), points[n_, line, 0])):
            key, run = ((u, v), pts_) if u < v else ((v, u), pts_[::-1])
            sides.setdefault(key, []).append(run)
    shared = [runs for runs in sides.values() if len(runs) > 1]
    assert len(shared) > 0 or nq == 0
    worst = max((float(np.abs(r.astype(np.float64) - runs[0]).max()) for runs in shared for r in runs[1:]), default=0.0)
    print("shared-edge texels: worst distance", worst, "bar", tol)
    assert worst <= tol
    return cols, rows, W, H


def check_texture(texture, points, ref, T, cols, rows):
    """A baked texture [H, W, 3] against ref = sample(gaussians, points, ...) at the atlas's own points: the rgb bar on
    every texel of a block below nq (their share of borderline terms within the bars' condition), zero past nq."""
    ref_s, ref_c, border, inside = ref
    texture = np.asarray(texture)
    nq = points.shape[0]
    assert texture.shape == (rows * T, cols * T, 3) and texture.dtype == np.float32 and np.isfinite(texture).all()
    blocks = texture.reshape(rows, T, cols, T, 3).transpose(0, 2, 1, 3, 4).reshape(rows * cols, T, T, 3)
    assert (blocks[nq:] == 0).all()
    if nq == 0:
        return {}
    out = {"border_share": float((border > 0).mean()), "sigma_min": float(ref_s.min()),
           "rgb_err": float(np.abs(blocks[:nq].reshape(-1, 3).astype(np.float64) - ref_c).max())}
    print(out)
    assert inside.all() and out["border_share"] <= 0.01 and out["sigma_min"] > 1e-3, out
    assert out["rgb_err"] <= 1e-5, out
    return out
