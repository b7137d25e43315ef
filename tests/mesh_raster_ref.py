"""include/lgm_meshraster.h restated in numpy, forward and backward, in fp64 (or, with dtype=np.float32, in the header's
own precision: the difference between the two is the rounding error a correct fp32 implementation may show, from which
the tests take their tolerances). Dense: every face against every pixel, in chunks of faces. Not a test module.

forward(...) also returns the per-pixel *ambiguous* mask: a pixel where, for any face, an e_i / A lies within AMB of 0,
or where the two smallest depths differ by less than AMB relative: there fp32 and fp64 may legitimately pick different
faces. The scenes of tests/test_mesh_raster.py and tests/test_mesh_raster_gpu.py are built here too, and their
references computed once."""
import functools

import numpy as np
import torch

AMB = 1e-5
CHUNK = 128


def project(vertices, cv, cvp, H, W, dt=np.float64):
    """(X, Y, w, z) [V, Nv] and the mask of vertices that are not cut."""
    x, y, z = (vertices[:, k].astype(dt)[None] for k in range(3))
    cv, cvp = cv.astype(dt), cvp.astype(dt)

    def col(M, c):
        return M[:, 0, c, None] * x + M[:, 1, c, None] * y + M[:, 2, c, None] * z + M[:, 3, c, None]

    with np.errstate(all="ignore"):
        w, zv = col(cvp, 3), col(cv, 2)
        X = (((col(cvp, 0) / w).astype(np.float64) + 1.0) * W - 1.0) * 0.5
        Y = (((col(cvp, 1) / w).astype(np.float64) + 1.0) * H - 1.0) * 0.5
        X, Y = X.astype(dt), Y.astype(dt)
        ok = (w > 0.2) & np.isfinite(w) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(zv)
    return X, Y, w, zv, ok


def hit(P, px, py):
    """Coverage, b, beta and depth of the header; P = three (X, Y, w, z) tuples broadcast against the pixels."""
    (X0, Y0, w0, z0), (X1, Y1, w1, z1), (X2, Y2, w2, z2) = P
    with np.errstate(all="ignore"):
        x0, y0, x1, y1, x2, y2 = X0 - px, Y0 - py, X1 - px, Y1 - py, X2 - px, Y2 - py
        e0, e1, e2 = x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0
        A = (e0 + e1) + e2
        b = (e0 / A, e1 / A, e2 / A)
        q0, q1, q2 = b[0] / w0, b[1] / w1, b[2] / w2
        iw = (q0 + q1) + q2
        beta = (q0 / iw, q1 / iw, q2 / iw)
        depth = (beta[0] * z0 + beta[1] * z1) + beta[2] * z2
        cov = (A != 0) & (b[0] >= 0) & (b[1] >= 0) & (b[2] >= 0) & (depth > 0) & np.isfinite(depth)
    return cov, A, b, beta, depth


def bilinear(u, v, Ht, Wt, dt):
    """The four texel indices (into the [Ht Wt, 3] texture) and weights of the header's fetch."""
    tx, ty = u * dt(Wt) - dt(0.5), (dt(1.0) - v) * dt(Ht) - dt(0.5)
    flx, fly = np.floor(tx), np.floor(ty)
    fx, fy = tx - flx, ty - fly
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    x0, x1 = np.clip(ix, 0, Wt - 1), np.clip(ix + 1, 0, Wt - 1)
    y0, y1 = np.clip(iy, 0, Ht - 1), np.clip(iy + 1, 0, Ht - 1)
    one = dt(1.0)
    return ((y0 * Wt + x0, y0 * Wt + x1, y1 * Wt + x0, y1 * Wt + x1),
            ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy))


def forward(vertices, faces, cv, cvp, bg, H, W, uvs=None, face_uvs=None, texture=None, colors=None, dt=np.float64,
            near=False, window=False):
    """The header's forward. Returns image [V, 3, H, W], alpha, depth [V, 1, H, W], face_id [V, H, W], ambiguous
    [V, H, W] bool, taps = (view, pixel, idx [n][K], wgt [n][K]) of the covered pixels for backward(), and with
    near=True `near` [Nf] bool: the faces that, in some view, cover a pixel to within AMB (every b_i >= -AMB) at a depth
    within 2 AMB relative of the pixel's smallest: the faces either precision may show. window=True evaluates a chunk
    of faces only on the pixel rows and columns its boxes reach, widened by two pixels (no face covers a pixel outside
    its box in either precision): much faster on small triangles, but the ambiguous mask then leaves out the pixels that
    lie on the extension of a distant face's edge, so the tests that use the mask do not set it."""
    V, Nv, Nf = cv.shape[0], vertices.shape[0], faces.shape[0]
    textured = texture is not None
    X, Y, w, zv, ok = project(vertices, cv, cvp, H, W, dt)
    fl = faces.astype(np.int64)
    valid = ((fl >= 0) & (fl < Nv)).all(axis=1) if Nf else np.zeros(0, bool)
    if textured and Nf:
        valid &= ((face_uvs >= 0) & (face_uvs < uvs.shape[0])).all(axis=1)
    ids = np.nonzero(valid)[0]
    px = np.tile(np.arange(W), H).astype(dt)[None]
    py = np.repeat(np.arange(H), W).astype(dt)[None]
    P_ = H * W
    d1 = np.full((V, P_), np.inf)
    d2 = np.full((V, P_), np.inf)
    f1 = np.full((V, P_), -1, np.int64)
    amb = np.zeros((V, P_), bool)
    near_f = np.zeros(Nf, bool)

    def chunks(v):
        step = CHUNK // 8 if window else CHUNK  # (short chunks: small unions of boxes)
        for c0 in range(0, len(ids), step):
            f = ids[c0:c0 + step]
            tri = fl[f]
            keep = ok[v][tri].all(axis=1)
            f, tri = f[keep], tri[keep]
            if len(f):
                P = tuple(tuple(a[v][tri[:, k]][:, None] for a in (X, Y, w, zv)) for k in range(3))
                xs = np.stack([P[k][0] for k in range(3)])
                ys = np.stack([P[k][1] for k in range(3)])
                sel = slice(None)
                if window:
                    sel = np.nonzero((px[0] >= xs.min() - 2) & (px[0] <= xs.max() + 2) & (py[0] >= ys.min() - 2) &
                                     (py[0] <= ys.max() + 2))[0]
                box = (px[:, sel] >= xs.min(0)) & (px[:, sel] <= xs.max(0)) & (py[:, sel] >= ys.min(0)) & \
                    (py[:, sel] <= ys.max(0))
                yield f, P, box, sel

    for v in range(V):
        for f, P, box, sel in chunks(v):
            cov, A, b, _, depth = hit(P, px[:, sel], py[:, sel])
            cov &= box
            with np.errstate(all="ignore"):
                amb[v, sel] |= ((A != 0) & ((np.abs(b[0]) < AMB) | (np.abs(b[1]) < AMB) |
                                            (np.abs(b[2]) < AMB))).any(axis=0)
            d = np.where(cov, depth.astype(np.float64), np.inf)
            if d.shape[0] > 1:
                part = np.partition(d, 1, axis=0)
                c1, c2 = part[0], part[1]
            else:
                c1, c2 = d[0], np.full(d.shape[1], np.inf)
            cf = f[np.argmin(d, axis=0)]  # (the first minimum: the smallest face index among equal depths)
            o1, o2 = d1[v, sel], d2[v, sel]
            better = c1 < o1
            d2[v, sel] = np.minimum(np.minimum(o2, c2), np.where(better, o1, c1))
            f1[v, sel] = np.where(better, cf, f1[v, sel])
            d1[v, sel] = np.where(better, c1, o1)
        if near:
            for f, P, box, sel in chunks(v):
                _, A, b, _, depth = hit(P, px[:, sel], py[:, sel])
                with np.errstate(all="ignore"):
                    almost = (A != 0) & (b[0] >= -AMB) & (b[1] >= -AMB) & (b[2] >= -AMB) & \
                        (depth <= d1[v, sel][None] * (1 + 2 * AMB))
                near_f[f] |= almost.any(axis=1)
    covered = np.isfinite(d1)
    with np.errstate(all="ignore"):
        amb |= covered & np.isfinite(d2) & ((d2 - d1) < AMB * d1)
    # shading of the winners
    vi, pi = np.nonzero(covered)
    f = f1[vi, pi]
    tri = fl[f] if len(f) else np.zeros((0, 3), np.int64)
    P = tuple(tuple(a[vi, tri[:, k]] for a in (X, Y, w, zv)) for k in range(3))
    _, _, _, beta, depth = hit(P, (pi % W).astype(dt), (pi // W).astype(dt))
    if textured:
        Ht, Wt = texture.shape[0], texture.shape[1]
        fu = face_uvs.astype(np.int64)[f] if len(f) else np.zeros((0, 3), np.int64)
        uv = [uvs[fu[:, k]].astype(dt) for k in range(3)]
        u = (beta[0] * uv[0][:, 0] + beta[1] * uv[1][:, 0]) + beta[2] * uv[2][:, 0]
        t = (beta[0] * uv[0][:, 1] + beta[1] * uv[1][:, 1]) + beta[2] * uv[2][:, 1]
        idx, wgt = bilinear(u, t, Ht, Wt, dt)
        src = texture.reshape(-1, 3).astype(dt)
    else:
        idx, wgt = tuple(tri[:, k] for k in range(3)), beta
        src = colors.astype(dt)
    col = wgt[0][:, None] * src[idx[0]]
    for k in range(1, len(idx)):
        col = col + wgt[k][:, None] * src[idx[k]]
    image = np.broadcast_to(np.asarray(bg, dt).reshape(1, 1, 3), (V, P_, 3)).copy()
    image[vi, pi] = col
    dep = np.zeros((V, P_), dt)
    dep[vi, pi] = depth
    out = {"image": image.transpose(0, 2, 1).reshape(V, 3, H, W), "alpha": covered.astype(dt).reshape(V, 1, H, W),
           "depth": dep.reshape(V, 1, H, W), "face_id": np.where(covered, f1, -1).astype(np.int32).reshape(V, H, W),
           "ambiguous": amb.reshape(V, H, W), "taps": (vi, pi, np.stack(idx, 1), np.stack(wgt, 1))}
    if near:
        out["near"] = near_f
    return out


def backward(fwd, d_image, n_rows, dt=np.float64):
    """The header's backward on the visibility of `fwd`: d_param [n_rows, 3] (n_rows = Ht Wt or Nv)."""
    vi, pi, idx, wgt = fwd["taps"]
    V = d_image.shape[0]
    d = d_image.reshape(V, 3, -1).transpose(0, 2, 1)[vi, pi].astype(dt)  # [n, 3]
    out = np.zeros((n_rows, 3), dt)
    for k in range(idx.shape[1]):
        np.add.at(out, idx[:, k], wgt[:, k, None].astype(dt) * d)
    return out


# --------------------------------------------------------------------------------------------------------- scenes
def cameras(elevations, azimuths, radius=1.5):
    """cam_view, cam_view_proj [V, 4, 4] float32 CPU tensors of orbit poses. None of the angles used by the tests is a
    multiple of 45 degrees: a grid-aligned camera looking down an axis puts whole rows of a surface-nets mesh's edges on
    pixel centres."""
    from lgm_amd.cameras import orbit_cameras_batched
    cv, cvp, _ = orbit_cameras_batched(torch.tensor(elevations, dtype=torch.float64),
                                       torch.tensor(azimuths, dtype=torch.float64), radius)
    return cv, cvp


HAND_CAMS = ((-13.0, 21.0), (17.0, 205.0))
NETS_CAMS = ((-23.0, 11.0), (37.0, 161.0))


def hand_scene(textured):
    """The hand-made scene: a quad of two large triangles that fills the screen, a small triangle in front of it (as
    the first camera sees it) and one behind, a zero-area triangle (a repeated vertex), a triangle with one vertex
    behind the first camera's near cut (dropped whole there; it passes through the quad, and the second camera draws the
    part on its side), and two faces with an
    out-of-range index. In texture mode every vertex has its own uv (some outside [0, 1]: clamp to edge) and one more
    face has a face_uvs entry out of range."""
    from lgm_amd.mesh import Mesh
    el, az = np.deg2rad(HAND_CAMS[0][0]), np.deg2rad(HAND_CAMS[0][1])
    campos = 1.5 * np.array([np.cos(el) * np.sin(az), -np.sin(el), np.cos(el) * np.cos(az)])
    v = np.array([[-1.5, -1.5, 0.0], [1.5, -1.5, 0.0], [1.5, 1.5, 0.0], [-1.5, 1.5, 0.0],
                  [-0.2, -0.1, 0.4], [0.25, -0.15, 0.4], [0.0, 0.3, 0.45],
                  [-0.3, -0.2, -0.4], [0.1, -0.35, -0.45], [0.15, 0.25, -0.4],
                  [0.1, 0.1, 0.2], [0.3, 0.4, 0.2],
                  [0.3, -0.3, -0.2], [-0.35, 0.2, -0.25], list(campos * (1.4 / 1.5)),
                  [0.4, 0.4, 0.3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 11], [12, 13, 14], [0, 1, 99], [-1, 2, 3],
                  [4, 6, 15]], np.int32)
    rng = np.random.default_rng(3)
    colors = rng.random((len(v), 3)).astype(np.float32)
    if not textured:
        return Mesh(torch.from_numpy(v), torch.from_numpy(f[:8]), torch.from_numpy(colors))
    uvs = (rng.random((len(v), 2)) * 1.2 - 0.1).astype(np.float32)
    fu = f.copy()
    fu[6] = [0, 1, 2]  # (the faces with a bad vertex index have good uvs)
    fu[7] = [1, 2, 3]
    fu[8] = [4, 6, len(v)]  # a good face with a face_uvs entry out of range: dropped
    tex = rng.random((5, 7, 3)).astype(np.float32)
    return Mesh(torch.from_numpy(v), torch.from_numpy(f), None, torch.from_numpy(uvs), torch.from_numpy(fu),
                torch.from_numpy(tex))


@functools.lru_cache(maxsize=None)
def nets_gaussians():
    """A few dozen synthetic Gaussians, their scales enlarged so that a resolution-24 grid resolves them."""
    from lgm_amd.synthetic import synthetic_gaussians
    g = synthetic_gaussians(1, 48, seed=0)[0].clone()
    g[:, 4:7] *= 6.0
    return g


@functools.lru_cache(maxsize=None)
def nets_mesh(texels):
    from lgm_amd.mesh import gaussians_to_mesh
    return gaussians_to_mesh(nets_gaussians(), resolution=24, texels=texels)


def pixel_cameras(H, W):
    """Two cameras under which a vertex (x, y, z) lands on the pixel ((x + 1) W - 1) / 2 (+ 0.3 in the second view),
    ((y + 1) H - 1) / 2 with w = 1 and view depth z: vertices can be placed in pixel units."""
    cv = torch.eye(4).repeat(2, 1, 1)
    cvp = torch.zeros(2, 4, 4)
    cvp[:, 0, 0] = cvp[:, 1, 1] = cvp[:, 2, 2] = cvp[:, 3, 3] = 1.0
    cvp[1, 3, 0] = 0.6 / W
    return cv, cvp


def boxes_scene(H=33, W=47):
    """Triangles whose pixel boxes sit on both sides of LGM_MESHRASTER_SMALL_BOX = 64 pixels (8 x 8, 8 x 9, 9 x 9,
    13 x 5, 1 x 64, 1 x 65), overlapping at different depths, one reaching far outside the image on every side and one
    wholly outside it: the switch between the kernels' two visibility paths and the clipping of a box to the image."""
    from lgm_amd.mesh import Mesh

    def tri(x0, y0, x1, y1, z, flip=False):  # a right triangle whose box is [x0, x1] x [y0, y1] in pixel units
        p = [(x0, y0), (x1, y0 + 0.37), (x0 + 0.41, y1)]
        if flip:
            p = [p[0], p[2], p[1]]
        return [[(2 * x + 1) / W - 1, (2 * y + 1) / H - 1, z] for x, y in p]

    boxes = [(2.5, 2.5, 10.4, 10.4, 1.0), (6.5, 4.5, 14.4, 13.4, 0.9, True), (9.5, 9.5, 18.4, 18.4, 1.1),
             (20.5, 3.5, 33.4, 8.4, 0.8), (-0.5, 20.3, 63.6, 20.9, 0.7), (-10.0, 24.2, 54.5, 24.8, 0.7),
             (-900.0, -700.0, 4000.0, 3000.0, 2.0, True), (60.0, 5.0, 70.0, 9.0, 0.5), (30.2, 10.1, 36.9, 17.8, 0.6)]
    v = np.asarray([p for b in boxes for p in tri(*b)], np.float32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    colors = np.random.default_rng(5).random((len(v), 3)).astype(np.float32)
    return Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(colors))


CASES = {  # name: (mesh builder, cameras, H, W)
    "boxes_33x47": (boxes_scene, None, 33, 47),
    "hand_colour_40x72": (lambda: hand_scene(False), HAND_CAMS, 40, 72),
    "hand_colour_64x64": (lambda: hand_scene(False), HAND_CAMS, 64, 64),
    "hand_texture_40x72": (lambda: hand_scene(True), HAND_CAMS, 40, 72),
    "hand_texture_64x64": (lambda: hand_scene(True), HAND_CAMS, 64, 64),
    "nets_texels2_64x64": (lambda: nets_mesh(2), NETS_CAMS, 64, 64),
    "nets_texels2_48x80": (lambda: nets_mesh(2), NETS_CAMS, 48, 80),
    "nets_texels4_64x64": (lambda: nets_mesh(4), NETS_CAMS, 64, 64),
    "nets_texels4_48x80": (lambda: nets_mesh(4), NETS_CAMS, 48, 80),
}
BG = (0.2, 0.5, 0.8)


def mesh_numpy(mesh):
    a = {"vertices": mesh.vertices.numpy(), "faces": mesh.faces.numpy()}
    if mesh.texture is not None:
        a.update(uvs=mesh.uvs.numpy(), face_uvs=mesh.face_uvs.numpy(), texture=mesh.texture.numpy())
    else:
        a.update(colors=mesh.colors.numpy())
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh, cam_view, cam_view_proj, H, W, ref64, ref32, d_image): the scene, the header evaluated in fp64 and in fp32
    and a seeded upstream gradient, zero on the ambiguous pixels. Computed once; treat as read-only."""
    build, cams, H, W = CASES[name]
    mesh = build()
    cv, cvp = pixel_cameras(H, W) if cams is None else cameras([c[0] for c in cams], [c[1] for c in cams])
    a = mesh_numpy(mesh)
    ref64 = forward(cv=cv.numpy(), cvp=cvp.numpy(), bg=BG, H=H, W=W, **a)
    ref32 = forward(cv=cv.numpy(), cvp=cvp.numpy(), bg=BG, H=H, W=W, dt=np.float32, **a)
    d = np.random.default_rng(7).standard_normal((cv.shape[0], 3, H, W)).astype(np.float32)
    d *= ~ref64["ambiguous"][:, None]
    return mesh, cv, cvp, H, W, ref64, ref32, d


def n_rows(mesh):
    return mesh.texture.shape[0] * mesh.texture.shape[1] if mesh.texture is not None else mesh.vertices.shape[0]


# --------------------------------------------------------------------------------------------------------- checks
def on(mesh, dev):
    """The mesh's tensors on `dev`."""
    from dataclasses import replace
    mv = lambda t: None if t is None else t.to(dev)
    return replace(mesh, vertices=mv(mesh.vertices), faces=mv(mesh.faces), colors=mv(mesh.colors), uvs=mv(mesh.uvs),
                   face_uvs=mv(mesh.face_uvs), texture=mv(mesh.texture))


def self_difference(name):
    """(image, depth): the largest difference of the header evaluated in fp32 and in fp64 on the case's non-ambiguous
    pixels (depth: relative). A correct fp32 implementation is this far from fp64, give or take the order of a few
    operations; the tests allow twice it."""
    _, _, _, _, _, r64, r32, _ = case(name)
    ok = ~r64["ambiguous"]
    assert np.array_equal(r64["face_id"][ok], r32["face_id"][ok]), "the reference disagrees with itself off the mask"
    e_img = float(np.abs(r64["image"] - r32["image"]).max(axis=1)[ok].max())
    hit = ok & (r64["face_id"] >= 0)
    e_dep = float((np.abs(r64["depth"] - r32["depth"])[:, 0][hit] / r64["depth"][:, 0][hit]).max())
    return e_img, e_dep


def check_forward(name, dev):
    """render_mesh on `dev` against the fp64 reference: the ambiguous share, face_id, alpha, image and depth off the
    mask, the background, and two calls bit for bit."""
    from lgm_amd.meshraster import render_mesh
    mesh, cv, cvp, H, W, r64, _, _ = case(name)
    m = on(mesh, dev)
    out = render_mesh(m, cv.to(dev), cvp.to(dev), H, W, BG)
    again = render_mesh(m, cv[None].to(dev), cvp[None].to(dev), H, W, BG)  # ([1, V, 4, 4] cameras too)
    for k in ("image", "alpha", "depth", "face_id"):
        assert torch.equal(out[k], again[k]), k
    img, alpha = out["image"].detach().cpu().numpy(), out["alpha"].cpu().numpy()
    depth, fid = out["depth"].cpu().numpy(), out["face_id"].cpu().numpy()
    assert img.shape == r64["image"].shape and fid.dtype == np.int32
    ok = ~r64["ambiguous"]
    covered = r64["face_id"] >= 0
    share = float((covered & ~ok).sum() / max(covered.sum(), 1))
    e_img, e_dep = self_difference(name)
    hit = ok & covered
    d_img = float(np.abs(img - r64["image"]).max(axis=1)[ok].max())
    d_dep = float((np.abs(depth - r64["depth"])[:, 0][hit] / r64["depth"][:, 0][hit]).max()) if hit.any() else 0.0
    print(f"{name} on {dev}: covered {int(covered.sum())} pixels, ambiguous share {share:.4f}; image error {d_img:.3e} "
          f"(fp32 self-difference {e_img:.3e}), depth error {d_dep:.3e} ({e_dep:.3e})")
    assert covered.sum() > 0 and share <= 0.02, share
    assert np.array_equal(fid[ok], r64["face_id"][ok])
    assert np.array_equal(alpha[:, 0][ok], r64["alpha"][:, 0][ok])
    assert set(np.unique(alpha)) <= {0.0, 1.0}
    assert d_img <= 2 * e_img and d_dep <= 2 * e_dep, (d_img, e_img, d_dep, e_dep)
    none = ok & ~covered
    assert np.array_equal(img.transpose(0, 2, 3, 1)[none], np.broadcast_to(np.float32(BG), (int(none.sum()), 3)))
    assert np.all(depth[:, 0][none] == 0) and np.all(fid[none] == -1)
    return out


def param_of(mesh):
    return mesh.texture if mesh.texture is not None else mesh.colors


def with_param(mesh, p):
    from dataclasses import replace
    return replace(mesh, texture=p) if mesh.texture is not None else replace(mesh, colors=p)


def check_backward(name, dev):
    """The gradient to the texture (or the colours) against the reference's backward on the reference's own
    visibility (the upstream gradient is zero on the ambiguous pixels, where the two may draw different faces); a second
    backward on one forward and a second forward + backward, bit for bit."""
    from lgm_amd.meshraster import render_mesh
    mesh, cv, cvp, H, W, r64, r32, d = case(name)
    rows = n_rows(mesh)
    want = backward(r64, d, rows)
    e_bw = float(np.abs(want - backward(r32, d, rows, np.float32)).max())
    m = on(mesh, dev)
    dd = torch.from_numpy(d).to(dev)
    grads = []
    for _ in range(2):
        p = param_of(m).clone().requires_grad_(True)
        loss = (render_mesh(with_param(m, p), cv.to(dev), cvp.to(dev), H, W, BG)["image"] * dd).sum()
        g1, = torch.autograd.grad(loss, p, retain_graph=True)
        g2, = torch.autograd.grad(loss, p)
        assert torch.equal(g1, g2), "a second backward on one forward"
        grads.append(g1)
    assert torch.equal(grads[0], grads[1]), "two calls"
    got = grads[0].cpu().numpy().reshape(rows, 3)
    err = float(np.abs(got - want).max())
    # twice the fp32 self-difference of the reference's backward, and for the order of an fp32 summation 8 ulp of the
    # largest sum of a row's terms' magnitudes (the torch path and numpy add the same terms in different orders; the
    # kernels' fixed-point sums have no order: their unit is at most 2^-30 of the largest |d_image|)
    tol = 2 * e_bw + 2.0 ** -21 * float(backward(r64, np.abs(d), rows).max())
    print(f"{name} on {dev}: gradient error {err:.3e} (fp32 self-difference {e_bw:.3e}, tolerance {tol:.3e}), "
          f"largest {np.abs(want).max():.3e}, nonzero rows {int((want != 0).any(axis=1).sum())} of {rows}")
    assert np.abs(want).max() > 0 and err <= tol, (err, tol)
    assert np.all(got[(want == 0).all(axis=1)] == 0), "a texel (vertex) no pixel reads has a gradient"


def check_adjoint(name, dev):
    """<render(t), d> == <t, backward(d)> for a random t and d over a zero background (the image is linear in t then):
    both sides are sums of the same products, rounded differently; each side's rounding is at most about 16 fp32
    operations per product (4 multiply-adds of the fetch, the product with d, the fixed-point rounding), so the two
    agree to 16 x 2^-24 = 1e-6 of the sum of the products' magnitudes."""
    from lgm_amd.meshraster import render_mesh
    mesh, cv, cvp, H, W, _, _, _ = case(name)
    m = on(mesh, dev)
    gen = torch.Generator().manual_seed(11)
    t = torch.randn(param_of(mesh).shape, generator=gen).to(dev).requires_grad_(True)
    d = torch.randn(cv.shape[0], 3, H, W, generator=gen).to(dev)
    image = render_mesh(with_param(m, t), cv.to(dev), cvp.to(dev), H, W, (0.0, 0.0, 0.0))["image"]
    g, = torch.autograd.grad((image * d).sum(), t)
    lhs = float((image.detach().double() * d.double()).sum())
    rhs = float((t.detach().double() * g.double()).sum())
    scale = float((image.detach().double() * d.double()).abs().sum() + (t.detach().double() * g.double()).abs().sum())
    print(f"{name} on {dev}: <render(t), d> = {lhs:.9e}, <t, backward(d)> = {rhs:.9e}, difference {abs(lhs - rhs):.3e}, "
          f"allowed {1e-6 * scale:.3e}")
    assert scale > 0 and abs(lhs - rhs) <= 1e-6 * scale


def check_hand_scene(dev):
    """What the hand-made scene is for: which faces each camera draws."""
    from lgm_amd.meshraster import render_mesh
    for name in ("hand_colour_64x64", "hand_texture_64x64"):
        mesh, cv, cvp, H, W, r64, _, _ = case(name)
        fid = render_mesh(on(mesh, dev), cv.to(dev), cvp.to(dev), H, W, BG)["face_id"].cpu().numpy()
        for ids in (fid, r64["face_id"]):
            seen = [set(np.unique(ids[v]).tolist()) for v in range(2)]
            assert seen[0] == {0, 1, 2}, seen  # the quad and the triangle in front; the near-cut face is dropped whole
            assert seen[1] == {0, 1, 3, 5}, seen  # from behind: the other triangle, and the face cut in view 0
            assert (ids >= 0).all()  # the quad fills the screen
        # the zero-area face (4), the faces with a bad index (6, 7) and, with a texture, a bad face_uvs entry (8): never


def check_camera_convention(dev):
    """One small isotropic opaque Gaussian and a small triangle around its centre land on the same pixel in
    GaussianRenderer.render and in render_mesh: the two renderers share the camera and pixel convention."""
    from lgm_amd import GaussianRenderer, Options
    from lgm_amd.mesh import Mesh
    from lgm_amd.meshraster import render_mesh
    S = 64
    p = np.array([0.23, -0.31, 0.12], np.float32)
    g = torch.tensor([[*p, 0.99, 0.02, 0.02, 0.02, 1, 0, 0, 0, 1.0, 0.0, 0.0]], dtype=torch.float32)
    r = 0.06  # about 2.8 pixels: the triangle's inscribed circle holds the pixel centre nearest to the projection
    ang = np.deg2rad([90.0, 210.0, 330.0])
    v = p[None] + r * np.stack([np.cos(ang), np.sin(ang), np.zeros(3)], 1).astype(np.float32)
    mesh = Mesh(torch.from_numpy(v), torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.ones(3, 3))
    cv, cvp = cameras([-10.0, 25.0], [20.0, -30.0])
    cp = torch.zeros(1, 2, 3)
    out_g = GaussianRenderer(Options(output_size=S)).render(g[None].to(dev), cv[None].to(dev), cvp[None].to(dev),
                                                            cp.to(dev), bg_color=torch.zeros(3, device=dev))
    alpha = out_g["alpha"][0, :, 0].cpu().numpy()
    fid = render_mesh(on(mesh, dev), cv.to(dev), cvp.to(dev), S, S)["face_id"].cpu().numpy()
    for view in range(2):
        y, x = np.unravel_index(np.argmax(alpha[view]), (S, S))
        assert alpha[view, y, x] > 0.5
        ys, xs = np.nonzero(fid[view] == 0)
        assert fid[view, y, x] == 0, (view, x, y, xs, ys)
        assert 3 <= len(xs) <= 40 and np.abs(xs - x).max() <= 4 and np.abs(ys - y).max() <= 4
        # the centre of the triangle's pixels is the centre of the Gaussian's alpha, within a pixel
        wsum = alpha[view].sum()
        gx = (alpha[view].sum(0) * np.arange(S)).sum() / wsum
        gy = (alpha[view].sum(1) * np.arange(S)).sum() / wsum
        assert abs(xs.mean() - gx) < 1 and abs(ys.mean() - gy) < 1, (xs.mean(), gx, ys.mean(), gy)


FIT = dict(iters=20, views=1, resolution=64, seed=0)


def check_fit_texture(dev):
    """fit_texture on the resolution-24 mesh at 64 x 64, 20 iterations: the loss on the training poses falls, the same
    seed gives the same bits, the texels no pose sees keep their baked value (seen: the texel blocks of the faces the
    reference finds visible, or within rounding of visible, from the poses used), fit_iters = 0 is bake_texture."""
    from lgm_amd import Options
    from lgm_amd.mesh import gaussians_to_mesh
    from lgm_amd.meshraster import _render_gaussians, fit_poses, fit_texture, render_mesh
    opt = Options()
    g = nets_gaussians().to(dev)
    baked = on(nets_mesh(2), dev)
    fitted = fit_texture(baked, g, opt, **FIT)
    again = fit_texture(baked, g, opt, **FIT)
    assert torch.equal(fitted.texture, again.texture), "the same seed"
    assert torch.equal(baked.texture, on(nets_mesh(2), dev).texture), "the input's texture is not touched"
    assert fitted.fit["iters"] == 20 and fitted.fit["loss_first"] > 0
    assert float(fitted.texture.min()) >= 0 and float(fitted.texture.max()) <= 1
    # the loss over the training poses, before and after
    el, az = fit_poses(FIT["iters"], FIT["views"], FIT["seed"])
    cv, cvp = cameras(el.reshape(-1).tolist(), az.reshape(-1).tolist(), opt.cam_radius)
    S = FIT["resolution"]
    white = torch.ones(3, device=dev)
    target = _render_gaussians(g, opt, cv.to(dev), cvp.to(dev), S, S, white)
    mse = [float(((render_mesh(m, cv.to(dev), cvp.to(dev), S, S)["image"] - target) ** 2).mean())
           for m in (baked, fitted)]
    print(f"fit_texture on {dev}: training-pose MSE {mse[0]:.6f} -> {mse[1]:.6f}; first / last iteration loss "
          f"{fitted.fit['loss_first']:.6f} / {fitted.fit['loss_last']:.6f}")
    assert mse[1] < mse[0], mse
    # texels of quads that no pose sees
    a = mesh_numpy(nets_mesh(2))
    ref = forward(cv=cv.numpy(), cvp=cvp.numpy(), bg=BG, H=S, W=S, near=True, window=True, **a)
    T = 2
    Ht, Wt = a["texture"].shape[:2]
    seen_quad = ref["near"].reshape(-1, 2).any(axis=1)
    cols = Wt // T
    seen = np.zeros((Ht // T, cols), bool)
    q = np.nonzero(seen_quad)[0]
    seen[q // cols, q % cols] = True
    seen = np.repeat(np.repeat(seen, T, axis=0), T, axis=1)
    tex0, tex1 = baked.texture.cpu().numpy(), fitted.texture.cpu().numpy()
    changed = (tex0 != tex1).any(axis=2)
    print(f"  {int(seen_quad.sum())} of {len(seen_quad)} quads seen; {int(changed.sum())} of {Ht * Wt} texels changed")
    assert (~seen).sum() > 0 and changed.sum() > 0
    assert not (changed & ~seen).any(), "a texel no pose sees changed"
    # fit_iters = 0: nothing is fitted, bit for bit
    plain = gaussians_to_mesh(g, resolution=24, texels=2)  # (on `dev`: bake_texture's mesh there)
    m0 = gaussians_to_mesh(g, resolution=24, texels=2, fit_iters=0)
    assert torch.equal(m0.texture, plain.texture) and torch.equal(m0.vertices, plain.vertices) and m0.fit is None
    assert torch.equal(m0.faces, plain.faces) and torch.equal(m0.uvs, plain.uvs)
