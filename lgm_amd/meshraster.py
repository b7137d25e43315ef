"""Mesh rasteriser and texture fit (include/lgm_meshraster.h): the last stage of the reference's convert.py export
(fit_mesh_uv, convert.py:364-442), which rasterises the UV mesh with nvdiffrast from random orbit cameras and fits the
texture to renders of the Gaussians.

  render_mesh   Mesh, cameras -> {"image" [V,3,H,W], "alpha" [V,1,H,W], "depth" [V,1,H,W], "face_id" [V,H,W]};
                differentiable in mesh.texture (or mesh.colors when there is no texture)
  fit_texture   Mesh with a baked texture, Gaussians -> Mesh whose texture is fitted to the Gaussians' renders
  mesh_psnr     PSNR of the mesh's render against the Gaussians' render on given cameras: the export's quality number

Pixel (x, y) of render_mesh and of GaussianRenderer.render is the same ray (the header's projection is the Gaussian
rasteriser's). GPU tensors run the kernels of lgm_amd/csrc/meshraster.hip (a missing library raises NativeError); CPU
tensors take the dense torch form of the same fp32 operations below. There is no antialiasing and no gradient to
vertices or cameras."""
from __future__ import annotations

import math
from dataclasses import replace
import torch

from . import _native as nat
from ._native import ptr
from .cameras import orbit_cameras_batched
from .mesh import Mesh, _check_gaussians

_NO_HIT = torch.iinfo(torch.int64).max
_FACE_CHUNK = 64  # faces per step of the dense torch path (short: a step looks at the union of its faces' boxes)


# ------------------------------------------------------------------------------------------------------- torch path
def _project_torch(vertices, cv, cvp, H, W):
    """The header's projection in fp32, every operation rounded on its own: (X, Y, w, z) [V, Nv] and the cut mask."""
    x, y, z = (vertices[:, k][None] for k in range(3))

    def col(M, c):
        return M[:, 0, c, None] * x + M[:, 1, c, None] * y + M[:, 2, c, None] * z + M[:, 3, c, None]

    w = col(cvp, 3)
    zv = col(cv, 2)
    X = (((col(cvp, 0) / w).double() + 1.0) * W - 1.0) * 0.5
    Y = (((col(cvp, 1) / w).double() + 1.0) * H - 1.0) * 0.5
    X, Y = X.float(), Y.float()
    ok = (w > 0.2) & torch.isfinite(w) & torch.isfinite(X) & torch.isfinite(Y) & torch.isfinite(zv)
    return X, Y, w, zv, ok


def _hit_torch(P, px, py):
    """The header's coverage, beta and depth (mr_hit of the kernels): P = ((X, Y, w, z) of the three vertices),
    broadcast against the pixel centres. Returns (hit, beta [3], depth)."""
    (X0, Y0, w0, z0), (X1, Y1, w1, z1), (X2, Y2, w2, z2) = P
    x0, y0, x1, y1, x2, y2 = X0 - px, Y0 - py, X1 - px, Y1 - py, X2 - px, Y2 - py
    e0, e1, e2 = x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0
    A = (e0 + e1) + e2
    b0, b1, b2 = e0 / A, e1 / A, e2 / A
    q0, q1, q2 = b0 / w0, b1 / w1, b2 / w2
    iw = (q0 + q1) + q2
    beta = (q0 / iw, q1 / iw, q2 / iw)
    depth = (beta[0] * z0 + beta[1] * z1) + beta[2] * z2
    hit = (A != 0) & (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (depth > 0) & torch.isfinite(depth)
    return hit, beta, depth


def _visibility_torch(vertices, faces, face_uvs, Nu, cv, cvp, H, W):
    """key [V, H W] int64: (fp32 bits of depth) << 32 | face of the visible face, _NO_HIT where none; and the
    projection."""
    V, Nv, Nf = cv.shape[0], vertices.shape[0], faces.shape[0]
    proj = _project_torch(vertices, cv, cvp, H, W)
    X, Y, w, zv, ok = proj
    key = torch.full((V, H * W), _NO_HIT, dtype=torch.int64)
    fl = faces.long()
    valid = ((fl >= 0) & (fl < Nv)).all(dim=1)
    if face_uvs is not None:
        valid &= ((face_uvs >= 0) & (face_uvs < Nu)).all(dim=1)
    px = torch.arange(W, dtype=torch.float32).repeat(H)[None]
    py = torch.arange(H, dtype=torch.float32).repeat_interleave(W)[None]
    ids = valid.nonzero().squeeze(1)
    for v in range(V):
        for c0 in range(0, ids.numel(), _FACE_CHUNK):
            f = ids[c0:c0 + _FACE_CHUNK]
            tri = fl[f]
            keep = ok[v][tri].all(dim=1)
            f, tri = f[keep], tri[keep]
            if f.numel() == 0:
                continue
            P = tuple(tuple(a[v][tri[:, k]][:, None] for a in (X, Y, w, zv)) for k in range(3))
            xs = torch.stack([P[k][0] for k in range(3)]), torch.stack([P[k][1] for k in range(3)])
            # only the pixels inside the union of the chunk's boxes (the header tests a face on its box alone)
            sel = ((px[0] >= xs[0].min()) & (px[0] <= xs[0].max()) & (py[0] >= xs[1].min()) &
                   (py[0] <= xs[1].max())).nonzero().squeeze(1)
            if sel.numel() == 0:
                continue
            qx, qy = px[:, sel], py[:, sel]
            box = (qx >= xs[0].amin(0)) & (qx <= xs[0].amax(0)) & (qy >= xs[1].amin(0)) & (qy <= xs[1].amax(0))
            hit, _, depth = _hit_torch(P, qx, qy)
            k64 = (depth.contiguous().view(torch.int32).long() << 32) | f[:, None]
            k64 = torch.where(hit & box, k64, torch.full((), _NO_HIT, dtype=torch.int64))
            key[v, sel] = torch.minimum(key[v, sel], k64.amin(dim=0))
    return key, proj


def _render_torch(mesh_arrays, param, cv, cvp, bg, H, W):
    """The dense torch path: visibility without a graph, shading in differentiable torch operations on `param` (the
    texture [Ht, Wt, 3] or the colours [Nv, 3]), in the header's operation order."""
    vertices, faces, uvs, face_uvs, textured = mesh_arrays
    V = cv.shape[0]
    with torch.no_grad():
        key, (X, Y, w, zv, _) = _visibility_torch(vertices, faces, face_uvs if textured else None,
                                                  uvs.shape[0] if textured else 0, cv, cvp, H, W)
        hit = key != _NO_HIT
        vi, pi = hit.nonzero(as_tuple=True)
        f = (key[vi, pi] & 0xffffffff)
        tri = faces.long()[f]
        P = tuple(tuple(a[vi, tri[:, k]] for a in (X, Y, w, zv)) for k in range(3))
        px, py = (pi % W).float(), (pi // W).float()
        _, beta, _ = _hit_torch(P, px, py)
        depth = torch.zeros(V, H * W)
        depth[vi, pi] = (key[vi, pi] >> 32).to(torch.int32).view(torch.float32)
        if textured:
            Ht, Wt = param.shape[0], param.shape[1]
            uv = [uvs[face_uvs.long()[f][:, k]] for k in range(3)]
            u = (beta[0] * uv[0][:, 0] + beta[1] * uv[1][:, 0]) + beta[2] * uv[2][:, 0]
            t = (beta[0] * uv[0][:, 1] + beta[1] * uv[1][:, 1]) + beta[2] * uv[2][:, 1]
            tx, ty = u * float(Wt) - 0.5, (1.0 - t) * float(Ht) - 0.5
            flx, fly = torch.floor(tx), torch.floor(ty)
            fx, fy = tx - flx, ty - fly
            ix = flx.clamp(-1.0, float(Wt)).nan_to_num(-1.0).long()
            iy = fly.clamp(-1.0, float(Ht)).nan_to_num(-1.0).long()
            x0, x1 = ix.clamp(0, Wt - 1), (ix + 1).clamp(0, Wt - 1)
            y0, y1 = iy.clamp(0, Ht - 1), (iy + 1).clamp(0, Ht - 1)
            idx = (y0 * Wt + x0, y0 * Wt + x1, y1 * Wt + x0, y1 * Wt + x1)
            wgt = ((1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy)
        else:
            idx = tuple(tri[:, k] for k in range(3))
            wgt = beta
    src = param.reshape(-1, 3)
    col = wgt[0][:, None] * src[idx[0]]
    for k in range(1, len(idx)):
        col = col + wgt[k][:, None] * src[idx[k]]
    image = bg.to(torch.float32).reshape(1, 1, 3).expand(V, H * W, 3).clone()
    image = image.index_put((vi, pi), col)
    face_id = torch.where(hit, key & 0xffffffff, torch.full((), -1, dtype=torch.int64)).to(torch.int32)
    return (image.permute(0, 2, 1).reshape(V, 3, H, W), hit.float().reshape(V, 1, H, W), depth.reshape(V, 1, H, W),
            face_id.reshape(V, H, W))


# ------------------------------------------------------------------------------------------------------- native path
class _RasterizeMesh(torch.autograd.Function):
    """lgm_meshraster_forward / _backward: differentiable in `param` (the texture or the colours) alone."""

    @staticmethod
    def forward(ctx, param, vertices, faces, uvs, face_uvs, cv, cvp, bg, H, W, textured):
        dev = vertices.device
        V, Nv, Nf = cv.shape[0], vertices.shape[0], faces.shape[0]
        Nu = uvs.shape[0] if textured else 0
        Ht, Wt = (param.shape[0], param.shape[1]) if textured else (0, 0)
        image = torch.empty(V, 3, H, W, dtype=torch.float32, device=dev)
        alpha = torch.empty(V, 1, H, W, dtype=torch.float32, device=dev)
        depth = torch.empty(V, 1, H, W, dtype=torch.float32, device=dev)
        face_id = torch.empty(V, H, W, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws, ws_bytes = nat.workspace("lgm_meshraster_workspace_size", dev, V, Nv, Nf, H, W, Ht, Wt)
            if ws_bytes == 0:
                raise nat.NativeError(f"lgm_meshraster: sizes V={V} Nv={Nv} Nf={Nf} H={H} W={W} texture {Ht} x {Wt} are "
                                      "out of range (every element count must stay below 2^31)")
            nat.call("lgm_meshraster_forward", dev, ptr(vertices) if Nv else None, Nv, ptr(faces) if Nf else None, Nf,
                     ptr(uvs) if textured else None, Nu, ptr(face_uvs) if textured else None,
                     ptr(param) if textured else None, Ht, Wt, None if textured else ptr(param), ptr(cv), ptr(cvp), V,
                     ptr(bg), H, W, ptr(image), ptr(alpha), ptr(depth), ptr(face_id), ptr(ws), ws_bytes)
        ctx.save_for_backward(faces, uvs, face_uvs, ws)
        ctx.dims = (V, Nv, Nf, Nu, Ht, Wt, H, W, textured, ws_bytes, tuple(param.shape))
        ctx.mark_non_differentiable(alpha, depth, face_id)
        return image, alpha, depth, face_id

    @staticmethod
    def backward(ctx, d_image, d_alpha, d_depth, d_face_id):
        faces, uvs, face_uvs, ws = ctx.saved_tensors
        V, Nv, Nf, Nu, Ht, Wt, H, W, textured, ws_bytes, shape = ctx.dims
        dev = faces.device
        d_image = d_image.float().contiguous()
        d_param = torch.empty(shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nat.call("lgm_meshraster_backward", dev, Nv, ptr(faces) if Nf else None, Nf, ptr(uvs) if textured else None,
                     Nu, ptr(face_uvs) if textured else None, Ht, Wt, V, H, W, ptr(d_image),
                     ptr(d_param) if textured else None, None if textured else ptr(d_param), ptr(ws), ws_bytes)
        return (d_param,) + (None,) * 10


# ------------------------------------------------------------------------------------------------------- public
def _cameras(cam_view, cam_view_proj, dev):
    cv, cvp = cam_view, cam_view_proj
    if cv.dim() == 4 and cv.shape[0] == 1:
        cv, cvp = cv[0], cvp[0]
    if cv.dim() != 3 or tuple(cv.shape[1:]) != (4, 4) or cv.shape != cvp.shape or cv.shape[0] < 1:
        raise ValueError(f"cam_view {tuple(cam_view.shape)}, cam_view_proj {tuple(cam_view_proj.shape)}: expected "
                         "[V, 4, 4] or [1, V, 4, 4], V >= 1")
    return (cv.detach().to(dev, torch.float32).contiguous(), cvp.detach().to(dev, torch.float32).contiguous())


def render_mesh(mesh: Mesh, cam_view: torch.Tensor, cam_view_proj: torch.Tensor, H: int, W: int, bg=None) -> dict:
    """The mesh drawn from cameras [V, 4, 4] (or [1, V, 4, 4]) as GaussianRenderer.render takes them, at H x W pixels
    (include/lgm_meshraster.h): the nearest face per pixel, both windings, no antialiasing; its colour from
    mesh.texture (bilinear, clamp to edge) through the UV atlas, or interpolated from mesh.colors when there is no
    texture; `bg` [3] (white by default, the renderer's) elsewhere. Returns {"image" [V, 3, H, W], "alpha" [V, 1, H, W]
    (1 where a face is hit), "depth" [V, 1, H, W] (view depth, 0 where none), "face_id" [V, H, W] int32 (-1 where
    none)}. The image is differentiable in mesh.texture, or in mesh.colors without a texture, and in nothing else."""
    dev = mesh.vertices.device
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"H={H}, W={W}: at least one pixel each")
    textured = mesh.texture is not None
    if textured and (mesh.uvs is None or mesh.face_uvs is None):
        raise ValueError("a mesh with a texture needs uvs and face_uvs (bake_texture makes them)")
    if not textured and mesh.colors is None:
        raise ValueError("render_mesh: the mesh has neither a texture nor colours")
    param = mesh.texture if textured else mesh.colors
    if param.device != dev or param.dtype != torch.float32:
        raise ValueError(f"texture / colours must be float32 on {dev}")
    if textured and (param.dim() != 3 or param.shape[2] != 3 or param.shape[0] < 1 or param.shape[1] < 1):
        raise ValueError(f"texture of shape {tuple(param.shape)}: expected [Ht, Wt, 3]")
    if not textured and tuple(param.shape) != (mesh.vertices.shape[0], 3):
        raise ValueError(f"colors of shape {tuple(param.shape)}: expected [{mesh.vertices.shape[0]}, 3]")
    vertices = mesh.vertices.detach().to(torch.float32).contiguous()
    faces = mesh.faces.detach().to(torch.int32).contiguous()
    uvs = mesh.uvs.detach().to(torch.float32).contiguous() if textured else None
    face_uvs = mesh.face_uvs.detach().to(torch.int32).contiguous() if textured else None
    if textured and face_uvs.shape[0] != faces.shape[0]:
        raise ValueError(f"face_uvs of {face_uvs.shape[0]} rows for {faces.shape[0]} faces")
    cv, cvp = _cameras(cam_view, cam_view_proj, dev)
    bgt = torch.ones(3) if bg is None else torch.as_tensor(bg, dtype=torch.float32)
    bgt = bgt.detach().to(dev, torch.float32).contiguous()
    param = param.contiguous()
    if dev.type == "cuda":
        out = _RasterizeMesh.apply(param, vertices, faces, uvs, face_uvs, cv, cvp, bgt, H, W, textured)
    else:
        out = _render_torch((vertices, faces, uvs, face_uvs, textured), param, cv, cvp, bgt, H, W)
    return {"image": out[0], "alpha": out[1], "depth": out[2], "face_id": out[3]}


def _render_gaussians(g, opt, cv, cvp, H, W, bg):
    """The Gaussians' clamped image [V, 3, H, W] from the same cameras, as GaussianRenderer.render draws it."""
    from .gs import rasterize, tan_half_fov
    tan = tan_half_fov(opt.fovy)
    with torch.no_grad():
        return rasterize(g[None], cv[None], cvp[None], bg, tan, tan, H, W, clamp=True)[0][0]


def fit_poses(iters: int, views: int = 1, seed: int = 0):
    """The orbit poses fit_texture draws: (elevation, azimuth) [iters, views] float64 in degrees from a seeded CPU
    generator; elevation uniform in [-80, 80] (short of the poles, where the look-at's up vector degenerates), azimuth
    in [0, 360): the whole orbit."""
    gen = torch.Generator("cpu").manual_seed(int(seed))
    r = torch.rand(int(iters), int(views), 2, generator=gen, dtype=torch.float64)
    return r[..., 0] * 160.0 - 80.0, r[..., 1] * 360.0


def fit_texture(mesh: Mesh, gaussians: torch.Tensor, opt, iters: int = 512, views: int = 1, resolution: int = 512,
                lr: float = 0.01, seed: int = 0, bg=None) -> Mesh:
    """convert.py:411-440 (fit_mesh_uv's loop): the mesh's baked texture fitted to renders of the Gaussians. Every
    iteration draws `views` poses of fit_poses(iters, views, seed) at radius opt.cam_radius, renders the Gaussians
    (without a graph) and the mesh at resolution^2 over `bg` (white by default), takes the MSE of the two images, steps
    the texture with the native AdamW (weight_decay = 0) and clamps it to [0, 1]. The texture itself is the parameter
    (the reference fits its inverse sigmoid), it starts from the mesh's texture (bake_texture's), and the poses span
    the whole orbit (the reference's: the front, +-15 degrees). A texel no pose sees keeps its value bit for bit; the
    same seed gives the same bits. Returns a new Mesh whose `fit` holds {"loss_first", "loss_last", "iters"}."""
    from .optim import AdamW
    if mesh.texture is None:
        raise ValueError("fit_texture: the mesh has no texture (bake_texture, or gaussians_to_mesh(texels=...), first)")
    g = _check_gaussians(gaussians)
    dev = mesh.vertices.device
    if g.device != dev:
        raise ValueError(f"gaussians on {g.device}, mesh on {dev}")
    iters, views, S = int(iters), int(views), int(resolution)
    if iters < 0 or views < 1 or S < 1:
        raise ValueError(f"iters={iters}, views={views}, resolution={S}: iters >= 0, views and resolution >= 1")
    if iters == 0:
        return replace(mesh, fit={"loss_first": None, "loss_last": None, "iters": 0})
    bgt = (torch.ones(3) if bg is None else torch.as_tensor(bg, dtype=torch.float32)).to(dev, torch.float32)
    tex = mesh.texture.detach().clone().contiguous().requires_grad_(True)
    optim = AdamW([tex], lr=lr, weight_decay=0.0)
    work = replace(mesh, texture=tex)
    el, az = fit_poses(iters, views, seed)
    losses = []
    for i in range(iters):
        cv, cvp, _ = orbit_cameras_batched(el[i], az[i], opt.cam_radius, opt.fovy, opt.znear, opt.zfar, device=dev)
        target = _render_gaussians(g, opt, cv, cvp, S, S, bgt)
        with torch.enable_grad():  # (callers such as an inference script run under no_grad)
            image = render_mesh(work, cv, cvp, S, S, bgt)["image"]
            loss = torch.nn.functional.mse_loss(image, target)
        optim.zero_grad(set_to_none=True)
        loss.backward()
        optim.step()
        with torch.no_grad():
            tex.clamp_(0.0, 1.0)
        if i == 0 or i == iters - 1:
            losses.append(loss.detach())
    fit = {"loss_first": float(losses[0]), "loss_last": float(losses[-1]), "iters": iters}
    return replace(mesh, texture=tex.detach(), fit=fit)


def mesh_psnr(mesh: Mesh, gaussians: torch.Tensor, opt, cam_view: torch.Tensor, cam_view_proj: torch.Tensor, H: int,
              W: int, bg=None) -> float:
    """-10 log10 of the MSE between render_mesh's image and the Gaussians' render (clamped, as GaussianRenderer.render
    returns it) from the same cameras [V, 4, 4] at H x W over `bg` (white by default)."""
    g = _check_gaussians(gaussians)
    dev = mesh.vertices.device
    cv, cvp = _cameras(cam_view, cam_view_proj, dev)
    bgt = (torch.ones(3) if bg is None else torch.as_tensor(bg, dtype=torch.float32)).to(dev, torch.float32)
    with torch.no_grad():
        image = render_mesh(mesh, cv, cvp, H, W, bgt)["image"]
        target = _render_gaussians(g.to(dev), opt, cv, cvp, int(H), int(W), bgt)
        mse = float(torch.nn.functional.mse_loss(image, target))
    return math.inf if mse == 0 else -10.0 * math.log10(mse)
