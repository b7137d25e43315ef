"""Dense torch restatement of the splat render with the antialias switch -- TEST INFRASTRUCTURE ONLY.

The frozen oracle (oracle/raster_oracle.c) has no opacity compensation, so the antialias tests need a reference of
their own. This one is written from the specification (SURVEY.md §2.3 and include/lgm_render.h
LGM_RENDER_ANTIALIAS) and shares no code with lgm_amd/cpu.py or the oracle: every (Gaussian, pixel) pair of a view
is evaluated densely -- no tiles lists, no chunks -- in the dtype asked for (fp64: the truth; fp32: the error a
faithful fp32 implementation has, which sets the gradient bar), and autograd gives the gradients.

Per view: preprocess (near cull 0.2, EWA covariance with the 1.3 tan-fov clamp, 0.3 dilation, radius
ceil(3 sqrt(lambda_max)), 16-pixel tile rect), depth order (fp32 depth, ties by id), then per pixel front-to-back
compositing of the Gaussians whose tile rect holds the pixel: alpha = min(0.99, o G), skipped when the exponent is
positive or alpha < 1/255, stopped before the first entry that would bring T under 1e-4. The discrete decisions that
upstream takes in fp32 (visibility, radius, rect, order) are taken from an fp32 evaluation whatever the dtype, as
oracle/raster_autograd.py takes them from the fp32 oracle; the per-pixel skip / stop tests run in the dtype.
Gradient conventions are upstream's: the 0.99 cap passes the gradient of o G, a clamped t.x / t.z (t.y / t.z)
carries none and an unclamped one passes it to the view-space x (y) only, and the conic's gradient reaches the 2D
covariance through 1 / (det^2 + 1e-7) in place of 1 / det^2 (upstream's guarded inverse; the antialias factor's own
gradient is the exact derivative). The algorithm's constants are upstream's fp32 literals (0.3f is not 0.3), in
either dtype, as in the oracle's fp64 build.
"""
from __future__ import annotations

import numpy as np
import torch

TILE = 16
_f = lambda x: float(np.float32(x))  # noqa: E731  (an fp32 literal's value)
DILATION, FOV_CLAMP, NEAR, W_EPS, DET_EPS = _f(0.3), _f(1.3), _f(0.2), _f(1e-7), _f(1e-7)
ALPHA_CAP, ALPHA_MIN, T_MIN, LAMBDA_MIN = _f(0.99), _f(_f(1.0) / _f(255.0)), _f(1e-4), _f(0.1)
AA_FLOOR = _f(2.5e-5)


class _ScaleGrad(torch.autograd.Function):
    """x in the forward; the gradient times k in the backward."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.save_for_backward(k)
        return x.clone()

    @staticmethod
    def backward(ctx, d):
        return d * ctx.saved_tensors[0], None


def aa_factor(a0, b, c0):
    """s = sqrt(min(1, fmaxf(2.5e-5, det0 / det))) of the undilated 2D covariance (a0, b, c0); NaN -> the floor."""
    det0 = a0 * c0 - b * b
    det = (a0 + DILATION) * (c0 + DILATION) - b * b
    r = det0 / det
    r = torch.where(r > AA_FLOOR, r, torch.full_like(r, AA_FLOOR))
    return torch.sqrt(torch.where(r < 1.0, r, torch.ones_like(r)))


def _project(g, view, proj, tanx, tany, H, W, mod):
    """Continuous per-Gaussian quantities of one view in g's dtype."""
    N = g.shape[0]
    ph = torch.cat([g[:, 0:3], torch.ones(N, 1, dtype=g.dtype)], 1)
    hom = ph @ proj  # row vector times the row-major matrix: the column-major read of core/gs.py:54-55
    t = (ph @ view)[:, :3]
    inv_w = 1.0 / (hom[:, 3] + W_EPS)
    px = ((hom[:, 0] * inv_w + 1.0) * W - 1.0) * 0.5
    py = ((hom[:, 1] * inv_w + 1.0) * H - 1.0) * 0.5
    tz = t[:, 2]
    limx, limy = FOV_CLAMP * tanx, FOV_CLAMP * tany
    rx, ry = t[:, 0] / tz, t[:, 1] / tz
    vx, vy = (rx.clamp(-limx, limx) * tz).detach(), (ry.clamp(-limy, limy) * tz).detach()
    outx, outy = (rx < -limx) | (rx > limx), (ry < -limy) | (ry > limy)
    tx = torch.where(outx, vx, t[:, 0] - t[:, 0].detach() + vx)  # value vx; gradient to t.x only where unclamped
    ty = torch.where(outy, vy, t[:, 1] - t[:, 1].detach() + vy)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    z = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, z, -fx * tx / (tz * tz)], 1),
                     torch.stack([z, fy / tz, -fy * ty / (tz * tz)], 1)], 1)  # [N,2,3]
    A = J @ view[:3, :3].T
    r, x, y, zq = g[:, 7], g[:, 8], g[:, 9], g[:, 10]  # un-normalised quaternion, as upstream
    R = torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - r * zq), 2 * (x * zq + r * y),
                     2 * (x * y + r * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - r * x),
                     2 * (x * zq - r * y), 2 * (y * zq + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(N, 3, 3)
    S2 = torch.diag_embed((mod * g[:, 4:7]) ** 2)
    cov = A @ (R @ S2 @ R.transpose(1, 2)) @ A.transpose(1, 2)
    a0, b, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    a, c = a0 + DILATION, c0 + DILATION
    det = a * c - b * b
    return {"px": px, "py": py, "depth": tz, "a0": a0, "b": b, "c0": c0, "a": a, "c": c, "det": det}


def _discrete(q, H, W):
    """Visibility, radius, tile rect and depth order from an (fp32) projection."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    mid = 0.5 * (q["a"] + q["c"])
    lam = mid + torch.sqrt(torch.clamp(mid * mid - q["det"], min=LAMBDA_MIN))
    rad = torch.ceil(3.0 * torch.sqrt(lam))
    px, py = q["px"], q["py"]
    x0 = torch.trunc((px - rad) / TILE).clamp(0, gx)
    y0 = torch.trunc((py - rad) / TILE).clamp(0, gy)
    x1 = torch.trunc((px + rad + (TILE - 1)) / TILE).clamp(0, gx)
    y1 = torch.trunc((py + rad + (TILE - 1)) / TILE).clamp(0, gy)
    vis = (q["depth"] > NEAR) & (q["det"] != 0) & ((x1 - x0) * (y1 - y0) > 0)
    order = torch.sort(q["depth"], stable=True).indices
    return {"vis": vis, "rect": (x0, y0, x1, y1), "order": order, "radius": torch.where(vis, rad, torch.zeros_like(rad))}


def render_view(g, view, proj, tanx, tany, H, W, bg, mod=1.0, antialias=False):
    """g [N,14] (fp64 or fp32, requires_grad ok); view / proj [4,4] of that dtype -> (image [3,H,W], depth [1,H,W],
    alpha [1,H,W], info) with info = the view's visibility mask, antialias factor s, compensated opacity and the
    condition a0 c0 / det0 of the undilated determinant (how far rounding of a0, b, c0 is amplified in the factor)."""
    dt = g.dtype
    q = _project(g, view, proj, tanx, tany, H, W, mod)
    with torch.no_grad():
        g32 = g.detach().float()
        q32 = q if dt == torch.float32 else _project(g32, view.float(), proj.float(), tanx, tany, H, W, mod)
        dsc = _discrete({k: v.detach() for k, v in q32.items()}, H, W)
    s = aa_factor(q["a0"], q["b"], q["c0"]) if antialias else torch.ones_like(q["det"])
    opac = g[:, 3] * s if antialias else g[:, 3]
    order, vis = dsc["order"], dsc["vis"]
    det = torch.where(q["det"] == 0, torch.ones_like(q["det"]), q["det"]).detach()
    k = det * det / (det * det + DET_EPS)  # upstream's guarded 1 / det^2 in the conic's backward
    a, b, c = (_ScaleGrad.apply(q[n], k) for n in ("a", "b", "c"))
    dc = a * c - b * b
    dc = torch.where(dc == 0, torch.ones_like(dc), dc)
    cA, cB, cC = c / dc, -b / dc, a / dc
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pxs, pys = xs.reshape(-1), ys.reshape(-1)
    x0, y0, x1, y1 = (r[order].to(torch.int64)[:, None] for r in dsc["rect"])
    txs, tys = (pxs // TILE)[None, :], (pys // TILE)[None, :]
    in_rect = vis[order][:, None] & (txs >= x0) & (txs < x1) & (tys >= y0) & (tys < y1)
    dx = q["px"][order][:, None] - pxs.to(dt)[None, :]
    dy = q["py"][order][:, None] - pys.to(dt)[None, :]
    power = -0.5 * (cA[order][:, None] * dx * dx + cC[order][:, None] * dy * dy) - cB[order][:, None] * dx * dy
    og = opac[order][:, None] * torch.exp(power)
    alpha = og + (og.clamp(max=ALPHA_CAP) - og).detach()  # the cap's value, the gradient of o G (upstream's backward)
    with torch.no_grad():
        valid = in_rect & (power <= 0) & (alpha >= ALPHA_MIN)
    one_minus = torch.where(valid, 1 - alpha, torch.ones_like(alpha))
    T_after = torch.cumprod(one_minus, 0)
    T_before = torch.cat([torch.ones_like(T_after[:1]), T_after[:-1]], 0)
    with torch.no_grad():
        stopped = torch.cumsum((valid & (T_after < T_MIN)).to(torch.int32), 0) > 0  # at or behind the first stop
        keep = valid & ~stopped
    wgt = torch.where(keep, alpha * T_before, torch.zeros_like(alpha))
    col = (g[:, 11:14][order].T[:, :, None] * wgt[None]).sum(1)
    dep = (q["depth"][order][:, None] * wgt).sum(0)
    T_fin = torch.where(keep, 1 - alpha, torch.ones_like(alpha)).prod(0)
    img = col + T_fin[None, :] * bg[:, None]
    det0 = (q["a0"] * q["c0"] - q["b"] * q["b"]).detach()
    cond = torch.where(det0 > 0, (q["a0"] * q["c0"]).detach() / det0, torch.full_like(det0, float("inf")))
    info = {"vis": vis, "s": s.detach(), "opacity": opac.detach(), "radius": dsc["radius"], "cond": cond}
    return img.reshape(3, H, W), dep.reshape(1, H, W), (1 - T_fin).reshape(1, H, W), info


def render(gaussians, cam_view, cam_view_proj, tan, H, W, bg, scale_modifier=1.0, dtype=torch.float64,
           antialias=False, d_image=None, d_depth=None, d_alpha=None):
    """[B,N,14], [B,V,4,4] x 2 (tensors or arrays) -> numpy dict: image [B,V,3,H,W], depth, alpha [B,V,1,H,W]; vis
    (bool), s, opacity (the factor and o s, the opacity the compositing consumes), cond (a0 c0 / det0) [B,V,N]; with any d_* given also
    d_gaussians [B,N,14], the gradient of sum(image d_image) + sum(depth d_depth) + sum(alpha d_alpha)."""
    as_t = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=dtype)  # noqa: E731
    g = as_t(gaussians).clone()
    cv, cvp, bgt = as_t(cam_view), as_t(cam_view_proj), as_t(bg).reshape(3)
    want = any(d is not None for d in (d_image, d_depth, d_alpha))
    g.requires_grad_(want)
    B, V = cv.shape[0], cv.shape[1]
    outs = [[render_view(g[b], cv[b, v], cvp[b, v], tan, tan, H, W, bgt, scale_modifier, antialias)
             for v in range(V)] for b in range(B)]
    stack = lambda i: torch.stack([torch.stack([o[i] for o in row]) for row in outs])  # noqa: E731
    image, depth, alpha = stack(0), stack(1), stack(2)
    res = {"image": image.detach().numpy(), "depth": depth.detach().numpy(), "alpha": alpha.detach().numpy()}
    for k in ("vis", "s", "opacity", "cond"):
        res[k] = torch.stack([torch.stack([o[3][k] for o in row]) for row in outs]).numpy()
    if want:
        loss = 0
        for out, d in ((image, d_image), (depth, d_depth), (alpha, d_alpha)):
            if d is not None:
                loss = loss + (out * as_t(d)).sum()
        loss.backward()
        res["d_gaussians"] = g.grad.numpy()
    return res
