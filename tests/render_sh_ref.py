"""Dense torch restatement of the splat render with spherical-harmonics colour -- TEST INFRASTRUCTURE ONLY.

Written from the specification (include/lgm_render.h LGM_RENDER_SH_MASK) with its own statement of the basis; it
shares no code with lgm_amd/sh.py, lgm_amd/cpu.py or the kernels. Per view the colour of every Gaussian is evaluated
in the dtype asked for, put in place of columns 11:14 of a 14-wide row, and the row is handed to
tests/render_aa_ref.render_view, which takes the discrete decisions from an fp32 evaluation and knows the antialias
switch. Autograd gives the gradients (fp64: the truth; fp32: the error a faithful fp32 implementation has).
"""
from __future__ import annotations

import numpy as np
import torch

from tests import render_aa_ref as R

K0 = 0.28209479177387814
K1 = 0.4886025119029199
K2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
K3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)


def basis(dirs):
    """All 16 functions at unit vectors dirs [.., 3] -> [.., 16] (a degree-d colour uses the first (d + 1)^2)."""
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, K0),
        -K1 * y, K1 * z, -K1 * x,
        K2[0] * x * y, K2[1] * y * z, K2[2] * (2 * zz - xx - yy), K2[3] * x * z, K2[4] * (xx - yy),
        K3[0] * y * (3 * xx - yy), K3[1] * x * y * z, K3[2] * y * (4 * zz - xx - yy),
        K3[3] * z * (2 * zz - 3 * xx - 3 * yy), K3[4] * x * (4 * zz - xx - yy), K3[5] * z * (xx - yy),
        K3[6] * x * (xx - 3 * yy)], dim=-1)


def degree_of_width(width):
    return {14: 0, 23: 1, 38: 2, 59: 3}[width]


def campos(view):
    """-t M^-1 of a [4,4] view matrix in the row-vector convention, the inverse in fp64; in view's dtype."""
    v = view.detach().double()
    return (-(v[3:4, :3] @ torch.linalg.inv(v[:3, :3]))[0]).to(view.dtype)


def view_colours(g, view):
    """g [N, 11 + 3K] -> (colour [N,3], unclamped [N,3]) of this view."""
    d = degree_of_width(g.shape[-1])
    K = (d + 1) ** 2
    v = g[:, 0:3] - campos(view)
    dirs = v / v.norm(dim=-1, keepdim=True)
    sh = g[:, 11:].reshape(-1, K, 3)
    raw = (basis(dirs)[:, :K, None] * sh).sum(1) + 0.5
    return raw.clamp(min=0), raw


def view_rows(g, view):
    """The 14-wide rows of one view: columns 0:11 and the view's colours."""
    if g.shape[-1] == 14:
        return g, None
    col, raw = view_colours(g, view)
    return torch.cat([g[:, :11], col], dim=-1), raw


def render(gaussians, cam_view, cam_view_proj, tan, H, W, bg, scale_modifier=1.0, dtype=torch.float64,
           antialias=False, d_image=None, d_depth=None, d_alpha=None, clamp=False):
    """[B,N,14 or 11 + 3K], [B,V,4,4] x 2 -> numpy dict: image [B,V,3,H,W] (clamped to [0, 1] if clamp), depth, alpha
    [B,V,1,H,W]; vis [B,V,N] (bool); for SH rows raw [B,V,N,3], the unclamped colours; with any d_* given also
    d_gaussians, the gradient of sum(image d_image) + sum(depth d_depth) + sum(alpha d_alpha)."""
    as_t = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=dtype)  # noqa: E731
    g = as_t(gaussians).clone()
    cv, cvp, bgt = as_t(cam_view), as_t(cam_view_proj), as_t(bg).reshape(3)
    want = any(d is not None for d in (d_image, d_depth, d_alpha))
    g.requires_grad_(want)
    B, V = cv.shape[0], cv.shape[1]
    outs, raws = [], []
    for b in range(B):
        row, rraw = [], []
        for v in range(V):
            g14, raw = view_rows(g[b], cv[b, v])
            row.append(R.render_view(g14, cv[b, v], cvp[b, v], tan, tan, H, W, bgt, scale_modifier, antialias))
            rraw.append(raw)
        outs.append(row)
        raws.append(rraw)
    stack = lambda i: torch.stack([torch.stack([o[i] for o in row]) for row in outs])  # noqa: E731
    image, depth, alpha = stack(0), stack(1), stack(2)
    if clamp:
        image = image.clamp(0, 1)
    res = {"image": image.detach().numpy(), "depth": depth.detach().numpy(), "alpha": alpha.detach().numpy(),
           "vis": torch.stack([torch.stack([o[3]["vis"] for o in row]) for row in outs]).numpy()}
    if raws[0][0] is not None:
        res["raw"] = torch.stack([torch.stack(r) for r in raws]).detach().numpy()
    if want:
        loss = 0
        for out, d in ((image, d_image), (depth, d_depth), (alpha, d_alpha)):
            if d is not None:
                loss = loss + (out * as_t(d)).sum()
        loss.backward()
        res["d_gaussians"] = g.grad.numpy()
    return res


REST_SIGMA = 0.6  # std of the drawn rest coefficients: sum_{k>=1} Y_k^2 = (K - 1) / (4 pi), so the view-dependent part
                  # of a colour has std 0.29 / 0.48 / 0.66 at degree 1 / 2 / 3 around an RGB uniform in (0, 1)


def lift(g14, degree, seed=21, sigma=REST_SIGMA):
    """[B,N,14] RGB rows -> [B,N,11 + 3K] SH rows: DC = (rgb - 1/2) / K0, rest ~ N(0, sigma^2) (sigma = 0: zero)."""
    K = (degree + 1) ** 2
    gen = torch.Generator().manual_seed(seed)
    rest = sigma * torch.randn(g14.shape[0], g14.shape[1], 3 * (K - 1), generator=gen, dtype=torch.float32)
    return torch.cat([g14[..., :11], (g14[..., 11:14] - 0.5) / K0, rest.to(g14.dtype)], dim=-1)


def clamped_fraction(res):
    """Share of the visible (view, Gaussian, channel) colours of a render() result that the clamp holds at 0."""
    raw = res["raw"][res["vis"]]
    return float((raw <= 0).mean())
