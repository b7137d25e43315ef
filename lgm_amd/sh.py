"""Spherical-harmonics colour (include/lgm_render.h, LGM_RENDER_SH_MASK) in torch: the 3DGS rasteriser's real basis,
the row layout [.., 11 + 3K] (coefficient k of channel c at column 11 + 3k + c, DC first) and the helpers that move
between it and the plain [.., 14] RGB rows. The CPU render path evaluates colours with eval_sh; the GPU path has its
own kernels (lgm_amd/csrc/render_sh.hip)."""
from __future__ import annotations

import torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)

WIDTHS = {14: 0, 23: 1, 38: 2, 59: 3}  # row width -> degree (14: plain RGB)


def num_coeffs(degree: int) -> int:
    return (degree + 1) ** 2


def row_width(degree: int) -> int:
    """Width of a Gaussian row at `degree` (0: the plain 14-wide RGB row)."""
    if degree not in (0, 1, 2, 3):
        raise ValueError(f"sh_degree must be 0..3, got {degree}")
    return 14 if degree == 0 else 11 + 3 * num_coeffs(degree)


def degree_of(width: int, sh_degree=None) -> int:
    """The SH degree of rows of `width` columns: inferred (14 -> 0, 23 / 38 / 59 -> 1 / 2 / 3), or checked against an
    explicit sh_degree. ValueError for any other width or a contradiction."""
    if width not in WIDTHS:
        raise ValueError(f"gaussians must be [B,N,14] (RGB) or [B,N,23 / 38 / 59] (SH degree 1 / 2 / 3), got width {width}")
    if sh_degree is not None and int(sh_degree) != WIDTHS[width]:
        row_width(int(sh_degree))  # (an out-of-range degree says so)
        raise ValueError(f"sh_degree={sh_degree} needs rows of {row_width(int(sh_degree))} columns, got {width}")
    return WIDTHS[width]


def basis(degree: int, dirs: torch.Tensor) -> torch.Tensor:
    """Y_0 .. Y_{K-1} at unit vectors dirs [.., 3] -> [.., K]."""
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    Y = [torch.full_like(x, C0)]
    if degree > 0:
        Y += [-C1 * y, C1 * z, -C1 * x]
    if degree > 1:
        xx, yy, zz = x * x, y * y, z * z
        Y += [C2[0] * (x * y), C2[1] * (y * z), C2[2] * (2 * zz - xx - yy), C2[3] * (x * z), C2[4] * (xx - yy)]
    if degree > 2:
        Y += [C3[0] * y * (3 * xx - yy), C3[1] * (x * y) * z, C3[2] * y * (4 * zz - xx - yy),
              C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
              C3[6] * x * (xx - 3 * yy)]
    return torch.stack(Y, dim=-1)


def eval_sh(degree: int, sh: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """Colour max(0, 1/2 + sum_k Y_k(dirs) sh[.., k, :]) for sh [.., K, 3] and unit dirs [.., 3] -> [.., 3].
    Differentiable (the clamp passes gradient where the unclamped colour is positive, as upstream's `clamped`)."""
    K = num_coeffs(degree)
    if sh.shape[-2] != K or sh.shape[-1] != 3:
        raise ValueError(f"sh must be [.., {K}, 3] at degree {degree}, got {tuple(sh.shape)}")
    return torch.clamp_min((basis(degree, dirs).unsqueeze(-1) * sh).sum(-2) + 0.5, 0.0)


def cam_positions(cam_view: torch.Tensor) -> torch.Tensor:
    """The point each view matrix [.., 4, 4] (row-vector convention) sends to the origin: -t M^-1, inverse in fp64."""
    cv = cam_view.detach().double()
    return -(cv[..., 3:4, :3] @ torch.linalg.inv(cv[..., :3, :3])).squeeze(-2)


def rgb_to_sh(g14: torch.Tensor, degree: int) -> torch.Tensor:
    """[.., 14] RGB rows -> [.., 11 + 3K]: DC = (rgb - 1/2) / C0, the rest zero (renders as the plain rows do)."""
    if g14.shape[-1] != 14:
        raise ValueError(f"rgb_to_sh takes [.., 14] rows, got width {g14.shape[-1]}")
    if degree == 0:
        return g14
    rest = g14.new_zeros(g14.shape[:-1] + (3 * (num_coeffs(degree) - 1),))
    return torch.cat([g14[..., :11], (g14[..., 11:14] - 0.5) / C0, rest], dim=-1)


def sh_to_rgb(g: torch.Tensor) -> torch.Tensor:
    """[.., 11 + 3K] (or [.., 14], returned as is) -> [.., 14] with the DC colour C0 dc + 1/2: the view-independent
    rows the mesh functions accept."""
    if degree_of(g.shape[-1]) == 0:
        return g
    return torch.cat([g[..., :11], C0 * g[..., 11:14] + 0.5], dim=-1)
