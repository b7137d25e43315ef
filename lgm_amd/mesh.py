"""Mesh export: Gaussians to a coloured triangle mesh (include/lgm_mesh.h), the step convert.py takes in the
reference. The reference fits a NeRF to renders of the Gaussians and runs marching cubes on its density; here the
Gaussians are the density field: they are sampled on convert.py's [-bound, bound]^3 grid (convert.py:263-289), the
iso-surface is extracted by naive surface nets and coloured from the Gaussians. Nothing is fitted and
nothing is random: two calls on the same input give the same bits.

  density_grid       Gaussians [N, 14] -> sigma [Gx, Gy, Gz], rgb [Gx, Gy, Gz, 3]
  extract_surface    sigma (and rgb) -> Mesh
  gaussians_to_mesh  both, after save_ply's opacity prune
  Mesh               vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None; save_obj, save_ply

GPU tensors run the kernels of lgm_amd/csrc/mesh.hip (a missing library raises NativeError); CPU tensors take the
vectorised torch forms of the same formulas below. `resolution = 256` is convert.py's grid size; `iso = 0.5` is a
choice, not a tuned value: no checkpoint exists offline, so neither default has been measured on a trained model.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as nat
from ._native import ptr
from .ply import write_mesh_ply

CUTOFF = 1e-4  # include/lgm_mesh.h LGM_MESH_CUTOFF
# the 12 edges of a cell in include/lgm_mesh.h's order: (lower corner, axis); corner c = 4 di + 2 dj + dk
_EDGES = ((0, 2), (0, 1), (0, 0), (1, 1), (1, 0), (2, 2), (2, 0), (3, 0), (4, 2), (4, 1), (5, 1), (6, 2))


def grid_params(resolution: Union[int, Sequence[int]], bound: float = 1.0):
    """(G, lo, h): the node counts and the fp32 origin and spacing of the grid over [-bound, bound]^3 whose node
    (i, j, k) sits at lo + (i, j, k) h (the linspace of convert.py:268-270)."""
    G = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(r) for r in resolution)
    if len(G) != 3 or min(G) < 3:
        raise ValueError(f"resolution {resolution}: an int or three ints, each >= 3")
    if G[0] * G[1] * G[2] >= 2 ** 31:
        raise ValueError(f"resolution {G}: {G[0] * G[1] * G[2]} nodes, the kernels index a grid with 31 bits")
    if not (bound > 0 and np.isfinite(bound)):
        raise ValueError(f"bound {bound} must be positive and finite")
    lo = np.full(3, -float(bound), np.float32)
    h = np.asarray([2.0 * float(bound) / (n - 1) for n in G], np.float64).astype(np.float32)
    return G, lo, h


def _c3(a: np.ndarray):
    return (ctypes.c_float * 3)(*[float(v) for v in a])


@dataclass
class Mesh:
    """A triangle mesh with per-vertex colours (tensors on the device that made them). Faces are wound so that
    normals point out of the dense side."""
    vertices: torch.Tensor
    faces: torch.Tensor
    colors: Optional[torch.Tensor] = None

    def _numpy(self):
        v = self.vertices.detach().cpu().numpy().astype(np.float32)
        f = self.faces.detach().cpu().numpy().astype(np.int32)
        c = None if self.colors is None else self.colors.detach().cpu().numpy().astype(np.float32)
        return v, f, c

    def save_obj(self, path: str) -> None:
        """Wavefront OBJ: `v x y z r g b` (the common vertex-colour extension; plain `v x y z` without colours) and
        1-based `f a b c` lines."""
        v, f, c = self._numpy()
        rows = v if c is None else np.concatenate([v, np.clip(c, 0.0, 1.0)], axis=1)
        with open(path, "w") as out:
            out.write(f"# {len(v)} vertices, {len(f)} faces\n")
            out.write("".join("v " + " ".join(repr(float(x)) for x in row) + "\n" for row in rows))
            out.write("".join(f"f {a + 1} {b + 1} {c_ + 1}\n" for a, b, c_ in f.tolist()))

    def save_ply(self, path: str) -> None:
        """Binary little-endian PLY: float x y z (and uchar red green blue), faces as `list uchar int vertex_indices`."""
        v, f, c = self._numpy()
        write_mesh_ply(path, v, f, c)


# ------------------------------------------------------------------------------------------------------- density
def _check_gaussians(g: torch.Tensor) -> torch.Tensor:
    if g.dim() == 3 and g.shape[0] == 1:
        g = g[0]
    if g.dim() != 2 or g.shape[1] != 14:
        raise ValueError(f"gaussians of shape {tuple(g.shape)}: expected [N, 14] (or [1, N, 14])")
    return g.detach().to(torch.float32).contiguous()


def _density_native(g, G, lo, h, scale_modifier, cutoff, sigma, rgb):
    dev = g.device
    N = g.shape[0]
    lo_c, h_c = _c3(lo), _c3(h)
    with torch.cuda.device(dev):
        # (these entry points are told the allocated size: ws.numel(), at least 1)
        ws0, _ = nat.workspace("lgm_mesh_density_workspace_size", dev, N, *G, 0)
        npairs = torch.zeros(1, dtype=torch.int64, device=dev)
        nat.call("lgm_mesh_density_count", dev, ptr(g) if N else None, N, float(scale_modifier), *G, lo_c, h_c,
                 float(cutoff), ptr(ws0), ws0.numel(), ptr(npairs))
        cap = int(npairs.item())  # the lists' length is data dependent: the one host sync of the density pass
        if cap >= 2 ** 31:
            raise nat.NativeError(f"lgm_mesh_density: {cap} (Gaussian, brick) pairs, the lists are indexed with 31 bits; "
                                  "raise the cutoff or lower the resolution")
        del ws0
        ws, _ = nat.workspace("lgm_mesh_density_workspace_size", dev, N, *G, cap)
        nat.call("lgm_mesh_density", dev, ptr(g) if N else None, N, float(scale_modifier), *G, lo_c, h_c, float(cutoff),
                 cap, ptr(sigma), ptr(rgb), ptr(ws), ws.numel())


def _density_torch(g, G, lo, h, scale_modifier, cutoff, sigma, rgb):
    """include/lgm_mesh.h's density formulas in fp64, vectorised: slabs of nodes along x against the Gaussians whose
    box reaches the slab."""
    g = g.double()
    fin = torch.isfinite(g).all(dim=1)
    o, s, q = g[:, 3], g[:, 4:7] * float(scale_modifier), g[:, 7:11]
    qn = q.norm(dim=1)
    keep = fin & (o > cutoff) & (s > 0).all(dim=1) & (qn > 0)
    g, o, s, q = g[keep], o[keep], s[keep], q[keep] / qn[keep, None]
    sigma.zero_()
    if rgb is not None:
        rgb.zero_()
    if g.shape[0] == 0:
        return
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    A = R.transpose(1, 2) / s[:, :, None]  # diag(s)^-1 R^T
    rho2 = 2.0 * torch.log(o / cutoff)
    ext_x = torch.sqrt(rho2 * ((R[:, 0, :] * s) ** 2).sum(dim=1)) * (1 + 1e-9) + 1e-12
    mu, c = g[:, 0:3], g[:, 11:14]
    ax = [float(lo[a]) + torch.arange(G[a], dtype=torch.float64) * float(h[a]) for a in range(3)]
    slab = max(1, (1 << 16) // (G[1] * G[2]))
    for i0 in range(0, G[0], slab):
        xs = ax[0][i0:i0 + slab]
        near = ((mu[:, 0] + ext_x >= xs[0]) & (mu[:, 0] - ext_x <= xs[-1])).nonzero().squeeze(1)
        if near.numel() == 0:
            continue
        X = torch.stack(torch.meshgrid(xs, ax[1], ax[2], indexing="ij"), dim=-1).reshape(-1, 3)
        sw = torch.zeros(X.shape[0], dtype=torch.float64)
        swc = torch.zeros(X.shape[0], 3, dtype=torch.float64)
        for n0 in range(0, near.numel(), 256):
            idx = near[n0:n0 + 256]
            yv = torch.einsum("nka,pna->pnk", A[idx], X[:, None, :] - mu[idx][None])
            d2 = (yv * yv).sum(dim=2)
            w = torch.where(d2 <= rho2[idx][None], o[idx][None] * torch.exp(-0.5 * d2), torch.zeros((), dtype=d2.dtype))
            sw += w.sum(dim=1)
            swc += w @ c[idx]
        sigma[i0:i0 + slab] = sw.reshape(len(xs), G[1], G[2]).float()
        if rgb is not None:
            col = torch.where(sw[:, None] > 0, swc / sw.clamp_min(1e-300)[:, None], torch.zeros((), dtype=sw.dtype))
            rgb[i0:i0 + slab] = col.reshape(len(xs), G[1], G[2], 3).float()


def density_grid(gaussians: torch.Tensor, resolution: Union[int, Sequence[int]] = 256, bound: float = 1.0,
                 scale_modifier: float = 1.0, cutoff: float = CUTOFF, *, colors: bool = True,
                 out: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None):
    """The Gaussians' density and colour on the grid of `resolution` nodes (an int or three) over [-bound, bound]^3
    (include/lgm_mesh.h, density pass): sigma = sum o exp(-d2 / 2), rgb = the sigma-weighted mean colour, each
    Gaussian cut where its term falls below `cutoff`. Returns (sigma [Gx, Gy, Gz], rgb [Gx, Gy, Gz, 3]) float32 on the
    Gaussians' device, rgb None with colors=False. out: (sigma, rgb) buffers to fill instead of new ones."""
    g = _check_gaussians(gaussians)
    G, lo, h = grid_params(resolution, bound)
    if not (cutoff > 0 and np.isfinite(cutoff)) or not np.isfinite(scale_modifier):
        raise ValueError(f"cutoff {cutoff} must be positive and finite, scale_modifier {scale_modifier} finite")
    if out is not None:
        sigma, rgb = out
        for t, shape in ((sigma, G), (rgb, G + (3,))):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != g.device
                                  or not t.is_contiguous()):
                raise ValueError(f"out: expected contiguous float32 {shape} on {g.device}")
    else:
        sigma = torch.empty(G, dtype=torch.float32, device=g.device)
        rgb = torch.empty(G + (3,), dtype=torch.float32, device=g.device) if colors else None
    (_density_native if g.is_cuda else _density_torch)(g, G, lo, h, scale_modifier, cutoff, sigma, rgb)
    return sigma, rgb


# ------------------------------------------------------------------------------------------------------- extraction
def _extract_native(sigma, rgb, iso, G, lo, h) -> Mesh:
    dev = sigma.device
    with torch.cuda.device(dev):
        ws, _ = nat.workspace("lgm_mesh_extract_workspace_size", dev, *G)  # (passed as ws.numel(), as above)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        nat.call("lgm_mesh_count", dev, ptr(sigma), *G, float(iso), ptr(ws), ws.numel(), ptr(counts))
        nv, nf = counts.tolist()  # the one host sync: the outputs' sizes
        vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        colors = torch.empty(nv, 3, dtype=torch.float32, device=dev) if rgb is not None else None
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        nat.call("lgm_mesh_emit", dev, ptr(sigma), ptr(rgb), *G, _c3(lo), _c3(h), float(iso), ptr(ws), ws.numel(), nv,
                 nf, ptr(vertices), ptr(colors), ptr(faces), nv, nf)
    return Mesh(vertices, faces, colors)


def _extract_torch(sigma, rgb, iso, G, lo, h) -> Mesh:
    """include/lgm_mesh.h's surface nets in fp32 torch operations, each rounded on its own, in the header's order."""
    iso = torch.tensor(float(iso), dtype=torch.float32)
    s = torch.where(torch.isfinite(sigma), sigma, torch.zeros((), dtype=torch.float32)).clone()
    s[0] = s[-1] = 0
    s[:, 0] = s[:, -1] = 0
    s[:, :, 0] = s[:, :, -1] = 0
    ins = s >= iso
    C = (G[0] - 1, G[1] - 1, G[2] - 1)
    m = sum(ins[(c >> 2):(c >> 2) + C[0], ((c >> 1) & 1):((c >> 1) & 1) + C[1], (c & 1):(c & 1) + C[2]].int()
            for c in range(8))
    active = ((m != 0) & (m != 8)).reshape(-1)
    vid = torch.cumsum(active.long(), 0) - 1
    cell = active.nonzero().squeeze(1)
    nv = cell.numel()
    ck = cell % C[2]
    cj = (cell // C[2]) % C[1]
    ci = cell // (C[2] * C[1])
    node = [((ci + (c >> 2)) * G[1] + cj + ((c >> 1) & 1)) * G[2] + ck + (c & 1) for c in range(8)]
    sf = s.reshape(-1)
    sc = [sf[n] for n in node]
    zero = torch.zeros((), dtype=torch.float32)
    p = [torch.zeros(nv, dtype=torch.float32) for _ in range(3)]
    col = torch.zeros(nv, 3, dtype=torch.float32)
    cnt = torch.zeros(nv, dtype=torch.float32)
    rf = None if rgb is None else rgb.reshape(-1, 3)
    for a, axis in _EDGES:
        b = a + (4 >> axis)
        ia, ib = sc[a] >= iso, sc[b] >= iso
        cross = ia != ib
        t = (iso - sc[a]) / torch.where(cross, sc[b] - sc[a], torch.ones((), dtype=torch.float32))
        off = [torch.full((nv,), float(a >> 2)), torch.full((nv,), float((a >> 1) & 1)), torch.full((nv,), float(a & 1))]
        off[axis] = t
        for d in range(3):
            p[d] = p[d] + torch.where(cross, off[d], zero)
        if rf is not None:
            col = col + torch.where(cross[:, None], rf[torch.where(ia, node[a], node[b])], zero)
        cnt = cnt + cross.float()
    lo_t, h_t = torch.from_numpy(np.asarray(lo, np.float32)), torch.from_numpy(np.asarray(h, np.float32))
    P = torch.stack([ci.float() + p[0] / cnt, cj.float() + p[1] / cnt, ck.float() + p[2] / cnt], dim=1)
    vertices = lo_t[None] + P * h_t[None]
    colors = None if rf is None else col / cnt[:, None]
    # faces: (node, axis) pairs in ascending order
    cross = torch.zeros(G + (3,), dtype=torch.bool)
    cross[:-1, :, :, 0] = ins[:-1] != ins[1:]
    cross[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    cross[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    hit = cross.reshape(-1).nonzero().squeeze(1)
    a = hit % 3
    n = hit // 3
    nn = torch.stack([n // (G[2] * G[1]), (n // G[2]) % G[1], n % G[2]], dim=1)
    eb = torch.nn.functional.one_hot((a + 1) % 3, 3)
    ec = torch.nn.functional.one_hot((a + 2) % 3, 3)

    def vertex_of(c):
        return vid[(c[:, 0] * C[1] + c[:, 1]) * C[2] + c[:, 2]]

    q0, q1, q2, q3 = vertex_of(nn - eb - ec), vertex_of(nn - ec), vertex_of(nn), vertex_of(nn - eb)
    in0 = ins.reshape(-1)[n]
    t1 = torch.where(in0[:, None], torch.stack([q0, q1, q2], 1), torch.stack([q0, q2, q1], 1))
    t2 = torch.where(in0[:, None], torch.stack([q0, q2, q3], 1), torch.stack([q0, q3, q2], 1))
    faces = torch.stack([t1, t2], dim=1).reshape(-1, 3).to(torch.int32)
    return Mesh(vertices, faces, colors)


def extract_surface(sigma: torch.Tensor, rgb: Optional[torch.Tensor] = None, iso: float = 0.5,
                    bound: float = 1.0) -> Mesh:
    """Naive surface nets (include/lgm_mesh.h, extraction pass) on sigma [Gx, Gy, Gz], a grid over [-bound, bound]^3:
    one vertex per cell the iso-surface passes through, two triangles per grid edge it crosses. The outermost node
    layer is read as 0, so every mesh is closed; normals point out of the dense side. rgb [Gx, Gy, Gz, 3] colours
    the vertices. iso = 0.5 is a choice, not a tuned value."""
    if sigma.dim() != 3:
        raise ValueError(f"sigma of shape {tuple(sigma.shape)}: expected [Gx, Gy, Gz]")
    G, lo, h = grid_params(tuple(sigma.shape), bound)
    if not (iso > 0 and np.isfinite(iso)):
        raise ValueError(f"iso {iso} must be positive and finite")
    sigma = sigma.detach().to(torch.float32).contiguous()
    if rgb is not None:
        if tuple(rgb.shape) != G + (3,) or rgb.device != sigma.device:
            raise ValueError(f"rgb of shape {tuple(rgb.shape)} on {rgb.device}: expected {G + (3,)} on {sigma.device}")
        rgb = rgb.detach().to(torch.float32).contiguous()
    return (_extract_native if sigma.is_cuda else _extract_torch)(sigma, rgb, iso, G, lo, h)


def gaussians_to_mesh(gaussians: torch.Tensor, resolution: Union[int, Sequence[int]] = 256, iso: float = 0.5,
                      bound: float = 1.0, min_opacity: float = 0.005, scale_modifier: float = 1.0) -> Mesh:
    """Gaussians [N, 14] or [1, N, 14] -> a closed, coloured triangle mesh: save_ply's opacity prune (>= min_opacity),
    density_grid, extract_surface. resolution = 256 is convert.py's grid; iso = 0.5 is a choice, not a tuned value (no
    trained checkpoint exists offline to tune it on)."""
    g = _check_gaussians(gaussians)
    g = g[g[:, 3] >= min_opacity]
    sigma, rgb = density_grid(g, resolution, bound, scale_modifier)
    return extract_surface(sigma, rgb, iso, bound)
