"""Times the mesh export (lgm_amd.mesh, include/lgm_mesh.h) on the GPU and prints one JSON line:

  density_grid      at --resolution^3 (256) on --n (65,536) LGM-like Gaussians (lgm_amd.synthetic), end to end
                    (its host sync included) and per kernel (KernelProfiler, in a pass of its own)
  extract_surface   on that grid at --iso, the same two ways
  baseline          the same density by a dense, chunked torch evaluation on the same GPU, at a size it can finish
                    (--baseline-resolution^3 x --baseline-n, 64^3 x 4,096), next to the kernels at that size: there
                    is no earlier implementation to time

  --texels T        also the textured export at T texels per quad edge (off by default: the output above is then
                    unchanged): mesh_atlas (atlas_ms), sample_field at the atlas points (sample_ms, per kernel too) and
                    the whole bake_texture (texture_ms) on the mesh above, with the point count and the (Gaussian,
                    brick) pairs; and, at the baseline's size, sample_field next to the same formulas as dense,
                    chunked fp32 torch operations over the same points (sample_torch_ms)

    python scripts/bench_mesh.py [--resolution 256] [--n 65536] [--iters 20] [--warmup 3] [--texels 4]

Times are host-clock around work that ends in a device synchronise, after warm-up; the per-kernel times come from HIP
events around each launch in separate iterations (profiling slows the host side).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, warmup: int, iters: int) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "iters": iters}


def kernels(fn, iters: int) -> dict:
    from lgm_amd import _native as nat
    prof = nat.KernelProfiler()
    with prof:
        for _ in range(iters):
            fn()
    torch.cuda.synchronize()
    out = {k: {"launches_per_call": n / iters, "ms_per_call": round(ms / iters, 4)} for k, (n, ms) in prof.summary().items()}
    prof.close()
    return out


def dense_torch_density(g: torch.Tensor, G, lo, h, cutoff: float = 1e-4, X: torch.Tensor = None):
    """include/lgm_mesh.h's density by dense fp32 torch operations on g's device: every node against every Gaussian,
    in chunks of 32,768 nodes x 256 Gaussians. X [M, 3]: those points instead of the grid's nodes (sigma [M],
    rgb [M, 3])."""
    o, s, q = g[:, 3], g[:, 4:7], g[:, 7:11]
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    A = R.transpose(1, 2) / s[:, :, None]
    rho2 = 2.0 * torch.log(o / cutoff)
    mu, c = g[:, 0:3], g[:, 11:14]
    given = X is not None
    if X is None:
        ax = [float(lo[a]) + torch.arange(G[a], device=g.device, dtype=torch.float32) * float(h[a]) for a in range(3)]
        X = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3)
    sw = torch.zeros(X.shape[0], device=g.device)
    swc = torch.zeros(X.shape[0], 3, device=g.device)
    for p0 in range(0, X.shape[0], 32768):
        Xp = X[p0:p0 + 32768]
        for n0 in range(0, g.shape[0], 256):
            sl = slice(n0, n0 + 256)
            yv = torch.einsum("nka,pna->pnk", A[sl], Xp[:, None, :] - mu[sl][None])
            d2 = (yv * yv).sum(dim=2)
            w = torch.where(d2 <= rho2[sl][None], o[sl][None] * torch.exp(-0.5 * d2), torch.zeros((), device=g.device))
            sw[p0:p0 + 32768] += w.sum(dim=1)
            swc[p0:p0 + 32768] += w @ c[sl]
    if given:
        return sw, swc / sw.clamp_min(1e-30)[:, None]
    return sw.reshape(G), (swc / sw.clamp_min(1e-30)[:, None]).reshape(tuple(G) + (3,))


def texture_section(M, g, mesh, gb, a, timed_, kernels_) -> dict:
    """--texels: the textured export on `mesh` (of g at --resolution), and sample_field next to dense torch at the
    baseline's size."""
    from lgm_amd import _native as nat
    T = a.texels
    points, uvs, face_uvs, (cols, rows, W, H) = M.mesh_atlas(mesh, T)
    G, lo, h = M.grid_params(a.resolution)
    ws, _ = nat.workspace("lgm_mesh_sample_workspace_size", g.device, g.shape[0], 0, *G, 0)
    npairs = torch.zeros(1, dtype=torch.int64, device=g.device)
    nat.call("lgm_mesh_sample_count", g.device, nat.ptr(g), g.shape[0], 1.0, *G, M._c3(lo), M._c3(h), M.CUTOFF,
             nat.ptr(ws), ws.numel(), nat.ptr(npairs))
    out = {"texels": T, "quads": int(points.shape[0]), "points": int(points.shape[0]) * T * T, "texture": [W, H],
           "pairs": int(npairs.item()),
           "atlas_ms": timed_(lambda: M.mesh_atlas(mesh, T), a.warmup, a.iters),
           "sample_ms": timed_(lambda: M.sample_field(g, points, a.resolution), a.warmup, a.iters),
           "texture_ms": timed_(lambda: M.bake_texture(mesh, g, T, resolution=a.resolution), a.warmup, a.iters),
           "sample_kernels": kernels_(lambda: M.sample_field(g, points, a.resolution), a.iters),
           "atlas_kernels": kernels_(lambda: M.mesh_atlas(mesh, T), a.iters)}
    # the torch composition, at a size it can finish: the baseline's Gaussians and the atlas points of their own mesh
    Gb, lo, h = M.grid_params(a.baseline_resolution)
    mb = M.extract_surface(*M.density_grid(gb, Gb), a.iso)
    pb = M.mesh_atlas(mb, T)[0].reshape(-1, 3)
    ref_s, ref_c = dense_torch_density(gb, Gb, lo, h, X=pb)
    our_s, our_c = M.sample_field(gb, pb, Gb)
    seen = ref_s > 1e-3
    out["baseline"] = {"resolution": a.baseline_resolution, "gaussians": int(gb.shape[0]), "points": int(pb.shape[0]),
                       "max_abs_sigma_difference": float((ref_s - our_s).abs().max()),
                       "max_abs_rgb_difference": float((ref_c - our_c)[seen].abs().max()) if bool(seen.any()) else 0.0,
                       "sample_torch_ms": timed_(lambda: dense_torch_density(gb, Gb, lo, h, X=pb), 1, a.baseline_iters),
                       "sample_ms": timed_(lambda: M.sample_field(gb, pb, Gb), a.warmup, a.iters)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--iso", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-resolution", type=int, default=64)
    ap.add_argument("--baseline-n", type=int, default=4096)
    ap.add_argument("--baseline-iters", type=int, default=3)
    ap.add_argument("--texels", type=int, default=None, help="also time the textured export at this many texels per quad edge")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU: no GPU found")
    from lgm_amd import build as B
    from lgm_amd import mesh as M
    from lgm_amd.synthetic import synthetic_gaussians
    B.build()
    dev = torch.device("cuda:0")
    g = synthetic_gaussians(1, a.n, seed=0)[0].to(dev)
    g = g[g[:, 3] >= 0.005].contiguous()  # gaussians_to_mesh's prune
    res = {"device": torch.cuda.get_device_name(0), "resolution": a.resolution, "gaussians": int(g.shape[0]), "iso": a.iso}
    sigma, rgb = M.density_grid(g, a.resolution)
    res["sigma_max"] = float(sigma.max())
    res["nodes_at_or_above_iso"] = int((sigma >= a.iso).sum())
    res["density_grid"] = timed(lambda: M.density_grid(g, a.resolution), a.warmup, a.iters)
    res["density_kernels"] = kernels(lambda: M.density_grid(g, a.resolution), a.iters)
    mesh = M.extract_surface(sigma, rgb, a.iso)
    res["vertices"], res["faces"] = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    res["extract_surface"] = timed(lambda: M.extract_surface(sigma, rgb, a.iso), a.warmup, a.iters)
    res["extract_kernels"] = kernels(lambda: M.extract_surface(sigma, rgb, a.iso), a.iters)
    # the baseline, and the kernels at its size
    gb = g[:a.baseline_n].contiguous()
    Gb, lo, h = M.grid_params(a.baseline_resolution)
    ref_s, ref_c = dense_torch_density(gb, Gb, lo, h)
    our_s, our_c = M.density_grid(gb, Gb)
    res["baseline"] = {"resolution": a.baseline_resolution, "gaussians": int(gb.shape[0]),
                       "max_abs_sigma_difference": float((ref_s - our_s).abs().max()), "sigma_max": float(ref_s.max()),
                       "dense_torch": timed(lambda: dense_torch_density(gb, Gb, lo, h), 1, a.baseline_iters),
                       "density_grid": timed(lambda: M.density_grid(gb, Gb), a.warmup, a.iters)}
    if a.texels is not None:
        res["texture"] = texture_section(M, g, mesh, gb, a, timed, kernels)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
