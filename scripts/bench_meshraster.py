"""Times the mesh rasteriser (lgm_amd.meshraster, include/lgm_meshraster.h) on the GPU at the workload's shape and
prints one JSON line:

  forward / backward  render_mesh and its gradient to the texture on the --resolution^3 (256) textured mesh of --n
                      (65,536) synthetic Gaussians (lgm_amd.synthetic) at --size^2 (512) pixels, V = 1 and 8 orbit views:
                      device-event medians per call, the kernels' own times (KernelProfiler, in a pass of its own), the
                      algorithmic bytes and their share of the 8 TB/s HBM peak
  fit_iteration       one whole fit_texture iteration (Gaussian render, mesh render, loss, backward, AdamW, clamp), V = 1
  psnr                mesh_psnr on 8 held-out orbit views before and after fit_texture(iters=--fit-iters): the export's
                      quality number (--fit-iters 0 skips the fit)

    python scripts/bench_meshraster.py [--resolution 256] [--n 65536] [--texels 4] [--size 512] [--iters 20]
                                       [--warmup 3] [--fit-iters 512]

Algorithmic bytes per call (what the algorithm has to move once, from the shapes): the projected vertices (16 B written
and read per (view, vertex)), the faces (12 B per (view, face)), the visibility buffer (8 B cleared and 8 B read per
pixel), the outputs (24 B per pixel) and the texture touched (12 B per texel some pixel reads, counted from a gradient
of ones); the backward: d_image twice, the visibility buffer, the int64 accumulators (cleared, read) and d_texture. The
dense torch path cannot run at this size, so there is no baseline ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def event_median(fn, warmup: int, iters: int) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "iters": iters}


def kernels(fn, iters: int) -> dict:
    from lgm_amd import _native as nat
    prof = nat.KernelProfiler()
    with prof:
        for _ in range(iters):
            fn()
    torch.cuda.synchronize()
    out = {k: round(ms / iters, 4) for k, (n, ms) in prof.summary().items()}
    prof.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--texels", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-iters", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshraster.py measures on the GPU: no GPU found")
    from dataclasses import replace

    from lgm_amd import Options
    from lgm_amd import build as B
    from lgm_amd import mesh as M
    from lgm_amd import meshraster as MR
    from lgm_amd.cameras import orbit_cameras_batched
    from lgm_amd.synthetic import synthetic_gaussians
    B.build()
    dev = torch.device("cuda:0")
    opt = Options(output_size=a.size)
    g = synthetic_gaussians(1, a.n, seed=0)[0].to(dev)
    mesh = M.gaussians_to_mesh(g, a.resolution, texels=a.texels)
    g = g[g[:, 3] >= 0.005].contiguous()  # gaussians_to_mesh's prune
    Nv, Nf = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    Ht, Wt = int(mesh.texture.shape[0]), int(mesh.texture.shape[1])
    S = a.size
    res = {"device": torch.cuda.get_device_name(0), "resolution": a.resolution, "gaussians": int(g.shape[0]),
           "vertices": Nv, "faces": Nf, "texture": [Wt, Ht], "size": S}
    for V in (1, 8):
        az = torch.arange(V, dtype=torch.float64) * (360.0 / V) + 13.0
        cv, cvp, _ = orbit_cameras_batched(torch.full((V,), -17.0, dtype=torch.float64), az, opt.cam_radius, opt.fovy,
                                           opt.znear, opt.zfar, device=dev)
        tex = mesh.texture.clone().requires_grad_(True)
        work = replace(mesh, texture=tex)
        out = MR.render_mesh(work, cv, cvp, S, S)
        ones, = torch.autograd.grad(out["image"], tex, torch.ones_like(out["image"]), retain_graph=True)
        touched = int((ones != 0).any(dim=2).sum())
        covered = int(out["alpha"].sum())
        d = torch.randn_like(out["image"])
        P = V * S * S
        fwd_bytes = {"projected_vertices": 2 * 16 * V * Nv + 12 * Nv, "faces": 12 * V * Nf, "visibility_buffer": 16 * P,
                     "outputs": 24 * P, "texture_touched": 12 * touched}
        bwd_bytes = {"d_image": 2 * 12 * P, "visibility_buffer": 8 * P, "accumulators": 2 * 24 * Ht * Wt,
                     "d_texture": 12 * Ht * Wt, "texture_touched_atomics": 24 * touched}
        with torch.no_grad():
            f = event_median(lambda: MR.render_mesh(mesh, cv, cvp, S, S), a.warmup, a.iters)
        b = event_median(lambda: torch.autograd.grad(out["image"], tex, d, retain_graph=True), a.warmup, a.iters)
        with torch.no_grad():
            fk = kernels(lambda: MR.render_mesh(mesh, cv, cvp, S, S), a.iters)
        bk = kernels(lambda: torch.autograd.grad(out["image"], tex, d, retain_graph=True), a.iters)
        for t, by, ks in ((f, fwd_bytes, fk), (b, bwd_bytes, bk)):
            t["bytes"] = by
            t["bytes_total"] = sum(by.values())
            t["kernels_ms"] = ks
            t["kernel_ms_total"] = round(sum(ks.values()), 4)
            t["hbm_share_of_call"] = round(t["bytes_total"] / (t["median_ms"] * 1e-3) / HBM_PEAK, 4)
            t["hbm_share_of_kernels"] = round(t["bytes_total"] / (max(t["kernel_ms_total"], 1e-9) * 1e-3) / HBM_PEAK, 4)
        res[f"V{V}"] = {"covered_pixels": covered, "texels_touched": touched, "forward": f, "backward": b}
        del out, ones
    # one whole fit_texture iteration: the time of a 1 + k iteration fit less that of a 1 iteration fit, over k
    k = 16

    def fit(n):
        return MR.fit_texture(mesh, g, opt, iters=n, resolution=S)

    t1 = event_median(lambda: fit(1), 1, 3)["median_ms"]
    tk = event_median(lambda: fit(1 + k), 1, 3)["median_ms"]
    res["fit_iteration"] = {"ms": round((tk - t1) / k, 4), "fit_1_ms": t1, f"fit_{1 + k}_ms": tk}
    # the payoff: PSNR against the Gaussians' renders on 8 held-out views (not among fit_poses' draws: fixed angles)
    az = torch.arange(8, dtype=torch.float64) * 45.0 + 22.5
    el = torch.tensor([-30.0, 10.0, 40.0, -10.0, 25.0, -45.0, 0.0, 60.0], dtype=torch.float64)
    cv, cvp, _ = orbit_cameras_batched(el, az, opt.cam_radius, opt.fovy, opt.znear, opt.zfar, device=dev)
    res["psnr"] = {"views": 8, "before": round(MR.mesh_psnr(mesh, g, opt, cv, cvp, S, S), 4),
                   "vertex_colours": round(MR.mesh_psnr(replace(mesh, texture=None, uvs=None, face_uvs=None), g, opt, cv,
                                                        cvp, S, S), 4)}
    if a.fit_iters > 0:
        fitted = MR.fit_texture(mesh, g, opt, iters=a.fit_iters, resolution=S)
        res["psnr"].update(after=round(MR.mesh_psnr(fitted, g, opt, cv, cvp, S, S), 4), fit_iters=a.fit_iters,
                           loss_first=fitted.fit["loss_first"], loss_last=fitted.fit["loss_last"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
