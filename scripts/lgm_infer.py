"""infer.py's flow on lgm_amd alone (no reference checkout): an RGBA PNG -> 4 views + rays (the recipe of
scripts/cfg1_cpu.load_views: the image composited on white and replicated to the four views MVDream would generate)
-> native LGM ('big': lgm_amd.models.LGM on the fused GroupNorm+SiLU, attention, head and render kernels) -> save_ply
and N orbit frames through lgm_amd.cameras.render_orbit_frames. Runs on the GPU or, with --device cpu, on the CPU
(torch paths of lgm_amd/cpu.py). Without --ckpt the weights are a seeded random init (no checkpoint exists offline).

    python scripts/lgm_infer.py [--png tests/golden/catstatue_rgba.png] [--ckpt STATE_DICT.pt] [--frames 8]
                                [--device cuda|cpu] [--bf16] [--native-conv] [--out bench_out_lgm_infer]
                                [--mesh [OBJ]] [--mesh-resolution 256] [--mesh-iso 0.5] [--mesh-texels N] [--mesh-fit K]

--native-conv (with --bf16 on the GPU) runs the UNet's stride-1 convolutions on the HIP kernel (UNet.native_conv)
instead of the library convolution: no first-call solver search.
--mesh also writes object.obj next to the PLY (lgm_amd.mesh: the Gaussians' density on a grid, surface nets) and adds
its vertex and face counts to the JSON line. --mesh-texels N bakes a texture from the Gaussians at N texels per quad
edge (object.mtl and object.png next to the OBJ) and adds its size to the JSON line. --mesh OBJ writes to that path
instead. --mesh-fit K (with --mesh-texels) fits that texture to renders of the Gaussians for K iterations
(lgm_amd.meshraster.fit_texture) and adds the first and last loss to the JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--png", default=os.path.join(ROOT, "tests", "golden", "catstatue_rgba.png"))
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out_lgm_infer"))
    ap.add_argument("--ckpt", default=None, help="a state_dict file (torch.save) of LGM 'big'")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--frames", type=int, default=8, help="orbit frames to render")
    ap.add_argument("--render-size", type=int, default=256)
    ap.add_argument("--antialias", action="store_true",
                    help="orbit frames with the opacity compensation of the 0.3 px^2 dilation (Options.antialias)")
    ap.add_argument("--bf16", action="store_true", help="run the model under bf16 autocast (GPU)")
    ap.add_argument("--native-conv", action="store_true",
                    help="the UNet's stride-1 convolutions on the HIP kernel (16-bit on the GPU: with --bf16)")
    ap.add_argument("--mesh", nargs="?", const=True, default=False, metavar="OBJ",
                    help="also export a coloured triangle mesh (object.obj in --out, or the given path)")
    ap.add_argument("--mesh-resolution", type=int, default=256)
    ap.add_argument("--mesh-iso", type=float, default=0.5)
    ap.add_argument("--mesh-texels", type=int, default=None,
                    help="with --mesh: texels per quad edge of a texture baked from the Gaussians (default: vertex colours)")
    ap.add_argument("--mesh-fit", type=int, default=0,
                    help="with --mesh-texels: iterations of the texture fit against renders of the Gaussians (default: none)")
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.threads > 0:
        torch.set_num_threads(a.threads)
    from cfg1_cpu import load_views
    from PIL import Image

    from lgm_amd import LGM, preset
    from lgm_amd.cameras import render_orbit_frames
    dev = torch.device(a.device)
    if dev.type == "cuda":
        from lgm_amd import build as B
        B.build()
    opt = preset("big", output_size=a.render_size, antialias=a.antialias)
    t = {}
    t0 = time.perf_counter()
    torch.manual_seed(a.seed)
    model = LGM(opt)
    if a.ckpt:
        sd = torch.load(a.ckpt, map_location="cpu", weights_only=True)
        model.load_state_dict(sd.get("model", sd) if isinstance(sd, dict) else sd, strict=True)
    model = model.to(dev).eval()
    model.unet.native_conv = bool(a.native_conv)
    t["build_s"] = time.perf_counter() - t0
    images = load_views(a.png, opt.input_size).to(dev)  # [1, 4, 9, 256, 256]
    with torch.no_grad():
        t0 = time.perf_counter()
        if a.bf16 and dev.type == "cuda":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                gaussians = model.forward_gaussians(images)
        else:
            gaussians = model.forward_gaussians(images)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t["model_s"] = time.perf_counter() - t0
        os.makedirs(a.out, exist_ok=True)
        ply = os.path.join(a.out, "catstatue.ply" if "catstatue" in a.png else "object.ply")
        model.gs.save_ply(gaussians, ply)
        mesh_info = {}
        if a.mesh:
            t0 = time.perf_counter()
            obj = os.path.join(a.out, "object.obj") if a.mesh is True else a.mesh
            mesh = model.gs.save_mesh(gaussians.float(), obj, resolution=a.mesh_resolution, iso=a.mesh_iso,
                                      texels=a.mesh_texels, fit_iters=a.mesh_fit)
            t["mesh_s"] = time.perf_counter() - t0
            mesh_info = {"mesh": obj, "mesh_vertices": int(mesh.vertices.shape[0]), "mesh_faces": int(mesh.faces.shape[0])}
            if mesh.texture is not None:
                mesh_info["mesh_texture"] = [int(mesh.texture.shape[1]), int(mesh.texture.shape[0])]  # W, H
            if mesh.fit is not None:
                mesh_info["mesh_fit"] = mesh.fit
        t0 = time.perf_counter()
        az = np.arange(a.frames, dtype=np.float64) * (360.0 / max(a.frames, 1))
        frames = render_orbit_frames(model.gs, gaussians, az, radius=opt.cam_radius).cpu().numpy()
        t["render_s"] = time.perf_counter() - t0
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(a.out, f"frame_{i:03d}.png"))
    print(json.dumps({"device": str(dev), "gaussians": list(gaussians.shape), "finite": bool(torch.isfinite(gaussians).all()),
                      "ply": ply, "ply_bytes": os.path.getsize(ply), "frames": list(frames.shape),
                      "frame_mean": float(frames.mean()), **mesh_info, "seconds": {k: round(v, 3) for k, v in t.items()}}))


if __name__ == "__main__":
    main()
