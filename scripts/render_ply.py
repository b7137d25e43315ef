"""Orbit frames of a 3DGS .ply as PNG files, through GaussianRenderer (GPU if there is one, else the CPU path):
python scripts/render_ply.py scene.ply out_dir [--frames 36] [--size 512] [--elevation 0] [--radius 1.5]
                             [--sh] [--antialias]
--sh keeps the file's f_rest_* coefficients (load_ply(sh=True): view-dependent colour, LGM_RENDER_SH_MASK); without it
the file renders with its DC colour. --antialias: the opacity compensation of LGM_RENDER_ANTIALIAS."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from lgm_amd import GaussianRenderer, Options  # noqa: E402
from lgm_amd.cameras import orbit_cameras  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply")
    ap.add_argument("out_dir")
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--batch", type=int, default=12, help="views rendered per call")
    ap.add_argument("--sh", action="store_true")
    ap.add_argument("--antialias", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    r = GaussianRenderer(Options(output_size=a.size))
    g = r.load_ply(a.ply, sh=a.sh)[None].to(dev)
    print(f"{g.shape[1]} Gaussians, row width {g.shape[2]}")
    cv, cvp, cp = orbit_cameras(a.frames, radius=a.radius, elevation=a.elevation)
    os.makedirs(a.out_dir, exist_ok=True)
    bg = torch.ones(3, device=dev)
    with torch.no_grad():
        for v0 in range(0, a.frames, a.batch):
            sl = slice(v0, min(a.frames, v0 + a.batch))
            img = r.render(g, cv[None, sl].to(dev), cvp[None, sl].to(dev), cp[None, sl].to(dev), bg_color=bg,
                           antialias=a.antialias)["image"][0]
            frames = np.round(img.clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy() * 255.0).astype(np.uint8)
            for k, f in enumerate(frames):
                Image.fromarray(f).save(os.path.join(a.out_dir, f"frame_{v0 + k:04d}.png"))
    print(f"{a.frames} frames -> {a.out_dir}")


if __name__ == "__main__":
    main()
