"""Timing of the fused batch assembly (lgm_amd.data.build_batch: lgm_data_cameras + lgm_data_views) against the torch
composition of the provider's lines (lgm_amd.data.build_batch_torch) on the same GPU, at the workload shapes:

  big    B 8, V 8, Vi 4, 512 x 512 uint8 RGBA -> h 256, So 512
  small  B 8, V 12, Vi 4, 512 x 512 uint8 RGBA -> h 256, So 256

with the augmentations on (every sample distorted and jittered: the dearest case) and off. Both sides get the uint8
views, the poses and one set of draws already made; host draws are not timed. Reported per row: median time of each, the
ratio, the kernels' own times (the library's profiler, a separate pass), and the model bytes (source bytes read once +
output bytes written) over the fused time, with its share of the HBM peak (8.0 TB/s).
Protocol: both warmed up first; A and B alternate inside one process; a sample is `--inner` calls between two device
events; medians over `--reps` samples. Writes bench_data.json under --out and prints each row.

    python scripts/bench_data.py [--out profiles/data] [--reps 15] [--inner 5] [--configs big small]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (spec)
CONFIGS = {"big": dict(B=8, V=8, Hs=512), "small": dict(B=8, V=12, Hs=512)}


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3  # us per call


def ab(fa, fb, reps, inner, warm=3):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa, inner))
        tb.append(timed(fb, inner))
    return statistics.median(ta), statistics.median(tb)


def inputs(dev, B, V, Hs, seed=0):
    from lgm_amd.cameras import orbit_camera
    gen = torch.Generator().manual_seed(seed)
    rgba = torch.randint(0, 256, (B, V, Hs, Hs, 4), dtype=torch.uint8, generator=gen)
    c2w = np.stack([np.stack([orbit_camera(-10.0 - 3 * b - 5 * v, 40.0 * v + 7 * b, radius=1.5) for v in range(V)])
                    for b in range(B)])
    return rgba.to(dev), torch.from_numpy(c2w).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data"))
    ap.add_argument("--configs", nargs="+", default=["big", "small"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_data.py needs a GPU: timings are taken on the device")
    from lgm_amd import _native as nat
    from lgm_amd import build as B_
    from lgm_amd import data as D
    from lgm_amd.options import preset
    B_.build()
    dev = torch.device("cuda:0")
    rows = []
    for name in a.configs:
        c = CONFIGS[name]
        opt = preset(name)
        assert opt.num_views == c["V"], (name, opt.num_views)
        rgba, c2w = inputs(dev, c["B"], c["V"], c["Hs"])
        Vi, h, So = opt.num_input_views, opt.input_size, opt.output_size
        moved = rgba.numel() + 4 * (c["B"] * Vi * 9 * h * h + c["B"] * c["V"] * 4 * So * So)
        for augment in (True, False):
            aug = None
            if augment:
                aug = D.draw_augmentation(dataclasses.replace(opt, prob_grid_distortion=1.0, prob_cam_jitter=1.0),
                                          c["B"], torch.Generator().manual_seed(1))

            def fused():
                return D.build_batch(opt, rgba, c2w, augment, augmentation=aug)

            def plain():
                return D.build_batch_torch(opt, rgba, c2w, aug)

            tf, tp = ab(fused, plain, a.reps, a.inner)
            prof = nat.KernelProfiler()
            with prof:
                for _ in range(a.inner):
                    fused()
            kern = {k: round(ms / n * 1e3, 2) for k, (n, ms) in prof.summary().items()}  # us per launch
            prof.close()
            rows.append({"config": name, "B": c["B"], "V": c["V"], "Vi": Vi, "Hs": c["Hs"], "h": h, "So": So,
                         "augment": augment, "fused_us": round(tf, 2), "torch_us": round(tp, 2),
                         "speedup": round(tp / tf, 3), "kernel_us": kern, "model_bytes": moved,
                         "fused_bytes_per_s": round(moved / (tf * 1e-6), 0),
                         "fused_hbm_fraction": round(moved / (tf * 1e-6) / HBM_PEAK, 4)})
            print(json.dumps(rows[-1]), flush=True)
        del rgba
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "reps": a.reps, "inner": a.inner,
           "rows": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_data.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
