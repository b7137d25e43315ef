"""Timing of the fused LPIPS kernels against the torch composition, on the shapes of LGM's training loss.

(a) Per tap: the five VGG16 taps of a 256 x 256 image (64 x 256^2, 128 x 128^2, 256 x 64^2, 512 x 32^2, 512 x 16^2)
    at 8 and 64 images, on bf16 features (under bf16 autocast, as the trunk hands them over in training) and on fp32
    features: `lpips_distance(f0, f1, w)` forward + backward (gradient to f1 only: the ground-truth side needs none)
    with fused = True against fused = False. Reported: median time of each, their ratio, and the bytes the fused pass
    has to move (forward f0 + f1 + the two norms, backward f0 + f1 + the norms + df1) over its time as a share of the
    HBM peak (8.0 TB/s).
(b) The input pass: loss_from_render's composite + resize + scaling of 8 and 64 views, S = 256 and 512 -> 256, forward
    + backward, fused against the torch lines.
(c) The whole module: LPIPS(size=256).loss_from_render forward + backward under bf16 autocast at 8 and 64 views
    (S = 256), fused against fused = False: median step time and torch.cuda.max_memory_allocated of each.
Protocol: every shape warmed up first; A and B alternate inside one process; a sample is `--inner` calls between two
device events; medians over `--reps` samples. Writes bench_lpips.json under --out and prints each row.

    python scripts/bench_lpips.py [--out profiles/lpips] [--images 8 64] [--reps 15] [--skip-module]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (spec)
TAPS = ((64, 256), (128, 128), (256, 64), (512, 32), (512, 16))  # (C, H = W) at a 256 x 256 input


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


def bench_taps(dev, images, reps, inner):
    from lgm_amd.lpips import lpips_distance
    rows = []
    for C, H in TAPS:
        for mode in ("bf16", "fp32"):
            for N in images:
                dt = torch.bfloat16 if mode == "bf16" else torch.float32
                f0 = torch.relu(torch.randn(N, C, H, H, device=dev)).to(dt)
                f1 = torch.relu(torch.randn(N, C, H, H, device=dev)).to(dt).requires_grad_(True)
                w = torch.rand(C, device=dev)
                g = torch.rand(N, device=dev)

                def run(fused):
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
                        d = lpips_distance(f0, f1, w, 1e-10, fused)
                    d.float().backward(g)
                    f1.grad = None

                tf, tp = ab(lambda: run(True), lambda: run(False), reps, inner)
                es, n = f0.element_size(), f0.numel()
                moved = (2 * n * es + 2 * N * H * H * 4) + (3 * n * es + 2 * N * H * H * 4)
                rows.append({"C": C, "H": H, "W": H, "mode": mode, "images": N, "fused_us": round(tf, 2),
                             "torch_us": round(tp, 2), "speedup": round(tp / tf, 3), "fused_bytes": moved,
                             "fused_hbm_fraction": round(moved / (tf * 1e-6) / HBM_PEAK, 4)})
                print(json.dumps(rows[-1]), flush=True)
                del f0, f1
                torch.cuda.empty_cache()
    return rows


def random_module(dev, size=256):
    from lgm_amd import LPIPS
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LPIPS(size=size).to(dev)


def render_like(dev, M, S):
    gen = torch.Generator(device="cpu").manual_seed(M + S)
    gt = torch.rand(1, M, 3, S, S, generator=gen).to(dev)
    mask = (torch.rand(1, M, 1, S, S, generator=gen) > 0.5).float().to(dev)
    pred = torch.rand(1, M, 3, S, S, generator=gen).to(dev).requires_grad_(True)
    return gt, mask, torch.rand(3, generator=gen).to(dev), pred


def bench_prep(dev, images, reps, inner):
    import torch.nn.functional as F

    from lgm_amd.lpips import SCALE, SHIFT, _LpipsPrep
    rows = []
    shift, scale = torch.tensor(SHIFT, device=dev).view(1, 3, 1, 1), torch.tensor(SCALE, device=dev).view(1, 3, 1, 1)
    for S in (256, 512):
        for M in images:
            gt, mask, bg, pred = render_like(dev, M, S)
            gt, mask, p = gt[0], mask[0], pred[0]
            dx = torch.randn(M, 3, 256, 256, device=dev)

            def fused():
                xp, xg = _LpipsPrep.apply(p, gt, mask, bg, 256, torch.float32)
                xp.backward(dx)
                pred.grad = None

            def plain():
                g = gt * mask + bg.view(1, 3, 1, 1) * (1 - mask)
                xg = (F.interpolate(g * 2 - 1, (256, 256), mode="bilinear", align_corners=False) - shift) / scale
                xp = (F.interpolate(p * 2 - 1, (256, 256), mode="bilinear", align_corners=False) - shift) / scale
                xp.backward(dx)
                pred.grad = None
                return xg

            tf, tp = ab(fused, plain, reps, inner)
            rows.append({"S": S, "R": 256, "images": M, "fused_us": round(tf, 2), "torch_us": round(tp, 2),
                         "speedup": round(tp / tf, 3)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_module(dev, images, reps):
    m = random_module(dev)
    rows = []
    for M in images:
        gt, mask, bg, pred = render_like(dev, M, 256)

        def step(fused):
            m.fused = fused
            with torch.autocast("cuda", dtype=torch.bfloat16):
                d = m.loss_from_render(gt, mask, bg, pred)
            d.float().mean().backward()
            pred.grad = None

        res = {}
        for fused in (True, False):  # warm-up, and the peak memory of one step of each
            step(fused)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            step(fused)
            torch.cuda.synchronize()
            res[fused] = torch.cuda.max_memory_allocated(dev) - base
        tf, tp = ab(lambda: step(True), lambda: step(False), reps, 1, warm=0)
        rows.append({"images": M, "fused_ms": round(tf / 1e3, 3), "unfused_ms": round(tp / 1e3, 3),
                     "speedup": round(tp / tf, 3), "fused_peak_bytes_above_inputs": res[True],
                     "unfused_peak_bytes_above_inputs": res[False]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips"))
    ap.add_argument("--images", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--module-reps", type=int, default=5)
    ap.add_argument("--skip-taps", action="store_true")
    ap.add_argument("--skip-prep", action="store_true")
    ap.add_argument("--skip-module", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py needs a GPU: timings are taken on the device")
    from lgm_amd import build as B
    B.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "reps": a.reps, "inner": a.inner}
    if not a.skip_taps:
        out["taps"] = bench_taps(dev, a.images, a.reps, a.inner)
    if not a.skip_prep:
        out["prep"] = bench_prep(dev, a.images, a.reps, a.inner)
    if not a.skip_module:
        out["module_bf16"] = bench_module(dev, a.images, a.module_reps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_lpips.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("taps", "prep", "module_bf16")}))


if __name__ == "__main__":
    main()
