"""Timing of the fused GroupNorm+SiLU(+resample) kernels against stock torch ops, on the shapes of LGM 'big'.

(a) Per level: every distinct GroupNorm -> SiLU (-> resample) site of UNet('big') (recorded from one forward of the
    native UNet), at B*V = 4 and 32 views, under bf16 autocast and in fp32: `group_norm_silu` forward + backward
    against F.group_norm -> F.silu -> F.avg_pool2d / F.interpolate (-> the next conv's cast to bf16 under autocast)
    called directly here. Reported: median time of each, their ratio, and the bytes the fused pass has to move
    (forward x + y, backward x + d_y + dx) over its time as a fraction of the HBM peak (8.0 TB/s).
(b) UNet('big') forward + backward under bf16 autocast at 4 and 32 views, fused = True against fused = False:
    median step time and torch.cuda.max_memory_allocated.
Protocol: every shape warmed up first; A and B alternate inside one process; a sample is `--inner` calls between two
device events; medians over `--reps` samples. Writes bench_unet.json under --out and prints it.

    python scripts/bench_unet.py [--out profiles/unet_gnsilu] [--views 4 32] [--reps 15] [--skip-unet]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (spec)


def big_sites(dev):
    """(C, H, W, groups, resample) -> count, over the GroupNorm+SiLU sites of one UNet('big') forward."""
    import lgm_amd.unet as U
    from lgm_amd import preset
    opt = preset("big")
    sites = {}
    orig = U.group_norm_silu

    def record(x, norm, resample=None):
        key = (x.shape[1], x.shape[2], x.shape[3], norm.num_groups, resample or "none")
        sites[key] = sites.get(key, 0) + 1
        return orig(x, norm, resample)

    U.group_norm_silu = record
    try:
        with torch.device("meta"):
            u = U.UNet(9, 14, down_channels=opt.down_channels, down_attention=opt.down_attention,
                       mid_attention=opt.mid_attention, up_channels=opt.up_channels, up_attention=opt.up_attention)
            for m in u.modules():
                if isinstance(m, U.MVAttention):
                    m.fused = False  # (meta tensors: shapes only)
            u(torch.empty(4, 9, opt.input_size, opt.input_size))
    finally:
        U.group_norm_silu = orig
    # 'big' builds no resampling ResnetBlock (its blocks resample with convolutions): one level of each, so that the
    # resample forms of the kernels are timed too (sites = 0: not part of the model)
    sites[(128, 128, 128, 32, "up")] = 0
    sites[(128, 128, 128, 32, "down")] = 0
    return sites


def stock(x, norm, resample, autocast):
    y = F.silu(F.group_norm(x.float() if autocast else x, norm.num_groups, norm.weight, norm.bias, norm.eps))
    if resample == "up":
        y = F.interpolate(y, scale_factor=2.0, mode="nearest")
    elif resample == "down":
        y = F.avg_pool2d(y, kernel_size=2, stride=2)
    return y.to(torch.bfloat16) if autocast else y


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


def bench_levels(dev, views, reps, inner):
    from lgm_amd.unet import group_norm_silu
    rows = []
    for (C, H, W, G, rs), count in sorted(big_sites(dev).items(), key=lambda kv: (-kv[0][1], kv[0][0], kv[0][4])):
        resample = None if rs == "none" else rs
        for mode in ("bf16", "fp32"):
            for N in views:
                norm = nn.GroupNorm(G, C).to(dev)
                xdt = torch.bfloat16 if mode == "bf16" else torch.float32  # under autocast the convs hand over bf16
                x = torch.randn(N, C, H, W, device=dev).to(xdt).requires_grad_(True)
                oh, ow = (2 * H, 2 * W) if rs == "up" else (H // 2, W // 2) if rs == "down" else (H, W)
                dy = torch.randn(N, C, oh, ow, device=dev).to(xdt)

                def fused():
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
                        y = group_norm_silu(x, norm, resample)
                    y.backward(dy)

                def plain():
                    y = stock(x, norm, resample, mode == "bf16")
                    y.backward(dy)

                tf, tp = ab(fused, plain, reps, inner)
                es = x.element_size()
                moved = (2 * x.numel() + 2 * dy.numel()) * es + x.numel() * es  # fwd x + y, bwd x + d_y + dx
                rows.append({"C": C, "H": H, "W": W, "groups": G, "resample": rs, "sites": count, "mode": mode,
                             "views": N, "fused_us": round(tf, 2), "stock_us": round(tp, 2),
                             "speedup": round(tp / tf, 3), "fused_bytes": moved,
                             "fused_hbm_fraction": round(moved / (tf * 1e-6) / HBM_PEAK, 4)})
                print(json.dumps(rows[-1]), flush=True)
                x.grad = None
                norm.zero_grad()
    return rows


def bench_unet(dev, views, reps):
    from lgm_amd import UNet, preset
    opt = preset("big")
    torch.manual_seed(0)
    u = UNet(9, 14, down_channels=opt.down_channels, down_attention=opt.down_attention,
             mid_attention=opt.mid_attention, up_channels=opt.up_channels, up_attention=opt.up_attention).to(dev)
    rows = []
    for N in views:
        x = torch.randn(N, 9, opt.input_size, opt.input_size, device=dev)

        def step(fused):
            u.fused = fused
            u.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = u(x)
            y.float().square().mean().backward()

        res = {}
        for fused in (True, False):  # warm-up, and the peak memory of one step of each
            step(fused)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            step(fused)
            torch.cuda.synchronize()
            res[fused] = {"max_memory_allocated": torch.cuda.max_memory_allocated(dev)}
        tf, tp = ab(lambda: step(True), lambda: step(False), reps, 1, warm=0)
        rows.append({"views": N, "fused_ms": round(tf / 1e3, 3), "unfused_ms": round(tp / 1e3, 3),
                     "speedup": round(tp / tf, 3), "fused_max_memory": res[True]["max_memory_allocated"],
                     "unfused_max_memory": res[False]["max_memory_allocated"]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_gnsilu"))
    ap.add_argument("--views", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--unet-reps", type=int, default=5)
    ap.add_argument("--skip-unet", action="store_true")
    ap.add_argument("--skip-levels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet.py needs a GPU: timings are taken on the device")
    from lgm_amd import build as B
    B.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "reps": a.reps,
           "inner": a.inner}
    if not a.skip_levels:
        out["levels"] = bench_levels(dev, a.views, a.reps, a.inner)
    if not a.skip_unet:
        out["unet_big_bf16"] = bench_unet(dev, a.views, a.unet_reps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_unet.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("levels", "unet_big_bf16")}))


if __name__ == "__main__":
    main()
