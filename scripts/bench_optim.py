"""Timing of the fused optimizer step (lgm_amd.optim.AdamW(max_grad_norm=1): k_optim_sqnorm + k_optim_reduce +
k_optim_adamw) against torch's composition on the same GPU, on the default LGM's own parameter list with random
gradients:

  fused    lgm_amd.AdamW(max_grad_norm=1).step()
  torch_f  torch.nn.utils.clip_grad_norm_(params, 1) + torch.optim.AdamW(fused=True).step()
  torch_e  the same with foreach=True

Each arm has its own copy of the parameters, gradients and state (the update is in place); all get the same values.
The gradients stay in place between steps (no zero_grad: allocation is not what is timed), so torch's clip rescales
already-scaled gradients on later steps: same work, other numbers. Reported: median time per step of each arm, the
ratios, the host time of enqueueing one fused step (a host clock around steps that nothing waits for), the kernels'
own times (the library's profiler, a separate pass), and the model bytes over the fused time with
its share of the HBM peak (8.0 TB/s): 4 B read per element for the norm + 16 B read and 12 B written for the update
= 32 B per element; torch's composition moves 4 + 8 + 28 = 40 B.
Protocol: all arms warmed up first; the arms alternate inside one process; a sample is `--inner` steps between two
device events; medians over `--reps` samples. Writes bench_optim.json under --out and prints the row.

    python scripts/bench_optim.py [--out profiles/optim] [--reps 15] [--inner 5] [--preset lrm] [--misaligned]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (spec)
HP = dict(lr=4e-4, betas=(0.9, 0.95), weight_decay=0.05)  # main.py:73


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3  # us per step


def interleaved(fns, reps, inner, warm=3):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
            t.append(timed(fn, inner))
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim"))
    ap.add_argument("--preset", default="lrm")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--misaligned", action="store_true",
                    help="the fused arm's parameters and gradients are views at odd element offsets of flat buffers "
                         "(only 4-byte aligned, as DDP bucket views can be): the kernels' element path")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a GPU: timings are taken on the device")
    from lgm_amd import LGM, preset
    from lgm_amd import _native as nat
    from lgm_amd import build as B_
    from lgm_amd import optim as O
    B_.build()
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in LGM(preset(a.preset)).parameters() if p.requires_grad]
    numel = sum(torch.Size(s).numel() for s in shapes)

    def arm(misaligned=False):
        gen = torch.Generator(device=dev).manual_seed(0)
        ps = []
        for s in shapes:
            p, g = torch.randn(s, device=dev, generator=gen), torch.randn(s, device=dev, generator=gen)
            if misaligned:
                n = p.numel()
                fp, fg = torch.empty(n + 8, device=dev), torch.empty(n + 8, device=dev)
                fp[1:1 + n].copy_(p.reshape(-1))
                fg[3:3 + n].copy_(g.reshape(-1))
                p, g = fp[1:1 + n].view(s), fg[3:3 + n].view(s)
            p.requires_grad_()
            p.grad = g
            ps.append(p)
        return ps

    pf, pt, pe = arm(a.misaligned), arm(), arm()
    fused_opt = O.AdamW(pf, max_grad_norm=1.0, **HP)
    torch_f = torch.optim.AdamW(pt, fused=True, **HP)
    torch_e = torch.optim.AdamW(pe, foreach=True, **HP)

    def fused():
        fused_opt.step()

    def plain_f():
        torch.nn.utils.clip_grad_norm_(pt, 1.0)
        torch_f.step()

    def plain_e():
        torch.nn.utils.clip_grad_norm_(pe, 1.0)
        torch_e.step()

    (tf, tt, te), spread = interleaved([fused, plain_f, plain_e], a.reps, a.inner)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.inner):
        fused()
    host_us = (time.perf_counter() - t0) / a.inner * 1e6
    torch.cuda.synchronize()
    prof = nat.KernelProfiler()
    with prof:
        for _ in range(a.inner):
            fused()
    kern = {k: round(ms / n * 1e3, 2) for k, (n, ms) in prof.summary().items()}  # us per launch
    prof.close()
    moved = 32 * numel
    row = {"preset": a.preset, "misaligned": a.misaligned, "tensors": len(shapes), "numel": numel,
           "chunks": sum(-(-torch.Size(s).numel() // nat.OPTIM_CHUNK) for s in shapes),
           "fused_us": round(tf, 2), "torch_fused_us": round(tt, 2), "torch_foreach_us": round(te, 2),
           "min_max_us": [[round(x, 2) for x in s] for s in spread],
           "speedup_vs_torch_fused": round(tt / tf, 3), "speedup_vs_torch_foreach": round(te / tf, 3),
           "fused_host_us": round(host_us, 2), "kernel_us": kern, "model_bytes": moved, "torch_model_bytes": 40 * numel,
           "fused_bytes_per_s": round(moved / (tf * 1e-6), 0),
           "fused_hbm_fraction": round(moved / (tf * 1e-6) / HBM_PEAK, 4)}
    print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "reps": a.reps, "inner": a.inner,
           "rows": [row]}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_optim.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
