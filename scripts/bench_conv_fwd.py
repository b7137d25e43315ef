"""Timing of the conv forward and input gradient kernels (lgm_conv_forward / lgm_conv_dgrad) against the library
convolution, on the shapes of LGM 'big'.

(a) Per shape: every distinct (Cin, Cout, H, W, ksize) stride-1 convolution site of UNet('big') (bench_conv.big_sites),
    at B*V = 4 and 32 views, in bf16: `lgm_amd.conv.conv_forward` on the fp32 weight and bias (the packing pass is part
    of the call) against F.conv2d on 16-bit operands, and `lgm_amd.conv.conv_dgrad` against aten.convolution_backward
    with output_mask [True, False, False]. Reported: median time of each, TFLOP/s (2 * N * H * W * Cin * Cout * k^2 per
    call) and their ratio.
(b) UNet('big') forward + backward under bf16 autocast at 4 and 32 views, native_conv = True against False
    (native_wgrad on in both arms), and the inference forward (no grad) the same way. The per-shape dispatch tables of
    lgm_amd/conv.py apply to the `on` arm; --all-native empties them first (every stride-1 conv on the kernel).
Protocol (scripts/bench_conv.py's): every shape warmed up first; the two arms alternate inside one process; a sample is
`--inner` calls between two device events; medians over `--reps` samples. Writes bench_conv_fwd.json under --out.

    python scripts/bench_conv_fwd.py [--out profiles/conv_fwd] [--views 4 32] [--reps 15] [--skip-unet] [--all-native]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_conv import big_sites, big_unet  # noqa: E402
from bench_unet import ab  # noqa: E402


def bench_shapes(dev, views, reps, inner):
    from lgm_amd.conv import conv_dgrad, conv_forward
    rows = []
    for (Cin, Cout, H, W, k, stride), count in sorted(big_sites().items(), key=lambda kv: (-kv[0][2], kv[0][0], kv[0][1])):
        if stride != 1:
            continue
        for N in views:
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn((N, Cin, H, W), device=dev, generator=g).to(torch.bfloat16)
            dy = torch.randn((N, Cout, H, W), device=dev, generator=g).to(torch.bfloat16)
            w32 = torch.randn((Cout, Cin, k, k), device=dev, generator=g) * (Cin * k * k) ** -0.5
            b32 = torch.randn((Cout,), device=dev, generator=g)
            w, b = w32.to(torch.bfloat16), b32.to(torch.bfloat16)
            p = (k - 1) // 2
            tfn, tft = ab(lambda: conv_forward(x, w32, b32, k), lambda: F.conv2d(x, w, b, 1, p), reps, inner)
            tdn, tdt = ab(lambda: conv_dgrad(dy, w32, k),
                          lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [p, p], [1, 1], False, [0, 0],
                                                                      1, [True, False, False]), reps, inner)
            flop = 2.0 * N * H * W * Cin * Cout * k * k
            rows.append({"Cin": Cin, "Cout": Cout, "H": H, "W": W, "ksize": k, "sites": count, "views": N,
                         "fwd_native_us": round(tfn, 2), "fwd_torch_us": round(tft, 2), "fwd_speedup": round(tft / tfn, 3),
                         "fwd_native_tflops": round(flop / tfn * 1e-6, 1), "fwd_torch_tflops": round(flop / tft * 1e-6, 1),
                         "dgrad_native_us": round(tdn, 2), "dgrad_torch_us": round(tdt, 2),
                         "dgrad_speedup": round(tdt / tdn, 3), "dgrad_native_tflops": round(flop / tdn * 1e-6, 1),
                         "dgrad_torch_tflops": round(flop / tdt * 1e-6, 1)})
            print(json.dumps(rows[-1]), flush=True)
            del x, dy, w, w32
    return rows


def bench_unet(dev, views, reps):
    torch.manual_seed(0)
    u, opt = big_unet(dev)
    rows = []
    for N in views:
        x = torch.randn(N, 9, opt.input_size, opt.input_size, device=dev)

        def step(native):
            u.native_conv = native
            u.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = u(x)
            y.float().square().mean().backward()

        def infer(native):
            u.native_conv = native
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return u(x)

        for native in (True, False):  # warm-up
            for fn in (step, step, infer, infer):
                fn(native)
        torch.cuda.synchronize()
        tn, tt = ab(lambda: step(True), lambda: step(False), reps, 1, warm=0)
        fn_, ft_ = ab(lambda: infer(True), lambda: infer(False), reps, 1, warm=0)
        rows.append({"views": N, "train_native_conv_ms": round(tn / 1e3, 3), "train_torch_conv_ms": round(tt / 1e3, 3),
                     "train_speedup": round(tt / tn, 3), "infer_native_conv_ms": round(fn_ / 1e3, 3),
                     "infer_torch_conv_ms": round(ft_ / 1e3, 3), "infer_speedup": round(ft_ / fn_, 3)})
        print(json.dumps(rows[-1]), flush=True)
    u.native_conv = False
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_fwd"))
    ap.add_argument("--name", default="bench_conv_fwd.json")
    ap.add_argument("--views", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--unet-reps", type=int, default=5)
    ap.add_argument("--skip-unet", action="store_true")
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--all-native", action="store_true",
                    help="empty lgm_amd.conv's forward / input-gradient dispatch tables: every stride-1 conv on the kernel")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_fwd.py needs a GPU: timings are taken on the device")
    from lgm_amd import build as B
    B.build()
    dev = torch.device("cuda:0")
    if a.all_native:
        from lgm_amd import conv as C
        C._FWD_TORCH_FASTER.clear()
        C._DGRAD_TORCH_FASTER.clear()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "all_native": a.all_native}
    if not a.skip_shapes:
        out["shapes"] = bench_shapes(dev, a.views, a.reps, a.inner)
    if not a.skip_unet:
        out["unet_big_bf16"] = bench_unet(dev, a.views, a.unet_reps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("shapes", "unet_big_bf16")}))


if __name__ == "__main__":
    main()
