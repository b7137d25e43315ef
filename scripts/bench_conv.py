"""Timing of the conv weight / bias gradient kernel (lgm_conv_wgrad) against torch's, on the shapes of LGM 'big'.

(a) Per shape: every distinct (Cin, Cout, H, W, ksize) stride-1 convolution site of UNet('big') (recorded with forward
    hooks from one meta-device forward, with the number of sites that share the shape; the stride-2 downsample sites
    are listed but not timed: the kernel does not take them), at B*V = 4 and 32 views, in bf16: `lgm_amd.conv.wgrad`
    against torch's weight + bias gradient alone, aten.convolution_backward with output_mask [False, True, True].
    Reported: median time of each, TFLOP/s (2 * N * H * W * Cin * Cout * k^2 per call) and their ratio.
(b) UNet('big') forward + backward under bf16 autocast at 4 and 32 views, native_wgrad = True against False.
Protocol (scripts/bench_unet.py's): every shape warmed up first; the two arms alternate inside one process; a sample
is `--inner` calls between two device events; medians over `--reps` samples. Writes bench_conv.json under --out.

    python scripts/bench_conv.py [--out profiles/conv_wgrad] [--views 4 32] [--reps 15] [--skip-unet]
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
import torch.nn as nn  # noqa: E402

from bench_unet import ab  # noqa: E402


def big_unet(dev):
    from lgm_amd import UNet, preset
    opt = preset("big")
    with torch.device(dev):
        u = UNet(9, 14, down_channels=opt.down_channels, down_attention=opt.down_attention,
                 mid_attention=opt.mid_attention, up_channels=opt.up_channels, up_attention=opt.up_attention)
    return u, opt


def big_sites():
    """(Cin, Cout, H, W, ksize, stride) -> count over the nn.Conv2d sites of one UNet('big') forward (H, W: the input's)."""
    import lgm_amd.unet as U
    sites = {}

    def hook(m, args, out):
        x = args[0]
        key = (m.in_channels, m.out_channels, x.shape[2], x.shape[3], m.kernel_size[0], m.stride[0])
        sites[key] = sites.get(key, 0) + 1

    u, opt = big_unet("meta")
    u.native_wgrad = False  # every conv through its module call, so that the hooks see it
    for m in u.modules():
        if isinstance(m, U.MVAttention):
            m.fused = False  # (meta tensors: shapes only)
        if isinstance(m, nn.Conv2d):
            m.register_forward_hook(hook)
    u(torch.empty(4, 9, opt.input_size, opt.input_size, device="meta"))
    return sites


def bench_shapes(dev, views, reps, inner):
    from lgm_amd.conv import wgrad
    rows, skipped = [], []
    for (Cin, Cout, H, W, k, stride), count in sorted(big_sites().items(), key=lambda kv: (-kv[0][2], kv[0][0], kv[0][1])):
        if stride != 1:
            skipped.append({"Cin": Cin, "Cout": Cout, "H": H, "W": W, "ksize": k, "stride": stride, "sites": count})
            continue
        for N in views:
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn((N, Cin, H, W), device=dev, generator=g).to(torch.bfloat16)
            dy = torch.randn((N, Cout, H, W), device=dev, generator=g).to(torch.bfloat16)
            w = torch.randn((Cout, Cin, k, k), device=dev, generator=g).to(torch.bfloat16)
            p = (k - 1) // 2

            def native():
                return wgrad(dy, x, k, True)

            def stock():
                return torch.ops.aten.convolution_backward(dy, x, w, [Cout], [1, 1], [p, p], [1, 1], False, [0, 0], 1,
                                                           [False, True, True])

            tn, tt = ab(native, stock, reps, inner)
            flop = 2.0 * N * H * W * Cin * Cout * k * k
            rows.append({"Cin": Cin, "Cout": Cout, "H": H, "W": W, "ksize": k, "sites": count, "views": N,
                         "native_us": round(tn, 2), "torch_us": round(tt, 2), "speedup": round(tt / tn, 3),
                         "native_tflops": round(flop / tn * 1e-6, 1), "torch_tflops": round(flop / tt * 1e-6, 1)})
            print(json.dumps(rows[-1]), flush=True)
            del x, dy, w
    return rows, skipped


def bench_unet(dev, views, reps):
    torch.manual_seed(0)
    u, opt = big_unet(dev)
    rows = []
    for N in views:
        x = torch.randn(N, 9, opt.input_size, opt.input_size, device=dev)

        def step(native):
            u.native_wgrad = native
            u.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = u(x)
            y.float().square().mean().backward()

        for native in (True, False):  # warm-up
            step(native)
            step(native)
        torch.cuda.synchronize()
        tn, tt = ab(lambda: step(True), lambda: step(False), reps, 1, warm=0)
        rows.append({"views": N, "native_wgrad_ms": round(tn / 1e3, 3), "torch_wgrad_ms": round(tt / 1e3, 3),
                     "speedup": round(tt / tn, 3)})
        print(json.dumps(rows[-1]), flush=True)
    u.native_wgrad = True
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_wgrad"))
    ap.add_argument("--name", default="bench_conv.json")
    ap.add_argument("--views", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--unet-reps", type=int, default=5)
    ap.add_argument("--skip-unet", action="store_true")
    ap.add_argument("--skip-shapes", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv.py needs a GPU: timings are taken on the device")
    from lgm_amd import build as B
    B.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner}
    if not a.skip_shapes:
        out["shapes"], out["not_taken"] = bench_shapes(dev, a.views, a.reps, a.inner)
    if not a.skip_unet:
        out["unet_big_bf16"] = bench_unet(dev, a.views, a.unet_reps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("shapes", "not_taken", "unet_big_bf16")}))


if __name__ == "__main__":
    main()
