"""What spherical-harmonics colour (LGM_RENDER_SH_MASK) costs: bench.py's pool (8 scenes), forward alone and
forward + backward, at degrees 0..3 in one process -- step time, per-kernel times (HIP events) and the ratios to
degree 0. The rows of degree d are the pool's own Gaussians lifted to SH (DC from their RGB, rest coefficients drawn),
so the geometry, the binning and the tile lists are the same at every degree. bench.py's own constants, synthetic
inputs, warm-up and timing helpers are imported; the flagship line itself does not change.
python scripts/bench_sh.py [--steps 40] [--warmup 5]  ->  one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from lgm_amd import GaussianRenderer, Options, _native  # noqa: E402
from lgm_amd import dist as D  # noqa: E402
from lgm_amd import sh as lsh  # noqa: E402
from lgm_amd.cameras import orbit_cameras  # noqa: E402
from lgm_amd.synthetic import synthetic_gaussians, synthetic_upstream_grads  # noqa: E402

REST_SIGMA = 0.3


def measure(dev, info, B, seed, steps, warmup):
    renderer = GaussianRenderer(Options(output_size=bench.RES))
    cv, cvp, cp = (t[None].expand(B, *t.shape).contiguous().to(dev) for t in orbit_cameras(bench.VIEWS))
    g14 = synthetic_gaussians(B, bench.N_GAUSS, seed=seed)
    d_img, _, d_alpha, bg = (t.to(dev) for t in synthetic_upstream_grads(B, bench.VIEWS, bench.RES, bench.RES,
                                                                         seed=seed + 1000))
    gen = torch.Generator().manual_seed(seed + 2000)
    rows = {}
    for d in range(4):
        g = lsh.rgb_to_sh(g14, d).clone()
        if d:
            g[..., 14:] = REST_SIGMA * torch.randn(g[..., 14:].shape, generator=gen)
        rows[d] = g.to(dev).requires_grad_(True)
    out = {}
    for d in (0, 1, 2, 3, 0, 1, 2, 3):  # interleaved: each degree twice
        g = rows[d]

        def fwd():
            with torch.no_grad():
                renderer.render(g, cv, cvp, cp, bg_color=bg)

        def step():
            o = renderer.render(g, cv, cvp, cp, bg_color=bg)
            torch.autograd.backward([o["image"], o["alpha"]], [d_img, d_alpha])
            g.grad = None

        rec = {}
        for name, fn in (("fwd", fwd), ("fwd_bwd", step)):
            D.warm_up(fn, warmup, torch.cuda.synchronize, info, dev)
            el = D.timed_steps(fn, steps, info, torch.cuda.synchronize, dev)
            rec[name + "_ms"] = round(1e3 * el / steps, 4)
        prof = _native.KernelProfiler()
        with prof:
            for _ in range(10):
                step()
            torch.cuda.synchronize()
        rec["kernels_avg_us"] = {k: round(1e3 * ms / n, 2) for k, (n, ms) in prof.summary().items()}
        prof.close()
        out.setdefault(f"degree{d}", []).append(rec)
    best = {d: {k: min(r[k] for r in out[f"degree{d}"]) for k in ("fwd_ms", "fwd_bwd_ms")} for d in range(4)}
    out["ratio_to_degree0"] = {f"degree{d}": {k: round(best[d][k] / best[0][k], 4) for k in best[d]} for d in (1, 2, 3)}
    # the colour pass's own traffic: B N 3K coefficients read once, B V N colours (12 B) + masks written, read again
    out["sh_bytes"] = {f"degree{d}": B * bench.N_GAUSS * 12 * (d + 1) ** 2 + 2 * B * bench.VIEWS * bench.N_GAUSS * 13
                       for d in (1, 2, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    info = D.rank_info()
    torch.cuda.set_device(info.local)
    dev = torch.device("cuda", info.local)
    print(json.dumps({"pool": measure(dev, info, bench.POOL_SCENES, bench.POOL_SEED, a.steps, a.warmup)}), flush=True)


if __name__ == "__main__":
    main()
