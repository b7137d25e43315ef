"""What LGM_RENDER_ANTIALIAS costs: bench.py's pool (8 scenes) and its single cfg3 scene, fwd+bwd, with the switch
off and on in one process -- step time, per-kernel times (HIP events) and the binned pair counts. bench.py's own
constants, synthetic inputs, warm-up and timing helpers are imported; the flagship line itself does not change.
python scripts/bench_antialias.py [--steps 40] [--warmup 5]  ->  one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from lgm_amd import GaussianRenderer, Options, _native  # noqa: E402
from lgm_amd import dist as D  # noqa: E402
from lgm_amd.cameras import orbit_cameras  # noqa: E402
from lgm_amd.gs import forward_state  # noqa: E402
from lgm_amd.synthetic import synthetic_gaussians, synthetic_upstream_grads  # noqa: E402


def measure(dev, info, B, seed, steps, warmup):
    renderer = GaussianRenderer(Options(output_size=bench.RES))
    tan = float(renderer.tan_half_fov)
    cv, cvp, cp = (t[None].expand(B, *t.shape).contiguous().to(dev) for t in orbit_cameras(bench.VIEWS))
    g = synthetic_gaussians(B, bench.N_GAUSS, seed=seed).to(dev).requires_grad_(True)
    d_img, _, d_alpha, bg = (t.to(dev) for t in synthetic_upstream_grads(B, bench.VIEWS, bench.RES, bench.RES,
                                                                         seed=seed + 1000))
    out = {}
    for aa in (False, True, False, True):  # interleaved: each setting twice
        def step():
            o = renderer.render(g, cv, cvp, cp, bg_color=bg, antialias=aa)
            torch.autograd.backward([o["image"], o["alpha"]], [d_img, d_alpha])
            g.grad = None

        D.warm_up(step, warmup, torch.cuda.synchronize, info, dev)
        el = D.timed_steps(step, steps, info, torch.cuda.synchronize, dev)
        prof = _native.KernelProfiler()
        with prof:
            for _ in range(10):
                step()
            torch.cuda.synchronize()
        kern = {k: round(1e3 * ms / n, 2) for k, (n, ms) in prof.summary().items()}
        prof.close()
        out.setdefault("antialias" if aa else "plain", []).append({"ms_per_step": round(1e3 * el / steps, 4),
                                                                   "kernels_avg_us": kern})
    for aa in (False, True):  # the (Gaussian, tile) pairs the forward bins
        fs = forward_state(g.detach(), cv, cvp, tan, tan, bench.RES, bench.RES, antialias=aa)
        out["pairs_binned_" + ("antialias" if aa else "plain")] = fs["K_binned"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    info = D.rank_info()
    torch.cuda.set_device(info.local)
    dev = torch.device("cuda", info.local)
    res = {"pool": measure(dev, info, bench.POOL_SCENES, bench.POOL_SEED, a.steps, a.warmup),
           "cfg3": measure(dev, info, 1, bench.CFG3_SEED, a.steps, a.warmup)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
