"""Golden vectors for tests/test_cfg1_cpu.py, recorded with a checkout of the reference LGM at hand (its code is
imported here and never stored): the output of the reference's own UNet('big') (core/unet.py, its fallback
attention, XFORMERS_DISABLED=1; fp32, CPU, torch.manual_seed(0) before construction) on the four catstatue views
of scripts/cfg1_cpu.load_views, and what only a run with that UNet can establish -- that scripts/cfg1_cpu.py's copy
with lgm_amd's MVAttention swapped into all 16 blocks (same seed, so the same weights) returns the same tensor:
the number of swapped blocks and the relative L2 distance of the two outputs. A strided sample of the input views is
kept too, so the test pins load_views to the input these outputs belong to.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cfg1_golden.py --reference LGM_CHECKOUT
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
INPUT_SAMPLE = 8192


def sample_indices(size, n=INPUT_SAMPLE):
    """The strided sample of a flattened array that the fixture keeps of the input views (shared with the test)."""
    return (np.arange(min(n, size), dtype=np.int64) * 7919 + 13) % size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference LGM (its core/unet.py)")
    a = ap.parse_args()
    import cfg1_cpu as H
    png = os.path.join(HERE, "catstatue_rgba.png")
    torch.manual_seed(0)
    swapped, n = H.build_big_unet(a.reference)
    from core.unet import UNet  # noqa: E402  (reference code, read-only)
    torch.manual_seed(0)
    ref = UNet(9, 14, **H.BIG)
    swapped.eval()
    ref.eval()
    views = H.load_views(png)
    x = views.view(4, 9, H.INPUT_SIZE, H.INPUT_SIZE)
    with torch.no_grad():
        ya, yb = swapped(x).numpy().astype(np.float64), ref(x).numpy()
    rel = float(np.linalg.norm(ya - yb) / np.linalg.norm(yb.astype(np.float64)))
    flat = views.numpy().reshape(-1)
    # one file per view ([14, 128, 128] fp32 each): the whole [4, 14, 128, 128] output is 3.7 MB
    for v in range(yb.shape[0]):
        np.savez_compressed(os.path.join(HERE, f"cfg1_unet_big_v{v}.npz"), unet_out=yb[v].astype(np.float32))
    np.savez_compressed(os.path.join(HERE, "cfg1_unet_big.npz"), n_views=np.int64(yb.shape[0]),
                        swapped_mvattention_blocks=np.int64(n), swapped_vs_reference_rel_l2=np.float64(rel),
                        views_shape=np.array(views.shape, np.int64), views_sample=flat[sample_indices(flat.size)])
    print("swapped", n, "rel_l2", rel, "unet_out", yb.shape)


if __name__ == "__main__":
    main()
