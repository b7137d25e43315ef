"""Golden data for tests/test_data_cpu.py and tests/test_data_gpu.py, recorded with a checkout of the reference LGM at
hand: its get_rays, grid_distortion and orbit_camera_jitter (core/utils.py) are imported here and never stored; the
files hold seeds, inputs and recorded results only.

  data_rays.npz     get_rays of two poses at h = 8 and 12 (fovy 49.1): rays_o, rays_d.
  data_distort.npz  grid_distortion of [3, 3, 12, 12] and [2, 3, 24, 24] images under np.random.seed(s) and
                    torch.manual_seed(s): seed, images, result, and the knots the seed gives.
  data_jitter.npz   orbit_camera_jitter of three poses under torch.manual_seed(s): seed, poses, result, the numbers u.
  data_tail.npz     the provider's tail (core/provider_lvis.py:141-213, composed here from torch ops and the three
                    reference functions) for one sample: V = 5 BGRA uint8 views of 16 x 16, Vi = 3, h = 8, So = 12,
                    distortion and jitter on: inputs, the draws (knots, jitter numbers) and every result.

`roma` and `kiui` need not be installed: small stand-in modules (kiui.op.safe_normalize; roma.rotvec_to_rotmat by
Rodrigues' formula), written here, are registered before the import when the real ones are missing. The metadata of
data_jitter.npz and data_tail.npz says so: those fixtures rest on the stand-in Rodrigues.

Every recipe is also evaluated in float64 (tests/data_ref.py) and the reference's float32 result must lie within 2e-6
relative L2 of it, so that the 1e-5 bars of the tests have room; a seed that fails this is replaced.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_data_golden.py --reference LGM_CHECKOUT
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FOVY, ZNEAR, ZFAR, RADIUS = 49.1, 0.5, 2.5, 1.5
FLOOR = 2e-6
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def register_stand_ins():
    """kiui.op.safe_normalize and roma.rotvec_to_rotmat when the packages are missing. Returns the names stood in."""
    stood = []
    try:
        importlib.import_module("kiui.op")
    except ImportError:
        def safe_normalize(x, eps=1e-20):
            return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))
        kiui, op = types.ModuleType("kiui"), types.ModuleType("kiui.op")
        op.safe_normalize = safe_normalize
        kiui.op = op
        sys.modules["kiui"], sys.modules["kiui.op"] = kiui, op
        stood.append("kiui.op.safe_normalize")
    try:
        importlib.import_module("roma")
    except ImportError:
        def rotvec_to_rotmat(r):
            th = r.norm(dim=-1, keepdim=True).clamp_min(1e-12)[..., None]
            k = r / th[..., 0]
            K = torch.zeros(*r.shape[:-1], 3, 3, dtype=r.dtype, device=r.device)
            K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
            K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
            return torch.eye(3, dtype=r.dtype, device=r.device) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)
        roma = types.ModuleType("roma")
        roma.rotvec_to_rotmat = rotvec_to_rotmat
        sys.modules["roma"] = roma
        stood.append("roma.rotvec_to_rotmat")
    return stood


def seed_all(s):
    np.random.seed(s)
    torch.manual_seed(s)


def poses(n, radius=RADIUS):
    from lgm_amd.cameras import orbit_camera
    return torch.from_numpy(np.stack([orbit_camera(-8.0 - 7 * i, 25.0 + 67 * i, radius=radius) for i in range(n)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference LGM (its core/utils.py)")
    a = ap.parse_args()
    sys.dont_write_bytecode = True  # the reference checkout is read-only
    stood = register_stand_ins()
    sys.path.insert(0, a.reference)
    from core.utils import get_rays, grid_distortion, orbit_camera_jitter  # noqa: E402  (imported, never stored)

    from lgm_amd.data import sample_grid_knots
    from tests import data_ref as R
    meta = "stand-ins: " + (", ".join(stood) or "none")

    def check(name, got, want):
        e = R.rel(got, want)
        print(f"  {name}: reference fp32 vs fp64 recipe relL2 = {e:.2e}")
        assert e <= FLOOR, (name, e)

    # rays
    P = poses(2)
    out = {"poses": P.numpy(), "fovy": np.float64(FOVY), "meta": np.array(meta)}
    for h in (8, 12):
        for i in range(2):
            o, d = get_rays(P[i], h, h, FOVY)
            out[f"o_h{h}_{i}"], out[f"d_h{h}_{i}"] = o.numpy(), d.numpy()
            o64, d64 = R.rays64(P[i].numpy(), h, FOVY)
            check(f"rays h={h} pose {i}", np.concatenate([o.numpy(), d.numpy()], -1), np.concatenate([o64, d64], -1))
    np.savez_compressed(os.path.join(HERE, "data_rays.npz"), **out)

    # distortion
    out = {"meta": np.array(meta)}
    for tag, shape, seed in (("a", (3, 3, 12, 12), 11), ("b", (2, 3, 24, 24), 12)):
        img = torch.rand(*shape, generator=torch.Generator().manual_seed(seed + 100))
        seed_all(seed)
        res = grid_distortion(img.clone())
        seed_all(seed)
        knots, n = sample_grid_knots(shape[0], shape[2], shape[3])
        want = np.stack([R.warp64(img[b].double().numpy(), knots[b, 0].numpy(), knots[b, 1].numpy(), n)
                         for b in range(shape[0])])
        check(f"distortion {shape} ({n} knots)", res.numpy(), want)
        out.update({f"seed_{tag}": np.int64(seed), f"images_{tag}": img.numpy(), f"out_{tag}": res.numpy(),
                    f"knots_{tag}": knots.numpy(), f"n_{tag}": np.int64(n)})
    np.savez_compressed(os.path.join(HERE, "data_distort.npz"), **out)

    # jitter
    P = poses(3)
    seed = 21
    seed_all(seed)
    res = orbit_camera_jitter(P.clone())
    seed_all(seed)
    u = torch.cat([torch.rand(3, 1) * 2 - 1, torch.rand(3, 1) * 2 - 1], 1)
    want = np.stack([R.jitter64(P[i].numpy(), u[i].numpy(), 0.1) for i in range(3)])
    check("jitter", res.numpy(), want)
    np.savez_compressed(os.path.join(HERE, "data_jitter.npz"), seed=np.int64(seed), poses=P.numpy(), out=res.numpy(),
                        u=u.numpy(), meta=np.array(meta))

    # the provider's tail for one sample
    V, Vi, Hs, h, So, seed = 5, 3, 16, 8, 12, 31
    gen = torch.Generator().manual_seed(seed + 100)
    bgra = torch.randint(0, 256, (V, Hs, Hs, 4), dtype=torch.uint8, generator=gen)
    bgra[..., 3][torch.rand(V, Hs, Hs, generator=gen) < 0.25] = 0  # alpha: 0, 255 and values between
    bgra[..., 3][torch.rand(V, Hs, Hs, generator=gen) < 0.25] = 255
    c2w = poses(V, radius=1.5)
    c2w[:, :3, 3] *= RADIUS / 1.5
    x = (torch.from_numpy(bgra.numpy().astype(np.float32) / 255)).permute(0, 3, 1, 2)  # [V, 4, Hs, Hs]
    masks = x[:, 3:4]
    images = (x[:, :3] * masks + (1 - masks))[:, [2, 1, 0]].contiguous()  # white background, bgr -> rgb
    T = torch.eye(4)
    T[2, 3] = RADIUS
    cam = (T @ torch.inverse(c2w[0])).unsqueeze(0) @ c2w
    img_in = F.interpolate(images[:Vi].clone(), size=(h, h), mode="bilinear", align_corners=False)
    cam_in = cam[:Vi].clone()
    seed_all(seed)
    img_in[1:] = grid_distortion(img_in[1:])
    cam_in[1:] = orbit_camera_jitter(cam_in[1:])
    img_in = (img_in - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    images_output = F.interpolate(images, size=(So, So), mode="bilinear", align_corners=False)
    masks_output = F.interpolate(masks, size=(So, So), mode="bilinear", align_corners=False)
    rays = []
    for i in range(Vi):
        o, d = get_rays(cam_in[i], h, h, FOVY)
        rays.append(torch.cat([torch.cross(o, d, dim=-1), d], dim=-1))
    inp = torch.cat([img_in, torch.stack(rays).permute(0, 3, 1, 2)], dim=1)
    cam[:, :3, 1:3] *= -1
    from lgm_amd.cameras import projection_matrix
    cam_view = torch.inverse(cam).transpose(1, 2)
    res = {"input": inp, "images_output": images_output, "masks_output": masks_output, "cam_view": cam_view,
           "cam_view_proj": cam_view @ projection_matrix(FOVY, ZNEAR, ZFAR), "cam_pos": -cam[:, :3, 3],
           "c2w_colmap": cam[:Vi].clone()}
    # the draws, replayed
    seed_all(seed)
    k, n = sample_grid_knots(Vi - 1, h, h)
    knots = torch.zeros(Vi, 2, 17, dtype=torch.int32)
    knots[1:] = k
    nknots = torch.tensor([0] + [n] * (Vi - 1), dtype=torch.int32)
    jit = torch.zeros(Vi, 2)
    jit[1:] = torch.cat([torch.rand(Vi - 1, 1) * 2 - 1, torch.rand(Vi - 1, 1) * 2 - 1], 1)
    c64 = R.cameras64(c2w[None].numpy(), Vi, jit[None].numpy(), 0.1, RADIUS, FOVY, ZNEAR, ZFAR)
    i64, o64, m64 = R.views64(x.permute(0, 2, 3, 1)[None].numpy(), True, c64["pose_in"], knots[None].numpy(),
                              nknots[None].numpy(), FOVY, Vi, h, So)
    want = dict(c64, input=i64, images_output=o64, masks_output=m64)
    for key, val in res.items():
        check(f"tail {key}", val.numpy(), want[key][0])
    np.savez_compressed(os.path.join(HERE, "data_tail.npz"), seed=np.int64(seed), bgra=bgra.numpy(), c2w=c2w.numpy(),
                        knots=knots.numpy(), nknots=nknots.numpy(), jitter=jit.numpy(),
                        sizes=np.array([V, Vi, Hs, h, So]), params=np.array([FOVY, ZNEAR, ZFAR, RADIUS]),
                        meta=np.array(meta), **{k: v.numpy() for k, v in res.items()})
    print("written; " + meta)


if __name__ == "__main__":
    main()
