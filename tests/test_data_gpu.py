"""The batch-assembly kernels (include/lgm_data.h, lgm_amd/csrc/data.hip) and lgm_amd/data.py on the GPU.

Truth is the float64 evaluation of the header's formulas in tests/data_ref.py; torch's own composition
(F.interpolate, F.grid_sample, torch.inverse: lgm_amd.data.views_torch / cameras_torch) runs on the same GPU and is
measured next to the kernels. Bar, per output: kernel error <= max(2 x torch's error, 1e-6) relative L2 (1e-6: one
fp32 output rounding and the few fp32 operations before it)."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

from lgm_amd import LGM, Options, data as D
from lgm_amd import _native as nat
from tests.data_ref import cameras64, jitter64, rel, views64
from tests.golden.make_unet_golden import TINY
from tests.test_data_cpu import KEYS, load, seed_all, tail_case

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
FOVY, ZNEAR, ZFAR, RADIUS = 49.1, 0.5, 2.5, 1.5
B, V, VI = 2, 3, 2


def make_src(Hs, Ws, seed=0):
    """uint8 RGBA [B, V, Hs, Ws, 4]; alpha holds 0, 255 and values between (each kind forced in every view)."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (B, V, Hs, Ws, 4), dtype=torch.uint8, generator=gen)
    kind = torch.rand(B, V, Hs, Ws, generator=gen)
    src[..., 3][kind < 0.3] = 0
    src[..., 3][kind > 0.7] = 255
    if Hs * Ws >= 3:
        a = src[..., 3].reshape(B, V, -1)
        a[..., 0], a[..., 1], a[..., 2] = 0, 255, 128
    return src


def make_c2w(nb=B, nv=V):
    """Orbit poses; the first pose of each sample is elevated and rolled about its viewing axis."""
    from lgm_amd.cameras import orbit_camera
    out = np.stack([np.stack([orbit_camera(-20.0 - 11 * b - 9 * v, 33.0 * b + 71 * v + 10, radius=RADIUS)
                              for v in range(nv)]) for b in range(nb)])
    for b in range(nb):
        a = 0.4 + 0.3 * b
        roll = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]], np.float32)
        out[b, 0, :3, :3] = out[b, 0, :3, :3] @ roll
    return torch.from_numpy(out)


def make_knots(h, n, seed=0):
    """knots [B, VI, 2, 17], nknots [[0, n], [2, n]]: view (0, 0) plain, (1, 0) one segment, the others n knots."""
    gen = torch.Generator().manual_seed(seed)
    knots = torch.zeros(B, VI, 2, 17, dtype=torch.int32)
    nknots = torch.tensor([[0, n], [2, n]], dtype=torch.int32)
    for b in range(B):
        for v in range(VI):
            m = int(nknots[b, v])
            if m:
                r = torch.rand(1, 2, m, generator=gen)
                knots[b, v] = D._pack_knots(D._knots_from_uniform(r[:, 0], h, 0.5), D._knots_from_uniform(r[:, 1], h, 0.5))[0]
    return knots, nknots


def check_bar(name, got, torch_got, want):
    ek, et = rel(got.cpu().numpy(), want), rel(torch_got.cpu().numpy(), want)
    print(f"  {name}: kernel {ek:.2e} torch {et:.2e}")
    assert ek <= max(2 * et, FLOOR), (name, ek, et)


CASES = [(16, 16, 8, 12, 9), (8, 8, 12, 12, 10), (10, 14, 7, 5, 8), (1, 1, 4, 4, 8), (32, 32, 16, 16, 17),
         (12, 12, 8, 8, 16)]  # Hs, Ws, h, So, knots; the last: 16 knots on 8 pixels (zero-length segments)


@pytest.mark.parametrize("Hs,Ws,h,So,n", CASES)
def test_views_against_fp64_and_torch(cuda, Hs, Ws, h, So, n):
    src = make_src(Hs, Ws, seed=Hs + h)
    knots, nknots = make_knots(h, n, seed=h)
    if n == 16:
        k = knots[0, 1].long()
        assert (k[:, 1:16] == k[:, :15]).any()  # a zero-length segment is in the case
    pose = D.data_cameras(make_c2w().to(cuda), VI, None, 0.1, RADIUS, FOVY, ZNEAR, ZFAR)[0]
    sd = src.to(cuda)
    prof = nat.KernelProfiler()
    with prof:
        out = D.data_views(sd, pose, knots, nknots, FOVY, VI, h, So)
    assert set(prof.summary()) == {"k_data_in", "k_data_out"}
    prof.close()
    src32 = src.float() / 255
    want = views64(src32.numpy(), False, pose.cpu().numpy(), knots.numpy(), nknots.numpy(), FOVY, VI, h, So)
    ref = D.views_torch(sd, pose, knots, nknots, FOVY, VI, h, So)
    print(f"views {Hs}x{Ws} -> h {h}, So {So}, {n} knots")
    for name, a, t, w in zip(("input", "images_output", "masks_output"), out, ref, want):
        assert a.shape == t.shape == w.shape and a.dtype == torch.float32
        check_bar(name, a, t, w)
    check_bar("input[:, :, :3]", out[0][:, :, :3], ref[0][:, :, :3], want[0][:, :, :3])
    check_bar("input[:, :, 3:]", out[0][:, :, 3:], ref[0][:, :, 3:], want[0][:, :, 3:])

    def same(x, y):
        return all(torch.equal(p, q) for p, q in zip(x, y))

    # two calls; the f32 path on u8 / 255; BGRA texels with swap_rb against the swapped source
    assert same(out, D.data_views(sd, pose, knots, nknots, FOVY, VI, h, So))
    assert same(out, D.data_views(src32.to(cuda), pose, knots, nknots, FOVY, VI, h, So))
    assert same(out, D.data_views(sd[..., [2, 1, 0, 3]].contiguous(), pose, knots, nknots, FOVY, VI, h, So,
                                  swap_rb=True))
    # views with nknots = 0 equal a call without knots, bitwise (all of a call with every count 0)
    plain = D.data_views(sd, pose, None, None, FOVY, VI, h, So)
    assert torch.equal(out[0][0, 0], plain[0][0, 0])
    assert same(plain, D.data_views(sd, pose, knots, torch.zeros_like(nknots), FOVY, VI, h, So))
    assert not torch.equal(out[0][0, 1, :3], plain[0][0, 1, :3]) or h <= 4


def test_u8_conversion_is_the_true_division(cuda):
    """All 256 byte values through a 1 : 1 resize: masks_output is a / 255 and, on opaque texels, images_output is
    rgb / 255, bit for bit torch's fp32 division."""
    ramp = torch.arange(256, dtype=torch.uint8).reshape(16, 16)
    src = torch.stack([ramp, ramp.flip(0), ramp.t(), ramp], -1)[None, None].contiguous()  # alpha: every value
    opaque = src.clone()
    opaque[..., 3] = 255
    for s in (src, opaque):
        _, img, msk = D.data_views(s.to(cuda), None, None, None, FOVY, 1, 4, 16, want_input=False)
        x = (s.float() / 255).permute(0, 1, 4, 2, 3)
        assert torch.equal(msk.cpu(), x[:, :, 3:4])
        if s is opaque:
            assert torch.equal(img.cpu(), x[:, :, :3])


def test_cameras_against_fp64_and_torch(cuda):
    c2w = make_c2w()
    gen = torch.Generator().manual_seed(2)
    jit = torch.rand(B, VI, 2, generator=gen) * 2 - 1
    got = dict(zip(("pose_in", "cam_view", "cam_view_proj", "cam_pos", "c2w_colmap"),
                   D.data_cameras(c2w.to(cuda), VI, jit, 0.1, RADIUS, FOVY, ZNEAR, ZFAR)))
    ref = dict(zip(("pose_in", "cam_view", "cam_view_proj", "cam_pos", "c2w_colmap"),
                   D.cameras_torch(c2w.to(cuda), VI, jit, 0.1, RADIUS, FOVY, ZNEAR, ZFAR)))
    want = cameras64(c2w.numpy(), VI, jit.numpy(), 0.1, RADIUS, FOVY, ZNEAR, ZFAR)
    for k in got:
        # the fp64 recipe rounds the normalised pose to fp32 once (the header); torch's is measured against the same
        check_bar(k, got[k], ref[k], want[k])
    assert rel(got["c2w_colmap"].cpu().numpy(), want["P"][:, :VI] * np.array([1, -1, -1, 1])) <= FLOOR
    # identity jitter returns the pose bitwise
    plain = D.data_cameras(c2w.to(cuda), VI, None, 0.1, RADIUS, FOVY, ZNEAR, ZFAR)
    zero = D.data_cameras(c2w.to(cuda), VI, torch.zeros(B, VI, 2), 0.1, RADIUS, FOVY, ZNEAR, ZFAR)
    assert all(torch.equal(a, b) for a, b in zip(plain, zero))
    assert not torch.equal(plain[0], got["pose_in"]) and all(torch.equal(a, got[k]) for a, k in
                                                             zip(plain[1:], ("cam_view", "cam_view_proj", "cam_pos",
                                                                             "c2w_colmap")))
    # view 0 (elevated, rolled) lands at the identity rotation and (0, 0, cam_radius)
    p0 = plain[0][:, 0].cpu().double()
    want0 = torch.eye(4, dtype=torch.float64)
    want0[2, 3] = RADIUS
    assert (p0 - want0).abs().max() <= 1e-6, (p0 - want0).abs().max()
    # cam_view c2w'^T = I, all views (Vi = V gives every c2w')
    full = D.data_cameras(c2w.to(cuda), V, None, 0.1, RADIUS, FOVY, ZNEAR, ZFAR)
    prod = full[1].cpu().double() @ full[4].cpu().double().transpose(2, 3)
    assert (prod - torch.eye(4, dtype=torch.float64)).abs().max() <= 1e-6
    assert torch.equal(full[3], -full[4][:, :, :3, 3])


def test_drop_ins_on_gpu(cuda):
    # get_rays / plucker_rays
    g = load("data_rays.npz")
    poses = torch.from_numpy(g["poses"]).to(cuda)
    for h in (8, 12):
        for i in range(2):
            o, d = D.get_rays(poses[i], h, h, float(g["fovy"]))
            assert o.is_cuda and d.is_cuda
            assert rel(o.cpu().numpy(), g[f"o_h{h}_{i}"]) <= 1e-5 and rel(d.cpu().numpy(), g[f"d_h{h}_{i}"]) <= 1e-5
    # grid_distortion: the draws are host draws, the same on both devices
    g = load("data_distort.npz")
    for tag in ("a", "b"):
        seed_all(g[f"seed_{tag}"])
        prof = nat.KernelProfiler()
        with prof:
            out = D.grid_distortion(torch.from_numpy(g[f"images_{tag}"]).to(cuda))
        assert set(prof.summary()) == {"k_data_in"}
        prof.close()
        assert out.is_cuda and rel(out.cpu().numpy(), g[f"out_{tag}"]) <= 1e-5
    with pytest.raises(nat.NativeError):
        D.grid_distortion(torch.zeros(1, 4, 8, 8, device=cuda))
    # orbit_camera_jitter draws on the poses' device: replay its draws
    g = load("data_jitter.npz")
    poses = torch.from_numpy(g["poses"]).to(cuda)
    torch.manual_seed(5)
    out = D.orbit_camera_jitter(poses)
    torch.manual_seed(5)
    u = torch.cat([torch.rand(3, 1, device=cuda) * 2 - 1, torch.rand(3, 1, device=cuda) * 2 - 1], 1).cpu().numpy()
    want = np.stack([jitter64(g["poses"][i], u[i], 0.1) for i in range(3)])
    assert rel(out.cpu().numpy(), want) <= FLOOR
    assert torch.equal(D.orbit_camera_jitter(poses, strength=0.0), poses)


def test_build_batch_against_fixture_and_cpu_path(cuda):
    opt, bgra, c2w, aug, g = tail_case()
    prof = nat.KernelProfiler()
    with prof:
        data = D.build_batch(opt, bgra.to(cuda), c2w.to(cuda), True, augmentation=aug, swap_rb=True)
    assert set(prof.summary()) == {"k_data_cameras", "k_data_in", "k_data_out"}
    prof.close()
    assert set(data) == set(KEYS)
    for k in KEYS:
        e = rel(data[k][0].cpu().numpy(), g[k])
        print(f"  tail {k}: relL2 {e:.2e}")
        assert data[k].is_cuda and e <= 1e-5, (k, e)
    # its own random stream: the same generator state gives the same batch on both devices
    opt = Options(input_size=8, output_size=12, num_views=V, num_input_views=VI, prob_grid_distortion=1.0,
                  prob_cam_jitter=1.0)
    src, poses = make_src(10, 14), make_c2w()
    on_gpu = D.build_batch(opt, src.to(cuda), poses.to(cuda), True, torch.Generator().manual_seed(9))
    on_cpu = D.build_batch(opt, src, poses, True, torch.Generator().manual_seed(9))
    plain = D.build_batch(opt, src.to(cuda), poses.to(cuda), False)
    for k in KEYS:
        e = rel(on_gpu[k].cpu().numpy(), on_cpu[k].numpy())
        print(f"  gpu vs cpu {k}: relL2 {e:.2e}")
        assert e <= 1e-5, (k, e)
    assert not torch.equal(on_gpu["input"][:, 1], plain["input"][:, 1])
    assert torch.equal(on_gpu["input"][:, 0], plain["input"][:, 0])  # view 0 is never augmented
    again = D.build_batch(opt, src.to(cuda), poses.to(cuda), False)
    assert all(torch.equal(plain[k], again[k]) for k in KEYS)


def test_lgm_takes_the_gpu_batch(cuda):
    """A tiny LGM (lambda_lpips = 0) on the kernels' batch and on the torch-composed one: same loss, backward runs."""
    opt = Options(input_size=16, splat_size=16, output_size=32, num_views=6, num_input_views=4, **TINY)
    torch.manual_seed(0)
    model = LGM(opt).to(cuda).eval()
    gen = torch.Generator().manual_seed(4)
    src = torch.randint(0, 256, (2, 6, 24, 24, 4), dtype=torch.uint8, generator=gen)
    yy, xx = torch.meshgrid(torch.arange(24), torch.arange(24), indexing="ij")
    src[..., 3] = (((yy - 12) ** 2 + (xx - 12) ** 2) < 81).to(torch.uint8) * 255  # an opaque disc
    c2w = make_c2w(2, 6)
    aug = D.draw_augmentation(dataclasses.replace(opt, prob_grid_distortion=1.0, prob_cam_jitter=1.0), 2,
                              torch.Generator().manual_seed(6))
    res = {}
    for name, fn in (("kernels", lambda: D.build_batch(opt, src.to(cuda), c2w.to(cuda), True, augmentation=aug)),
                     ("torch", lambda: D.build_batch_torch(opt, src.to(cuda), c2w.to(cuda), aug))):
        data = fn()
        model.zero_grad()
        out = model(data)
        out["loss"].backward()
        assert math.isfinite(out["loss"].item()) and math.isfinite(out["psnr"].item())
        assert model.conv.weight.grad is not None and bool(torch.isfinite(model.conv.weight.grad).all())
        res[name] = out["loss"].item()
    print(f"  LGM loss on the kernels' batch {res['kernels']:.7f}, on torch's {res['torch']:.7f}")
    assert abs(res["kernels"] - res["torch"]) <= 1e-5 * abs(res["torch"])


def test_errors_are_reported_not_launched(cuda):
    L = nat.lib()
    p = nat.ptr
    src = make_src(8, 8).to(cuda)
    pose = torch.eye(4, device=cuda).expand(B, VI, 4, 4).contiguous()
    knots, nknots = make_knots(8, 9)
    kd = knots.to(cuda)
    inp, img, msk = (torch.empty(B, VI, 9, 8, 8, device=cuda), torch.empty(B, V, 3, 8, 8, device=cuda),
                     torch.empty(B, V, 1, 8, 8, device=cuda))
    c2w = make_c2w().to(cuda)
    cam = [torch.empty(B, V, 4, 4, device=cuda) for _ in range(4)]
    st = nat.stream_of(cuda)

    def nk(t):
        return ctypes.c_void_p(t.data_ptr())

    def views(dt=nat.DATA_U8, Vi=VI, h=8, s=src, counts=nknots):
        return L.lgm_data_views(dt, 0, B, V, Vi, 8, 8, h, 8, p(s) if s is not None else None, p(pose), p(kd),
                                nk(counts), FOVY, p(inp), p(img), p(msk), st, nat.diag())

    prof = nat.KernelProfiler()
    with prof:
        for bad in (dict(Vi=V + 1), dict(h=0), dict(h=-3), dict(s=None), dict(dt=7), dict(dt=1),
                    dict(counts=torch.tensor([[0, 1], [2, 9]], dtype=torch.int32)),
                    dict(counts=torch.tensor([[0, 9], [18, 9]], dtype=torch.int32)),
                    dict(counts=torch.tensor([[-1, 9], [2, 9]], dtype=torch.int32))):
            rc = views(**bad)
            assert rc < 0 and L.lgm_last_error(), bad
        rc = L.lgm_data_views(nat.DATA_U8, 0, B, V, VI, 8, 8, 8, 8, p(src), None, None, None, FOVY, p(inp), p(img),
                              p(msk), st, nat.diag())
        assert rc < 0 and b"null" in L.lgm_last_error()  # input without pose_in
        rc = L.lgm_data_views(nat.DATA_U8, 0, B, V, VI, 8, 8, 8, 8, p(src), p(pose), None, None, FOVY, p(inp), p(img),
                              None, st, nat.diag())
        assert rc < 0  # images_output without masks_output

        def cameras(Vi=VI, c=c2w, out0=cam[0], fovy=FOVY):
            return L.lgm_data_cameras(B, V, Vi, p(c) if c is not None else None, None, 0.1, RADIUS, fovy, ZNEAR, ZFAR,
                                      p(out0) if out0 is not None else None, p(cam[1]), p(cam[2]), p(cam[3]), None, st,
                                      nat.diag())
        for bad in (dict(Vi=V + 1), dict(Vi=0), dict(c=None), dict(out0=None), dict(fovy=0.0)):
            rc = cameras(**bad)
            assert rc < 0 and L.lgm_last_error(), bad
        assert not prof.summary()
        assert views() == 0 and cameras() == 0
        assert set(prof.summary()) == {"k_data_in", "k_data_out", "k_data_cameras"}
    prof.close()
