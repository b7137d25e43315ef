"""The native UNet and LGM on the GPU (lgm_amd/unet.py, lgm_amd/models.py), tiny configuration of
tests/golden/unet_tiny.npz: the fused GroupNorm+SiLU path against the recorded reference results and against the same
module with fused = False (torch ops), in fp32 and under bf16 autocast (both against an fp64 CPU run of the same
module), a num_frames = 2 UNet, and LGM.forward end to end."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lgm_amd import LGM, Options, UNet
from lgm_amd import _native as nat
from tests.golden.make_unet_golden import GRAD_PARAMS, TINY
from tests.lgm_ref import lgm_data
from tests.render_cases import rel_l2

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# bf16 autocast: (fused error) / (unfused error), both against fp64, must stay below this. Measured over three seeds
# on an MI355X the largest ratio over all groups was 1.124; the bar is that + 25 %. By construction
# the fused path rounds where torch rounds; the margin is for MIOpen choosing differently on inputs that differ in
# the last bit.
BF16_RATIO_BAR = 1.41
GROUPS = {"conv.weight": lambda k: "conv" in k and k.endswith("weight") or k.endswith("shortcut.weight") or
          k.endswith("sample.weight"),
          "conv.bias": lambda k: ("conv" in k or "shortcut" in k or "sample" in k) and k.endswith("bias"),
          "norm.weight": lambda k: "norm" in k and k.endswith("weight"),
          "norm.bias": lambda k: "norm" in k and k.endswith("bias"),
          "attn.qkv.weight": lambda k: k.endswith("attn.qkv.weight"),
          "attn.proj.weight": lambda k: k.endswith("attn.proj.weight"),
          "attn.proj.bias": lambda k: k.endswith("attn.proj.bias")}


def grouped(named_grads):
    """Parameter gradients concatenated per kind of parameter (every parameter falls in exactly one group)."""
    out = {}
    seen = set()
    for g, pred in GROUPS.items():
        ks = [k for k in named_grads if pred(k) and k not in seen]
        seen.update(ks)
        out[g] = torch.cat([named_grads[k].detach().double().cpu().reshape(-1) for k in ks])
    assert seen == set(named_grads), sorted(set(named_grads) - seen)
    return out


def relv(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def run_unet(u, x, w, autocast=False):
    u.zero_grad()
    xa = x.clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = u(xa)
    else:
        y = u(xa)
    (y.float() * w).sum().backward() if y.dtype != w.dtype else (y * w).sum().backward()
    return y.detach().float(), xa.grad, {k: p.grad.clone() for k, p in u.named_parameters()}


@pytest.fixture(scope="module")
def tiny(cuda):
    z = np.load(os.path.join(GOLDEN, "unet_tiny.npz"))
    torch.manual_seed(0)
    u = UNet(9, 14, **TINY)
    return z, u


def test_tiny_unet_fp32_against_fixture(cuda, tiny):
    z, u_cpu = tiny
    u = copy.deepcopy(u_cpu).to(cuda)
    x, w = torch.from_numpy(z["x"]).to(cuda), torch.from_numpy(z["w"]).to(cuda)
    errs = {}
    prof = nat.KernelProfiler()
    for fused in (True, False):
        u.fused = fused
        with prof:
            y, gx, gp = run_unet(u, x, w)
        ran = prof.summary()
        prof.reset()
        gns = {k for k in ran if k.startswith("k_gns_")}
        assert bool(gns) == fused, sorted(ran)  # the HIP kernels ran, or none of them
        e = {"y": rel_l2(y.cpu().numpy(), z["y"]), "grad_x": rel_l2(gx.cpu().numpy(), z["grad_x"])}
        for k in GRAD_PARAMS:
            e[k] = rel_l2(gp[k].cpu().numpy(), z["grad_" + k])
        errs[fused] = e
    prof.close()
    for k in errs[True]:
        print(f"tiny fp32 {k}: fused {errs[True][k]:.3e} unfused {errs[False][k]:.3e}")
    bad = {k: (errs[True][k], errs[False][k]) for k in errs[True] if not errs[True][k] <= max(1e-5, 2 * errs[False][k])}
    assert not bad, bad


def test_tiny_unet_bf16_autocast_against_fp64(cuda, tiny):
    _, u0 = tiny
    worst = 0.0
    for seed in (0, 1, 2):
        torch.manual_seed(100 + seed)
        u_cpu = UNet(9, 14, **TINY) if seed else copy.deepcopy(u0)
        gen = torch.Generator().manual_seed(seed)
        x, w = torch.randn(8, 9, 16, 16, generator=gen), torch.randn(8, 14, 16, 16, generator=gen)
        u64 = copy.deepcopy(u_cpu).double()
        x64 = x.double().requires_grad_(True)
        y64 = u64(x64)
        (y64 * w.double()).sum().backward()
        ref = {"y": y64.detach(), "grad_x": x64.grad, **grouped({k: p.grad for k, p in u64.named_parameters()})}
        u = copy.deepcopy(u_cpu).to(cuda)
        errs = {}
        for fused in (True, False):
            u.fused = fused
            y, gx, gp = run_unet(u, x.to(cuda), w.to(cuda), autocast=True)
            got = {"y": y, "grad_x": gx, **grouped(gp)}
            errs[fused] = {k: relv(got[k], ref[k]) for k in ref}
        for k in ref:
            r = errs[True][k] / errs[False][k]
            worst = max(worst, r)
            print(f"tiny bf16 seed {seed} {k}: fused {errs[True][k]:.3e} unfused {errs[False][k]:.3e} ratio {r:.3f}")
    print(f"tiny bf16 largest fused / unfused error ratio: {worst:.3f} (bar {BF16_RATIO_BAR})")
    assert worst <= BF16_RATIO_BAR


def test_num_frames_2(cuda):
    torch.manual_seed(4)
    u = UNet(9, 14, num_frames=2, **TINY).to(cuda)
    gen = torch.Generator().manual_seed(4)
    x, w = torch.randn(4, 9, 16, 16, generator=gen).to(cuda), torch.randn(4, 14, 16, 16, generator=gen).to(cuda)
    assert all(m.num_frames == 2 for m in u.modules() if hasattr(m, "num_frames"))
    u.fused = True
    ya, gxa, gpa = run_unet(u, x, w)
    u.fused = False
    yb, gxb, gpb = run_unet(u, x, w)
    # two fp32 evaluations of one function: the fp32 bar of the fixture comparison
    assert relv(ya, yb) < 1e-5 and relv(gxa, gxb) < 1e-5
    ga, gb = grouped(gpa), grouped(gpb)
    for k in ga:
        assert relv(ga[k], gb[k]) < 1e-5, k


def test_lgm_forward_backward(cuda):
    opt = Options(input_size=16, splat_size=16, output_size=32, **TINY)
    torch.manual_seed(0)
    model = LGM(opt).to(cuda)
    data = lgm_data(cuda)
    model.train()
    torch.manual_seed(7)
    res = model(data)
    assert set(res) == {"gaussians", "images_pred", "alphas_pred", "loss", "psnr"}
    assert res["gaussians"].shape == (2, 4 * 16 * 16, 14)
    assert res["images_pred"].shape == (2, 2, 3, 32, 32) and res["alphas_pred"].shape == (2, 2, 1, 32, 32)
    assert torch.isfinite(res["loss"]) and torch.isfinite(res["psnr"])
    res["loss"].backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k

    # the unfused composition: torch GroupNorm / SiLU in the UNet, render without gt_*, then core/models.py:151-153
    def composed(bg):
        model.unet.fused = False
        with torch.no_grad():
            g = model.forward_gaussians(data["input"])
            out = model.gs.render(g, data["cam_view"], data["cam_view_proj"], data["cam_pos"], bg_color=bg)
        model.unet.fused = True
        gt = data["images_output"] * data["masks_output"] + bg.view(1, 1, 3, 1, 1) * (1 - data["masks_output"])
        return out, F.mse_loss(out["image"], gt) + F.mse_loss(out["alpha"], data["masks_output"]), gt

    torch.manual_seed(7)
    bg = torch.rand(3, dtype=torch.float32, device=cuda)  # the draw LGM.forward made in training mode
    out, loss, gt = composed(bg)
    assert abs(float(res["loss"]) - float(loss)) <= 1e-4 * abs(float(loss))
    psnr = -10 * torch.log10(torch.mean((out["image"] - gt) ** 2))
    assert abs(float(res["psnr"]) - float(psnr)) <= 1e-4 * abs(float(psnr))

    # eval: the white background
    model.eval()
    with torch.no_grad():
        res_e = model(data)
    out_w, loss_w, _ = composed(torch.ones(3, device=cuda))
    assert abs(float(res_e["loss"]) - float(loss_w)) <= 1e-4 * abs(float(loss_w))
    assert relv(res_e["images_pred"], out_w["image"]) < 1e-4
    assert abs(float(loss_w) - float(loss)) > 1e-3 * abs(float(loss))  # (the two backgrounds do differ)
