"""A whole LGM training iteration at flash-attention widths (tests/lgm_ref.py MID: 46.9 M parameters, six
MVAttention blocks at C = 512 / head dim 32 on 256 tokens) against a staged float64 reference.

* float64 chain (tests/lgm_ref.py fp64_chain): float64 model on the CPU -> float64 oracle render -> LGM's MSE terms in
  torch -> the oracle's analytic backward -> the float64 model's backward. The same chain in fp32 on the CPU lies
  0.6e-5 to 1.5e-5 (every parameter group) from it: the inputs are well conditioned (test 1 pins that).
* fp32 on the GPU is compared end to end (test 2): loss, Gaussians, d_gaussians, every parameter group; next to it
  the same model as upstream's torch composition (`stock`) on the same GPU.
* under bf16 autocast the end-to-end gradient is NOT a usable observable: on the CPU (stock torch ops, three seeds) the
  bf16 Gaussians are 6.5e-3 from float64 and every parameter group then ends up 9e-2 to 1.7e-1 away, all groups
  together, because the render gradient is that sensitive to the Gaussians' perturbation; a 1 % kernel error would hide
  under it. So bf16 is cut at the Gaussians: the UNet + head stage differentiated at the float64 chain's d_gaussians
  (a fixed, realistic, sparse and heavy-tailed seed: the stage is linear in it), as native error / stock error per
  group (test 3), and the render stage of LGM.forward against the oracle at the Gaussians the head handed it (test 4).
* two whole steps -- batch assembly, bf16 forward with LPIPS, backward, clip + AdamW under OneCycleLR -- with the
  optimizer held to float64 AdamW fed the very gradients the backward produced (test 5).
The measured errors go to tests/render_cases.PRECISION, which the session writes out as grad_precision.json
(tests/conftest.py).
"""
import contextlib
import copy
import dataclasses

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import OneCycleLR

from lgm_amd import LGM
from lgm_amd import _native as nat
from tests.lgm_ref import (RENDER_GROUPS, fp64_chain, grouped, lgm_data, mid_options, oracle_step, rel, relf, stock)
from tests.render_cases import PRECISION, grad_bar

SEEDS = (0, 1, 2)
BG_CPU = np.array([0.25, 0.5, 0.75])  # (fp32-exact: the fp32 and the float64 chain see one background)
FP32_BAR = 1e-4  # the project's fp32 bar (tests/test_training_gpu.py, tests/test_unet_gpu.py)
# bf16 autocast, UNet + head stage of MID: (native error) / (stock error), both against float64, largest over the
# Gaussians, d_input, every parameter group and the three seeds. Measured on an MI355X in six runs,
# largest ratio of seed 0 | 1 | 2: 1.018 | 1.018 | 1.349, 0.990 | 0.960 | 1.108, 1.058 | 1.240 | 1.142,
# 1.038 | 1.012 | 1.093, 1.337 | 1.260 | 0.998, 1.039 | 1.066 | 1.020. Both arms differ between runs (torch's library
# kernels are not run-to-run reproducible here). Every group but the head's two stays within 0.86 - 1.07
# (head.conv.bias: 0.04 - 0.11, the head kernel sums it in fp32 where torch's conv rounds to bf16), and every value
# above 1.07 is head.conv.weight: 196 elements whose
# error (1.2e-2 - 2.1e-2 in either arm) is that of the bf16 UNet output it is a sum over, so the ratio of the two arms'
# errors moves by +-30 % with the last bits of that output. The bar is the largest measured ratio + 25 %, as
# tests/test_unet_gpu.py BF16_RATIO_BAR was set.
BF16_STAGE_RATIO_BAR = 1.69


def make_model(seed):
    torch.manual_seed(seed)
    return LGM(mid_options())


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """(seed, bg) -> (the CPU model, the float64 chain of its iteration on lgm_data(B=1, seed)), computed once."""
    models, chains = {}, {}

    def get(seed, bg=BG_CPU):
        key = (seed, tuple(float(v) for v in bg))
        if seed not in models:
            models[seed] = make_model(seed)
        if key not in chains:
            r = fp64_chain(models[seed], lgm_data("cpu", B=1, seed=seed), np.asarray(bg, np.float64), oracle_mod)
            r["groups"] = grouped(r["grads"])
            chains[key] = r
        return models[seed], chains[key]

    yield get
    models.clear()
    chains.clear()


def render_group_errors(got, want):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().double().cpu().numpy() if isinstance(want, torch.Tensor) else want
    return {n: rel(got[..., sl], want[..., sl]) for n, sl in RENDER_GROUPS.items()}


def launched(prof):
    return {k: n for k, (n, _) in prof.summary().items()}


def has(ran, prefix):
    return any(k.startswith(prefix) for k in ran)


# ---- 1. the reference is well conditioned (CPU)
def test_fp32_cpu_chain_against_fp64(oracle_mod, refs):
    """The fp32 CPU chain against the float64 chain on MID: loss <= 1e-6 relative, every parameter group <= 1e-4
    (measured 0.6e-5 to 1.5e-5), the same pair count, no pixel near a clamp bound (asserted by both chains). That keeps
    the inputs, not only the kernels, inside the bars of the GPU tests below."""
    from tests.test_training_gpu import _oracle_seeds
    model, r64 = refs(0)
    data = lgm_data("cpu", B=1, seed=0)
    r32 = fp64_chain(model, data, BG_CPU, oracle_mod, precision=torch.float32)
    g32 = grouped(r32["grads"])
    errs = {k: rel(g32[k], r64["groups"][k]) for k in r64["groups"]}
    e_loss, e_g = relf(r32["loss"], r64["loss"]), rel(r32["gaussians"], r64["gaussians"])
    print(f"cpu fp32 chain vs fp64: loss {e_loss:.2e} gaussians {e_g:.2e} K {r32['K']} / {r64['K']} "
          f"mean alpha {r64['alpha'].mean():.3f}")
    for k, e in errs.items():
        print(f"  {k}: {e:.3e}")
    PRECISION.append({"test": "lgm_step MID: fp32 CPU chain vs fp64 chain", "loss": e_loss, "gaussians": e_g,
                      "K": r64["K"], "groups": errs})
    # what autograd fed the oracle's backward is the seed pair the render tests state in numpy
    S = data["images_output"].shape[-1]
    n_a = float(data["masks_output"].numel())
    d_img, d_alpha, _ = _oracle_seeds({"image": r64["raw_image"], "alpha": r64["alpha"]},
                                      data["images_output"].double().numpy(), data["masks_output"].double().numpy(),
                                      BG_CPU, 3.0 * n_a, n_a)
    assert rel(r64["rec"]["d_image"], d_img) < 1e-12 and rel(r64["rec"]["d_alpha"], d_alpha) < 1e-12 and S == 32
    assert r64["alpha"].mean() > 0.1 and r64["K"] > 1000  # the scene is visible
    assert r32["K"] == r64["K"]
    assert e_loss <= 1e-6
    assert all(e <= FP32_BAR for e in errs.values()), errs


# ---- 2. fp32 on the GPU, end to end
@pytest.mark.gpu
def test_fp32_end_to_end(cuda, oracle_mod, refs):
    """LGM(MID).train() forward + backward in fp32: loss and psnr (1e-5), Gaussians (1e-5 per render group),
    gaussians.grad (grad_bar per render group), every parameter group within max(1e-4, 2 x the stock composition's
    error on the same GPU) of the float64 chain (2 x: what test_tiny_unet_fp32_against_fixture allows between two
    fp32 orders), and the kernels that must and must not have run in each arm."""
    torch.manual_seed(7)
    bg = torch.rand(3, dtype=torch.float32, device=cuda)  # the draw LGM.forward makes in training mode
    cpu_model, ref = refs(0, bg.cpu().numpy())
    model = copy.deepcopy(cpu_model).to(cuda).train()
    data = lgm_data(cuda, B=1, seed=0)
    prof = nat.KernelProfiler()

    def arm():
        model.zero_grad()
        torch.manual_seed(7)
        prof.reset()
        with prof:
            res = model(data)
            res["gaussians"].retain_grad()
            res["loss"].backward()
            torch.cuda.synchronize()
        named = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}
        return res, grouped(named), launched(prof), named

    res, got, ran, named = arm()
    with stock(model):
        res_s, got_s, ran_s, named_s = arm()
    prof.close()
    for k in ("k_attn_fwd", "k_attn_delta", "k_attn_dq", "k_attn_dkdv", "k_mva_gn_", "k_mva_out", "k_gns_",
              "k_head_fwd", "k_head_bwd", "k_render_fwd", "k_render_bwd", "k_preproc_bwd"):
        assert has(ran, k), (k, sorted(ran))
    assert ran["k_attn_fwd"] == 6 and "k_mva_out_bwd" in ran
    assert not has(ran, "k_wgrad") and not has(ran, "k_conv_wgrad"), sorted(ran)
    for k in ("k_attn_", "k_mva_", "k_gns_", "k_head_"):
        assert not has(ran_s, k), (k, sorted(ran_s))
    assert has(ran_s, "k_render_fwd") and has(ran_s, "k_render_bwd")

    e_loss, e_psnr = relf(res["loss"], ref["loss"]), relf(res["psnr"], ref["psnr"])
    e_g = render_group_errors(res["gaussians"], ref["gaussians"])
    orc = oracle_step(ref["gaussians"], data, bg.cpu().numpy(), oracle_mod)  # (the fp32 oracle's own error)
    assert rel(orc["d_gaussians"], ref["d_gaussians"]) < 1e-12
    rec = {"test": "lgm_step MID fp32 end to end vs fp64 chain", "loss": e_loss, "psnr": e_psnr, "gaussians": e_g,
           "d_gaussians": {}, "groups": {}}
    e_dg, e_dg_s = (render_group_errors(r["gaussians"].grad, ref["d_gaussians"]) for r in (res, res_s))
    e_o32 = render_group_errors(orc["d_gaussians_f32"], orc["d_gaussians"])
    for n in RENDER_GROUPS:
        rec["d_gaussians"][n] = {"bar": grad_bar(e_o32[n]), "fp32_oracle": e_o32[n], "native": e_dg[n],
                                 "stock": e_dg_s[n]}
    for k in ref["groups"]:
        en, es = rel(got[k], ref["groups"][k]), rel(got_s[k], ref["groups"][k])
        rec["groups"][k] = {"bar": max(FP32_BAR, 2 * es), "native": en, "stock": es}
    # and every parameter tensor by itself (a fault in one wrapper's path can be a small share of its group's norm)
    tensors = {k: (rel(named[k], ref["grads"][k]), rel(named_s[k], ref["grads"][k])) for k in ref["grads"]}
    k_n, k_s = max(tensors, key=lambda k: tensors[k][0]), max(tensors, key=lambda k: tensors[k][1])
    rec["worst_tensor"] = {"native": [k_n, tensors[k_n][0]], "stock": [k_s, tensors[k_s][1]]}
    print(f"  worst tensor of {len(tensors)}: native {k_n} {tensors[k_n][0]:.3e}, stock {k_s} {tensors[k_s][1]:.3e}")
    PRECISION.append(rec)
    print(f"fp32 end to end: loss {e_loss:.2e} psnr {e_psnr:.2e} stock loss {relf(res_s['loss'], ref['loss']):.2e}")
    for part in ("d_gaussians", "groups"):
        for k, r in rec[part].items():
            print(f"  {k}: native {r['native']:.3e} stock {r['stock']:.3e} bar {r['bar']:.3e}")
    print("  gaussians: " + " ".join(f"{n} {e:.2e}" for n, e in e_g.items()))
    assert res["gaussians"].dtype == torch.float32
    assert e_loss <= 1e-5 and e_psnr <= 1e-5, (e_loss, e_psnr)
    assert all(e <= 1e-5 for e in e_g.values()), e_g
    for part in ("d_gaussians", "groups"):
        bad = {k: r for k, r in rec[part].items() if not r["native"] <= r["bar"]}
        assert not bad, bad
    bad = {k: v for k, v in tensors.items() if not v[0] <= max(FP32_BAR, 2 * v[1])}
    assert not bad, bad


# ---- 3. bf16 autocast, the UNet + head stage
def native_conv_count(model):
    """The stride-1 convolutions of the UNet that lgm_amd.conv serves under the active autocast (every one of them is
    called once per forward; the stride-2 downsamples and the head's conv never go there)."""
    from lgm_amd.conv import _takes
    dev = next(model.parameters()).device
    convs = [m for m in model.unet.modules() if isinstance(m, torch.nn.Conv2d)]
    took = [c for c in convs if _takes(torch.empty(1, c.in_channels, 8, 8, device=dev), c) is not None]
    assert all(c.stride == (1, 1) for c in took) and len(convs) - len(took) == sum(c.stride == (2, 2) for c in convs)
    return len(took)


@contextlib.contextmanager
def recorded_sites(sites):
    """While entered, every call of the UNet's conv2d and of MVAttention's Linear wrapper appends its module and its
    input to `sites`; the backward then adds the gradient that arrived at its output."""
    import lgm_amd.attention as A
    import lgm_amd.unet as U

    def wrap(fn):
        def call(x, mod):
            out = fn(x, mod)
            site = {"mod": mod, "x": x.detach()}
            out.register_hook(lambda g, site=site: site.__setitem__("g", g.detach()))
            sites.append(site)
            return out
        return call

    saved = (U.conv2d, A._linear16)
    U.conv2d, A._linear16 = wrap(U.conv2d), wrap(A._linear16)
    try:
        yield sites
    finally:
        U.conv2d, A._linear16 = saved


def site_truth(site, dt=torch.bfloat16):
    """The weight and bias gradient of one recorded site in float64 (on the GPU: unfold + matmul, no convolution
    library) from the very 16-bit operands its wrapper saw: x and the output's gradient, each rounded to `dt`."""
    mod = site["mod"]
    x, g = site["x"].to(dt).double(), site["g"].to(dt).double()
    if isinstance(mod, torch.nn.Linear):
        g2, x2 = g.reshape(-1, mod.out_features), x.reshape(-1, mod.in_features)
        return g2.T @ x2, g2.sum(0)
    k = mod.kernel_size[0]
    unf = torch.nn.functional.unfold(x, k, padding=(k - 1) // 2)  # [N, Cin * k * k, H * W]
    return torch.einsum("nop,ncp->oc", g.flatten(2), unf).reshape(mod.weight.shape), g.sum((0, 2, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_bf16_unet_head_stage(cuda, refs, seed):
    """forward_gaussians under bf16 autocast, then gaussians.backward(the float64 chain's d_gaussians): the Gaussians,
    d_input and every parameter group against the float64 model, native and stock; native error / stock error <=
    BF16_STAGE_RATIO_BAR. The 16-bit kernels must have run: flash attention without k_attn_delta, k_wgrad twice per
    MVAttention block, k_conv_wgrad once per stride-1 conv.

    The bf16 stage errors are 3e-2 to 4e-2 in both arms, so a weight gradient that is off by a per cent would pass
    the ratio. The weight and bias gradient of every conv2d / Linear wrapper site is therefore also held, where it
    arrives in p.grad, to float64 on the operands that site saw in this very backward (whatever layout they came in):
    1e-5, the bar of tests/test_conv_wgrad.py and tests/test_wgrad.py."""
    cpu_model, ref = refs(seed)
    model = copy.deepcopy(cpu_model).to(cuda).train()
    data = lgm_data(cuda, B=1, seed=seed)
    dg = ref["d_gaussians"].float().to(cuda)
    want = {"gaussians": ref["gaussians"], "d_input": ref["d_input"], **ref["groups"]}
    prof = nat.KernelProfiler()

    def arm(sites):
        model.zero_grad()
        x = data["input"].clone().requires_grad_(True)
        prof.reset()
        with prof, recorded_sites(sites):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                g = model.forward_gaussians(x)
                n_conv = native_conv_count(model)
            g.backward(dg)
            torch.cuda.synchronize()
        for k, p in model.named_parameters():
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, k
        got = {"gaussians": g, "d_input": x.grad, **grouped({k: p.grad for k, p in model.named_parameters()})}
        return g, {k: rel(got[k], want[k]) for k in want}, launched(prof), n_conv

    sites = []
    g, en, ran, n_conv = arm(sites)
    n_mva = sum(type(m).__name__ == "MVAttention" for m in model.modules())
    assert n_mva == 6 and n_conv > 20
    assert len(sites) == n_conv + 2 * n_mva and len({id(s["mod"]) for s in sites}) == len(sites)
    name_of = {id(m): k for k, m in model.named_modules()}
    e_sites = {}
    for s in sites:
        rw, rb = site_truth(s)
        e_sites[name_of[id(s["mod"])] + ".weight"] = rel(s["mod"].weight.grad, rw)
        if s["mod"].bias is not None:
            e_sites[name_of[id(s["mod"])] + ".bias"] = rel(s["mod"].bias.grad, rb)
    with stock(model):
        g_s, es, ran_s, _ = arm([])
    prof.close()
    assert g.dtype == torch.float32 and g_s.dtype == torch.float32 and g.shape == (1, 4 * 16 * 16, 14)
    for k in ("k_attn_fwd", "k_attn_dq", "k_attn_dkdv"):
        assert ran.get(k) == n_mva, (k, ran)
    assert "k_attn_delta" not in ran
    assert ran.get("k_wgrad") == 2 * n_mva and ran.get("k_conv_wgrad") == n_conv, (ran, n_conv)
    assert has(ran, "k_gns_") and ran.get("k_head_fwd") == 1 and ran.get("k_head_bwd") == 1
    assert has(ran, "k_mva_gn_") and "k_mva_out" in ran and "k_mva_out_bwd" in ran
    assert not ran_s, sorted(ran_s)
    ratios = {k: en[k] / es[k] for k in want}
    worst, worst_site = max(ratios, key=ratios.get), max(e_sites, key=e_sites.get)
    for k in want:
        print(f"bf16 stage seed {seed} {k}: native {en[k]:.3e} stock {es[k]:.3e} ratio {ratios[k]:.3f}")
    print(f"bf16 stage seed {seed} largest native / stock error ratio: {ratios[worst]:.3f} ({worst}; bar "
          f"{BF16_STAGE_RATIO_BAR}); largest of {len(e_sites)} wrapper gradients against fp64 on their own operands: "
          f"{e_sites[worst_site]:.2e} ({worst_site})")
    PRECISION.append({"test": f"lgm_step MID bf16 UNet + head stage vs fp64, seed {seed}", "bar": BF16_STAGE_RATIO_BAR,
                      "native": en, "stock": es, "ratio": ratios,
                      "wrapper_gradients_on_their_operands": {"bar": 1e-5,
                                                              "largest": [worst_site, e_sites[worst_site]]}})
    assert e_sites[worst_site] < 1e-5, {k: e for k, e in e_sites.items() if not e < 1e-5}
    assert BF16_STAGE_RATIO_BAR is not None, "the bar has not been set from a measurement"
    assert ratios[worst] <= BF16_STAGE_RATIO_BAR, (worst, ratios[worst])


# ---- 4. bf16 autocast, the render stage of LGM.forward
@pytest.mark.gpu
def test_bf16_render_stage(cuda, oracle_mod, refs):
    """LGM.forward under bf16 autocast: what the head hands the render is what the render differentiates. The oracle
    at the Gaussians of this very forward: loss and psnr 1e-5, images_pred and alphas_pred 1e-4, gaussians.grad within
    grad_bar of float64 per render group."""
    cpu_model, _ = refs(0)
    model = copy.deepcopy(cpu_model).to(cuda).train()
    data = lgm_data(cuda, B=1, seed=0)
    torch.manual_seed(7)
    bg = torch.rand(3, dtype=torch.float32, device=cuda)
    torch.manual_seed(7)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        res = model(data)
    res["gaussians"].retain_grad()
    res["loss"].backward()
    g = res["gaussians"]
    assert g.dtype == torch.float32 and g.grad.dtype == torch.float32 and res["images_pred"].dtype == torch.float32
    orc = oracle_step(g, data, bg.cpu().numpy(), oracle_mod)
    e = {"loss": relf(res["loss"], orc["loss"]), "psnr": relf(res["psnr"], orc["psnr"]),
         "images_pred": rel(res["images_pred"], orc["image"]), "alphas_pred": rel(res["alphas_pred"], orc["alpha"])}
    e_o32 = render_group_errors(orc["d_gaussians_f32"], orc["d_gaussians"])
    e_dg = render_group_errors(g.grad, orc["d_gaussians"])
    rec = {"test": "lgm_step MID bf16 LGM.forward: render stage vs fp64 oracle at the head's Gaussians", **e,
           "d_gaussians": {n: {"bar": grad_bar(e_o32[n]), "fp32_oracle": e_o32[n], "gpu": e_dg[n]} for n in e_dg}}
    PRECISION.append(rec)
    print("bf16 render stage: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for n, r in rec["d_gaussians"].items():
        print(f"  d_gaussians {n}: gpu {r['gpu']:.3e} fp32 oracle {r['fp32_oracle']:.3e} bar {r['bar']:.3e}")
    assert e["loss"] <= 1e-5 and e["psnr"] <= 1e-5, e
    assert e["images_pred"] <= 1e-4 and e["alphas_pred"] <= 1e-4, e
    bad = {n: r for n, r in rec["d_gaussians"].items() if not r["gpu"] < r["bar"]}
    assert not bad, bad
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype and bool(torch.isfinite(p.grad).all()), k


# ---- 5. two whole training steps
def cat64(ts):
    """As tests/optim_ref.cat64, on the tensors' own device (47 M elements a list: the GPU's float64 is quicker)."""
    return torch.cat([t.detach().double().reshape(-1) for t in ts])


@pytest.mark.gpu
def test_two_training_steps(cuda):
    """Batch assembly -> LGM(MID, native LPIPS) under bf16 autocast -> backward -> lgm_amd.optim.AdamW(max_grad_norm=1)
    under OneCycleLR, twice. The optimizer against tests/optim_ref.truth_step in float64 fed the very gradients the
    backward produced, after each step, by the bars of tests/test_optim_gpu.py: error <= max(2 x the error of torch's
    own fp32 clip + AdamW on the same inputs, 1e-6), the update's floor 2 x the error of the float64 result rounded
    once to fp32."""
    from lgm_amd import data as D, optim as O
    from tests.optim_ref import FLOOR, HP, rel as orel, truth_step
    from tests.test_data_gpu import make_c2w
    from tests.test_lpips_cpu import random_lpips
    from tests.test_lpips_gpu import BF16_RATIO_BAR as LPIPS_BF16_RATIO_BAR
    opt = mid_options(num_views=6, lambda_lpips=1.0)
    torch.manual_seed(0)
    model = LGM(opt, lpips=random_lpips(size=48)).to(cuda).train()
    gen = torch.Generator().manual_seed(4)
    src = torch.randint(0, 256, (1, 6, 24, 24, 4), dtype=torch.uint8, generator=gen)
    yy, xx = torch.meshgrid(torch.arange(24), torch.arange(24), indexing="ij")
    src[..., 3] = (((yy - 12) ** 2 + (xx - 12) ** 2) < 81).to(torch.uint8) * 255  # an opaque disc
    c2w = make_c2w(1, 6)
    aug = D.draw_augmentation(dataclasses.replace(opt, prob_grid_distortion=1.0, prob_cam_jitter=1.0), 1,
                              torch.Generator().manual_seed(6))
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    p_nat = [p for p in model.parameters() if p.requires_grad]
    assert not any(k.startswith("lpips_loss") for k in names) and len(p_nat) > 100
    p_tor = [p.detach().clone().requires_grad_() for p in p_nat]
    truth = [dict(p=p.detach().double(), m=None, v=None, t=0) for p in p_nat]
    nopt, topt = O.AdamW(p_nat, max_grad_norm=1.0, **HP), torch.optim.AdamW(p_tor, **HP)
    scheds = [OneCycleLR(o, max_lr=HP["lr"], total_steps=20, pct_start=0.3) for o in (nopt, topt)]
    prof = nat.KernelProfiler()
    losses, table = [], {}
    for step in (1, 2):
        prof.reset()
        with prof:
            data = D.build_batch(opt, src.to(cuda), c2w.to(cuda), True, augmentation=aug)
            nopt.zero_grad(set_to_none=True)
            torch.manual_seed(7)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                res = model(data)
            res["loss"].backward()
            grads = [p.grad.detach().clone() for p in p_nat]
            before = (cat64(p_nat), cat64(p_tor), cat64([t["p"] for t in truth]))
            nopt.step()
            torch.cuda.synchronize()
        ran = launched(prof)
        for k in ("k_data_", "k_lpips_", "k_optim_", "k_attn_fwd", "k_wgrad", "k_conv_wgrad", "k_render_bwd"):
            assert has(ran, k), (k, sorted(ran))
        assert all(p.grad is None for p in model.lpips_loss.parameters())
        losses.append(float(res["loss"].detach()))
        for p, g in zip(p_tor, grads):
            p.grad = g.clone()
        tnorm = torch.nn.utils.clip_grad_norm_(p_tor, 1.0)
        topt.step()
        hyper = [(list(range(len(p_nat))), gr["lr"], gr["betas"][0], gr["betas"][1], gr["eps"], gr["weight_decay"])
                 for gr in topt.param_groups]
        hyper_n = [(gr["lr"], gr["betas"]) for gr in nopt.param_groups]
        assert hyper_n == [(gr["lr"], gr["betas"]) for gr in topt.param_groups]
        norm = truth_step(truth, [g.double() for g in grads], hyper, 1.0)
        want = cat64([t["p"] for t in truth])
        got, tor = cat64(p_nat), cat64(p_tor)
        rows = {"p": (orel(got, want), orel(tor, want), FLOOR)}
        for key, tk in (("exp_avg", "m"), ("exp_avg_sq", "v")):
            w = cat64([t[tk] for t in truth])
            rows[key] = (orel(cat64([nopt.state[p][key] for p in p_nat]), w),
                         orel(cat64([topt.state[p][key] for p in p_tor]), w), FLOOR)
        du = want - before[2]
        rounded = want.float().double() - before[2].float().double()
        rows["update"] = (orel(got - before[0], du), orel(tor - before[1], du), 2 * orel(rounded, du))
        rows["norm"] = (abs(float(nopt.grad_norm) - norm) / norm, abs(float(tnorm) - norm) / norm, FLOOR)
        table[step] = {"grad_norm": norm, "loss": losses[-1],
                       **{k: {"kernel": a, "torch": b, "floor": c} for k, (a, b, c) in rows.items()}}
        for k, (ek, et, floor) in rows.items():
            print(f"  step {step} {k}: kernel {ek:.2e} torch {et:.2e} floor {floor:.1e} (norm {norm:.3e})")
        for k, (ek, et, floor) in rows.items():
            assert ek <= max(2 * et, floor), (step, k, ek, et, floor)
        assert all(float(nopt.state[p]["step"]) == step for p in p_nat)
        assert all(torch.equal(p.grad, g) for p, g in zip(p_nat, grads)), "the step wrote a gradient"
        if step == 1:
            # loss_lpips: the fused value against lpips_loss with fused = False on the same images_pred under the same
            # autocast, by the module's bf16 bar (tests/test_lpips_gpu.py): fused error / unfused error against an fp64
            # CPU evaluation <= BF16_RATIO_BAR, on the per-view distances
            lp = model.lpips_loss
            pred, args = res["images_pred"].detach(), (data["images_output"], data["masks_output"])
            torch.manual_seed(7)
            bg = torch.rand(3, dtype=torch.float32, device=cuda)
            d = {}
            for fused in (True, False):
                lp.fused = fused
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    d[fused] = lp.loss_from_render(*args, bg, pred).float().view(-1)
            lp.fused = True
            lp64 = copy.deepcopy(lp).cpu().double()
            with torch.no_grad():
                d64 = lp64.loss_from_render(*(a.cpu().double() for a in args), bg.cpu().double(),
                                            pred.cpu().double()).view(-1)
            ef, eu = orel(d[True].cpu().double(), d64), orel(d[False].cpu().double(), d64)
            value = float(res["loss_lpips"].detach())
            e_mean = relf(value, d[True].mean())
            print(f"  loss_lpips {value:.6f}: fused {ef:.3e} unfused {eu:.3e} vs fp64, ratio "
                  f"{ef / eu:.3f} (bar {LPIPS_BF16_RATIO_BAR}); the step's value vs recomputed {e_mean:.1e}")
            table["loss_lpips"] = {"fused": ef, "unfused": eu, "bar_ratio": LPIPS_BF16_RATIO_BAR}
            assert value > 0 and e_mean <= 1e-6
            assert ef / eu <= LPIPS_BF16_RATIO_BAR, (ef, eu)
        for s in scheds:
            s.step()
    prof.close()
    PRECISION.append({"test": "lgm_step MID: two training steps, optimizer vs fp64 on the backward's gradients",
                      **table})
    assert table[1]["grad_norm"] > 0 and abs(losses[1] - losses[0]) > 1e-6 * abs(losses[0]), losses
