"""lgm_amd.conv.conv2d_native (forward, input gradient and weight gradient on the HIP kernels) against conv2d and fp64,
its fallbacks and other input forms, and the UNet's opt-in `native_conv` switch (tiny configuration of
tests/test_unet_gpu.py)."""
import copy

import pytest
import torch
import torch.nn as nn

from lgm_amd import UNet
from lgm_amd import _native as nat
from lgm_amd.conv import conv2d, conv2d_native
from tests.golden.make_unet_golden import TINY
from tests.test_conv_module_gpu import FALLBACKS, conv_weights
from tests.test_unet_gpu import grouped, relv

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -9  # one bf16 output rounding
# bf16 autocast, tiny UNet: (error with native_conv on) / (error with it off), both against fp64, per group of
# tests/test_unet_gpu.py. Measured over three seeds and four runs on an MI355X the largest ratio was RATIO_MEASURED
# (DESIGN.md §2); the bar is that + 25 %: MIOpen's arm moves between runs.
RATIO_MEASURED = 1.120
RATIO_BAR = 1.25 * RATIO_MEASURED


def run(conv, x0, gy, fn, prep=None):
    conv.zero_grad()
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = fn(x if prep is None else prep(x), conv)
    y.backward(gy.to(y.dtype))
    return (y.detach(), x.grad.clone(), conv.weight.grad.clone(), None if conv.bias is None else conv.bias.grad.clone())


def fp64(conv, x16, g16):
    """fp64 CPU output and input gradient of the conv on the 16-bit operands the GPU paths see."""
    c = copy.deepcopy(conv).cpu().double()
    with torch.no_grad():
        c.weight.copy_(conv.weight.detach().to(x16.dtype).double().cpu())
        if c.bias is not None:
            c.bias.copy_(conv.bias.detach().to(x16.dtype).double().cpu())
    x = x16.detach().double().cpu().requires_grad_(True)
    y = c(x)
    y.backward(g16.detach().double().cpu())
    return y.detach(), x.grad


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", [(3, 2, 24, 40, 10, 10), (1, 2, 16, 8, 8, 8)], ids=["3x3", "1x1"])
def test_conv2d_native_against_conv2d(cuda, shape, bias):
    """Under bf16 autocast: output and input gradient within max(2 x conv2d's error, one rounding) of fp64; weight / bias
    gradients bitwise conv2d's (the same lgm_conv_wgrad on the same operands); a no-grad call launches k_conv_fwd."""
    k, N, Cin, Cout, H, W = shape
    torch.manual_seed(3)
    conv = nn.Conv2d(Cin, Cout, k, padding=k // 2, bias=bias).to(cuda)
    x0 = torch.randn(N, Cin, H, W, device=cuda)
    gy = torch.randn(N, Cout, H, W, device=cuda)
    run(conv, x0, gy, conv2d)  # (warm-up)
    yt, dxt, dwt, dbt = run(conv, x0, gy, conv2d)
    prof = nat.KernelProfiler()
    with prof:
        yn, dxn, dwn, dbn = run(conv, x0, gy, conv2d_native)
    ran = {k_: v[0] for k_, v in prof.summary().items()}
    assert ran.get("k_conv_fwd") == 1 and ran.get("k_conv_dgrad") == 1 and ran.get("k_conv_wgrad") == 1, ran
    assert yn.dtype == yt.dtype == torch.bfloat16 and dxn.dtype == dxt.dtype
    ry, rx = fp64(conv, x0.to(torch.bfloat16), gy.to(torch.bfloat16))
    for name, mine, theirs, ref in (("y", yn, yt, ry), ("dx", dxn, dxt, rx)):
        e, et = relv(mine, ref), relv(theirs, ref)
        print(f"conv2d_native {shape} bias={bias} {name}: rel L2 native {e:.3e}, conv2d {et:.3e}")
        assert e <= max(2 * et, FLOOR)
    assert torch.equal(dwn, dwt)
    if bias:
        assert torch.equal(dbn, dbt)
    prof.reset()
    with prof, torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y0 = conv2d_native(x0, conv)
    ran = prof.summary()
    prof.close()
    assert ran.get("k_conv_fwd", (0,))[0] == 1 and "k_conv_dgrad" not in ran and "k_conv_wgrad" not in ran, ran
    assert torch.equal(y0, yn) and not y0.requires_grad


@pytest.mark.parametrize("name", ["fp32", "stride2", "5x5", "reflect"])
def test_fallbacks_are_conv(cuda, name, monkeypatch):
    """What the kernels do not take is conv(x) itself: the autograd Function is never entered and no k_conv_* launch."""
    from lgm_amd import conv as CV

    def boom(*a, **k):
        raise AssertionError("_ConvNative used on a call the kernels do not take")

    monkeypatch.setattr(CV._ConvNative, "apply", boom)
    kw, autocast, _ = FALLBACKS[name]
    torch.manual_seed(5)
    conv = nn.Conv2d(16, 24, **kw).to(cuda)
    x0 = torch.randn(2, 16, 12, 12, device=cuda)
    outs = []
    prof = nat.KernelProfiler()
    for native in (False, True, False):  # (the first call of a shape is MIOpen's warm-up)
        conv.zero_grad()
        x = x0.clone().requires_grad_(True)
        with prof, torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = conv2d_native(x, conv) if native else conv(x)
            y.float().square().sum().backward()
        outs.append(y.detach())
    ran = prof.summary()
    prof.close()
    assert not [k for k in ran if k.startswith("k_conv")], ran
    assert outs[1].dtype == outs[2].dtype and torch.equal(outs[1], outs[2])


def test_other_input_forms(cuda):
    """A channels_last input and a 16-bit input that is an offset view of a flat buffer (2-byte aligned only) agree with
    the contiguous call bitwise: output, input gradient and weight gradient."""
    torch.manual_seed(6)
    conv = nn.Conv2d(16, 24, 3, padding=1).to(cuda)
    x0 = torch.randn(2, 16, 12, 12, device=cuda)
    gy = torch.randn(2, 24, 12, 12, device=cuda)
    base = run(conv, x0, gy, conv2d_native)
    cl = run(conv, x0, gy, conv2d_native, prep=lambda t: t.contiguous(memory_format=torch.channels_last))
    gcl = run(conv, x0, gy.contiguous(memory_format=torch.channels_last), conv2d_native)
    for a, b, c in zip(base, cl, gcl):
        assert torch.equal(a, b) and torch.equal(a, c)

    conv16 = copy.deepcopy(conv).to(torch.bfloat16)

    def view_of(t, by):
        flat = torch.zeros(t.numel() + 8, device=cuda, dtype=torch.bfloat16)
        v = flat[by:by + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 2 * by
        return v

    res = []
    for by in (0, 1):
        conv16.zero_grad()
        xv = view_of(x0, by).requires_grad_(True)
        y = conv2d_native(xv, conv16)
        y.backward(view_of(gy, by))
        res.append((y.detach(), xv.grad.clone(), conv16.weight.grad.clone(), conv16.bias.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert relv(res[0][0], base[0]) < 2.0 ** -6  # (the 16-bit module rounds its weights; the same convolution)


@pytest.fixture(scope="module")
def tiny_runs(cuda):
    """Tiny UNets under bf16 autocast, three seeds: default construction, native_conv on (twice) and off, and the fp64
    CPU run of the module."""
    out = []
    for seed in (0, 1, 2):
        torch.manual_seed(200 + seed)
        u_cpu = UNet(9, 14, **TINY)
        assert u_cpu.native_conv is False
        gen = torch.Generator().manual_seed(seed)
        x, w = torch.randn(8, 9, 16, 16, generator=gen), torch.randn(8, 14, 16, 16, generator=gen)
        u64 = copy.deepcopy(u_cpu).double()
        x64 = x.double().requires_grad_(True)
        y64 = u64(x64)
        (y64 * w.double()).sum().backward()
        ref = {"y": y64.detach(), "grad_x": x64.grad, **grouped({k: p.grad for k, p in u64.named_parameters()})}
        u = copy.deepcopy(u_cpu).to(cuda)
        runs = {}
        for key, native in (("warm-up", None), ("default", None), ("on", True), ("on2", True), ("off", False)):
            if native is not None:
                u.native_conv = native
            u.zero_grad()
            xa = x.to(cuda).requires_grad_(True)
            prof = nat.KernelProfiler()
            with prof:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = u(xa)
                (y.float() * w.to(cuda)).sum().backward()
            ran = prof.summary()
            prof.close()
            runs[key] = (y.detach().float(), xa.grad.clone(), {k: p.grad.clone() for k, p in u.named_parameters()}, ran)
        out.append((u, ref, runs))
    return out


def test_unet_switch_and_kernel_counts(cuda, tiny_runs):
    """Default construction: native_conv False and no k_conv_fwd. Switch on: k_conv_fwd, k_conv_dgrad and k_conv_wgrad
    once per stride-1 conv (these runs ask for the input's gradient, so conv_in runs its input gradient too), and one
    k_conv_wpack in front of each forward and each input gradient."""
    u, _, runs = tiny_runs[0]
    ran_d, ran_on, ran_off = runs["default"][3], runs["on"][3], runs["off"][3]
    assert "k_conv_fwd" not in ran_d and "k_conv_dgrad" not in ran_d, ran_d
    assert "k_conv_fwd" not in ran_off and "k_conv_dgrad" not in ran_off, ran_off
    n_native = len([k for k in conv_weights(runs["on"][2]) if "downsample" not in k])
    assert ran_on["k_conv_fwd"][0] == n_native and ran_on["k_conv_wpack"][0] == 2 * n_native, ran_on
    assert ran_on["k_conv_dgrad"][0] == n_native and ran_on["k_conv_wgrad"][0] == n_native, ran_on


def test_unet_first_conv_runs_no_dgrad(cuda, tiny_runs):
    """With an input that needs no gradient (training: the images), conv_in runs no input gradient: k_conv_dgrad one
    time fewer than k_conv_fwd."""
    u = tiny_runs[0][0]
    u.native_conv = True
    u.zero_grad()
    x = torch.randn(8, 9, 16, 16, device=cuda)
    prof = nat.KernelProfiler()
    with prof:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = u(x)
        y.float().square().sum().backward()
    ran = prof.summary()
    prof.close()
    u.native_conv = False
    assert ran["k_conv_dgrad"][0] == ran["k_conv_fwd"][0] - 1, ran


def test_unet_native_conv_repeatable(cuda, tiny_runs):
    for _, _, runs in tiny_runs:
        a, b = runs["on"], runs["on2"]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for k in conv_weights(a[2]):
            if "downsample" not in k:
                assert torch.equal(a[2][k], b[2][k]), k


def test_unet_error_ratio_against_fp64(cuda, tiny_runs):
    worst = 0.0
    for seed, (_, ref, runs) in enumerate(tiny_runs):
        errs = {}
        for key in ("on", "off"):
            y, gx, gp, _ = runs[key]
            got = {"y": y, "grad_x": gx, **grouped(gp)}
            errs[key] = {k: relv(got[k], ref[k]) for k in ref}
        for k in ref:
            r = errs["on"][k] / errs["off"][k]
            worst = max(worst, r)
            print(f"tiny bf16 seed {seed} {k}: native_conv on {errs['on'][k]:.3e} off {errs['off'][k]:.3e} ratio {r:.3f}")
    print(f"tiny bf16 largest native_conv on / off error ratio: {worst:.3f} (bar {RATIO_BAR:.3f})")
    assert worst <= RATIO_BAR
