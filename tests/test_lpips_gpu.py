"""The LPIPS kernels (include/lgm_lpips.h, lgm_amd/csrc/lpips.hip) and lgm_amd/lpips.py on the GPU, against explicit
fp64 CPU evaluations of the header's formulas, with torch's own composition (same inputs, dtypes and GPU) measured
next to the distance kernel.

Bars of the distance kernel (as tests/test_gn_silu_gpu.py): rel-L2 error against fp64 <= max(2 x the torch
composition's error, floor); the floor is one output rounding: 1e-6 for fp32 results (`out` always), 2^-9 for bf16 and
2^-11 for f16 gradients. The torch composition runs under autocast for the 16-bit dtypes (what it sees in training).
"""
import copy
import warnings

import pytest
import torch
import torch.nn.functional as F

from lgm_amd import LGM, LPIPS, Options
from lgm_amd import _native as nat
from lgm_amd._native import DTYPE_CODES as _DTYPES
from lgm_amd.lpips import _LpipsPrep, _torch_distance, lpips_distance
from tests.golden.make_unet_golden import TINY
from tests.test_lpips_cpu import lgm_data, random_lpips

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FLOOR = {F32: 1e-6, BF16: 2.0 ** -9, F16: 2.0 ** -11}
EPS = 1e-10
# bf16 autocast, LPIPS(size=32): (fused error) / (unfused error), both against an fp64 CPU run, must stay below this.
# Measured over three seeds on an MI355X the largest ratio (value and gradient) was 1.001 (the
# gradient's; the value's ratios were 0.035-0.494, the fused distance being fp32 where torch's 1x1 head is bf16); the
# bar is that + 25 %.
BF16_RATIO_BAR = 1.26


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def make_feats(cuda, N, C, H, W, dt, seed=0, mis=False, near=False, signed=False):
    """f0, f1 = relu(randn) with channel 0 replaced by |randn| + 0.1 (no zero norm); w >= 0; g. mis: contiguous views
    of base[1:] (element-aligned, not 16-byte aligned). near: f1 = f0 + 1e-3 randn. signed: channel 0 keeps randn's
    sign."""
    gen = torch.Generator().manual_seed(seed)

    def one(src=None):
        x = torch.relu(torch.randn(N, C, H, W, generator=gen))
        c0 = torch.randn(N, H, W, generator=gen)
        x[:, 0] = (c0.abs() + 0.1) * (torch.sign(c0) if signed else 1.0)
        if src is not None:
            x = src + 1e-3 * torch.randn(N, C, H, W, generator=gen)
        return x

    a = one()
    b = one(a if near else None)
    out = []
    for x in (a, b):
        flat = torch.zeros(x.numel() + (1 if mis else 0))
        flat[(1 if mis else 0):] = x.reshape(-1)
        flat = flat.to(cuda).to(dt)
        v = (flat[1:] if mis else flat).view(N, C, H, W)
        assert v.is_contiguous() and (not mis or v.data_ptr() % 16 != 0)
        out.append(v)
    w = torch.rand(C, generator=gen).to(cuda)
    g = (torch.rand(N, generator=gen) + 0.5).to(cuda)
    return out[0], out[1], w, g


def dist_forward(f0, f1, w, eps=EPS, ws_bytes=None, norms=True, dt1=None):
    N, C, H, W = f0.shape
    L = nat.lib()
    out = torch.full((N,), -1.0, device=f0.device)
    n0 = torch.empty(N, H, W, device=f0.device) if norms else None
    n1 = torch.empty(N, H, W, device=f0.device) if norms else None
    need = L.lgm_lpips_dist_workspace_size(N, C, H, W)
    ws = torch.empty(max(need, 1), device=f0.device, dtype=torch.uint8)
    rc = L.lgm_lpips_dist_forward(_DTYPES[f0.dtype], _DTYPES[f1.dtype] if dt1 is None else dt1, N, C, H, W, eps,
                                  nat.ptr(f0), nat.ptr(f1), nat.ptr(w), nat.ptr(out), nat.ptr(n0), nat.ptr(n1),
                                  nat.ptr(ws), need if ws_bytes is None else ws_bytes, nat.stream_of(f0.device),
                                  nat.diag())
    return rc, out, n0, n1


def dist_backward(f0, f1, w, n0, n1, g, want=(True, True), eps=EPS):
    N, C, H, W = f0.shape
    df0 = torch.empty_like(f0) if want[0] else None
    df1 = torch.empty_like(f1) if want[1] else None
    code = _DTYPES[f0.dtype]
    rc = nat.lib().lgm_lpips_dist_backward(code, code, N, C, H, W, eps, nat.ptr(f0), nat.ptr(f1), nat.ptr(w),
                                           nat.ptr(n0), nat.ptr(n1), nat.ptr(g), nat.ptr(df0), nat.ptr(df1),
                                           nat.stream_of(f0.device), nat.diag())
    return rc, df0, df1


def reference64(f0, f1, w, g, eps=EPS):
    """fp64 on the CPU, from the (already rounded) inputs: out and the gradients by the header's closed form, with the
    second term dropped where a norm is exactly 0 (elsewhere this is autograd's result; checked in the test below)."""
    a, b, w, g = (t.detach().double().cpu() for t in (f0, f1, w, g))
    N, C, H, W = a.shape
    wv = w.view(1, C, 1, 1)
    na, nb = a.pow(2).sum(1, keepdim=True).sqrt(), b.pow(2).sum(1, keepdim=True).sqrt()
    A, B = na + eps, nb + eps
    ah, bh = a / A, b / B
    d = ah - bh
    out = (wv * d * d).sum(1).mean(dim=(1, 2))
    t0, t1 = (wv * d * ah).sum(1, keepdim=True), (wv * d * bh).sum(1, keepdim=True)
    ia = torch.where(na > 0, 1 / na.clamp_min(1e-300), torch.zeros_like(na))
    ib = torch.where(nb > 0, 1 / nb.clamp_min(1e-300), torch.zeros_like(nb))
    k = g.view(N, 1, 1, 1) / (H * W)
    df0 = k * (2 * wv * d / A - 2 * t0 * a * ia / A)
    df1 = k * (-2 * wv * d / B + 2 * t1 * b * ib / B)
    return out, df0, df1


def torch_ops(f0, f1, w, g):
    a, b = f0.detach().clone().requires_grad_(True), f1.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=f0.dtype, enabled=f0.dtype != F32):
        out = _torch_distance(a, b, w, EPS)
    da, db = torch.autograd.grad(out.float(), [a, b], g)
    return out.detach(), da, db


def form(vec, lp):
    s = ("v" if vec else "s") + ("" if lp == 256 else str(lp))
    return {"k_lpips_dist_" + s, "k_lpips_dist_sum", "k_lpips_dist_bwd_" + s}


def check_case(cuda, N, C, H, W, dt, kernels=None, **kw):
    f0, f1, w, g = make_feats(cuda, N, C, H, W, dt, **kw)
    prof = nat.KernelProfiler()
    with prof:
        rc, out, n0, n1 = dist_forward(f0, f1, w)
        assert rc == 0, nat.lib().lgm_last_error()
        rc, df0, df1 = dist_backward(f0, f1, w, n0, n1, g)
        assert rc == 0, nat.lib().lgm_last_error()
    ran = set(prof.summary())
    prof.close()
    if kernels is not None:
        assert ran == kernels, sorted(ran)
    rout, rdf0, rdf1 = reference64(f0, f1, w, g)
    tout, tdf0, tdf1 = torch_ops(f0, f1, w, g)
    assert float(out.min()) >= 0
    # the stored norms
    n64 = f0.detach().double().cpu().pow(2).sum(1).sqrt()
    assert rel(n0, n64) < 1e-6
    bad = []
    for name, mine, theirs, ref, floor in (("out", out, tout, rout, FLOOR[F32]), ("df0", df0, tdf0, rdf0, FLOOR[dt]),
                                           ("df1", df1, tdf1, rdf1, FLOOR[dt])):
        assert torch.isfinite(mine.float()).all(), name
        e_k, e_t = rel(mine, ref), rel(theirs, ref)
        bar = max(2 * e_t, floor)
        print(f"lpips_dist N{N} C{C} {H}x{W} {str(dt)[6:]} {kw} {name}: kernel {e_k:.3e} torch {e_t:.3e} "
              f"ratio {e_k / max(e_t, 1e-300):.2f} bar {bar:.3e}")
        if not e_k <= bar:
            bad.append((name, e_k, e_t, bar))
    assert not bad, bad


# (N, C, H, W), vector form, pixel items per workgroup (lp_of in lpips.hip), misaligned
ISSUE_CASES = [
    ((2, 64, 16, 16), True, 16, False),    # vector form
    ((1, 3, 5, 7), False, 16, False),      # ragged
    ((2, 512, 4, 4), True, 16, False),     # many channels, small plane
    ((3, 128, 1, 1), False, 16, False),    # single pixel
    ((2, 256, 33, 17), False, 16, False),  # ragged, 36 tiles per image
    ((2, 1, 8, 8), True, 16, False),       # C = 1: every normalised value is 1, the distance ~ 1e-20 (eps): 0 in fp32
    ((2, 64, 8, 8), False, 16, True),      # element-aligned pointer (a base[1:] view)
]


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", ISSUE_CASES, ids=lambda c: "N%d_C%d_%dx%d" % c[0] + ("_mis" if c[3] else ""))
def test_distance_against_fp64(cuda, case, dt):
    (N, C, H, W), vec, lp, mis = case
    check_case(cuda, N, C, H, W, dt, kernels=form(vec, lp), mis=mis)


# every form the dispatch can take: items per plane <= 64 or C >= 256: 16 items x 16 channel slices; else items <= 256
# or C >= 32: 64 x 4; else the workgroup along pixels. Vector items are 4 pixels (HW % 4 == 0, aligned).
FORM_CASES = [
    ((1, 8, 16, 16), True, 16), ((1, 8, 10, 26), True, 64),   # 64 | 65 vector items
    ((1, 8, 32, 32), True, 64), ((1, 8, 4, 257), True, 256),  # 256 | 257 vector items
    ((1, 32, 40, 40), True, 64),                              # 400 items, C = 32: 7 tiles of 64
    ((1, 31, 36, 36), True, 256),                             # 324 items, C = 31: 2 tiles of 256
    ((1, 256, 16, 20), True, 16),                             # 80 items, C = 256: 5 tiles of 16
    ((1, 8, 8, 8), False, 16, True), ((1, 8, 5, 13), False, 64),     # 64 (misaligned) | 65 scalar items
    ((1, 8, 16, 16), False, 64, True), ((1, 8, 1, 257), False, 256),  # 256 (misaligned) | 257 scalar items
    ((1, 40, 9, 29), False, 64),                              # 261 items, C = 40: 5 tiles, 10 channels per slice
    ((2, 5, 33, 35), False, 256),                             # 1155 items: 5 tiles of 256
]


@pytest.mark.parametrize("case", FORM_CASES, ids=lambda c: "C%d_%dx%d" % c[0][1:] + ("_v" if c[1] else "_s") + str(c[2]))
def test_distance_forms(cuda, case):
    (N, C, H, W), vec, lp = case[:3]
    mis = len(case) > 3
    check_case(cuda, N, C, H, W, F32, kernels=form(vec, lp), mis=mis)
    check_case(cuda, N, C, H, W, BF16, kernels=form(vec, lp), mis=mis)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: str(d)[6:])
def test_near_identical_pair(cuda, dt):
    check_case(cuda, 2, 64, 16, 16, dt, near=True)
    check_case(cuda, 2, 256, 33, 17, dt, near=True)


def test_single_channel_signed(cuda):
    """C = 1 with both signs: the normalised values are +-1 and the distance is 4 w times the share of pixels whose
    signs differ (with positive values only, as in the C = 1 case above, it is 0 to fp32). The gradient of f / |f| is
    0 but for eps, so only its size is checked: no more than eps-sized against the first term alone."""
    for dt, (H, W) in ((F32, (8, 8)), (BF16, (8, 8)), (F32, (5, 7))):
        f0, f1, w, g = make_feats(cuda, 2, 1, H, W, dt, signed=True)
        rc, out, n0, n1 = dist_forward(f0, f1, w)
        assert rc == 0
        rc, df0, df1 = dist_backward(f0, f1, w, n0, n1, g)
        assert rc == 0
        rout, _, _ = reference64(f0, f1, w, g)
        differ = (torch.sign(f0.float()) != torch.sign(f1.float())).double().mean(dim=(1, 2, 3)).cpu()
        assert rel(rout, 4 * float(w[0]) * differ) < 1e-6 and float(differ.min()) > 0
        assert rel(out, rout) <= 1e-6
        # |2 w d / A| <= 4 w / 0.1 per unit of g / HW; what is left after the two terms cancel is a rounding of that
        bound = 4 * float(w[0]) / 0.1 * float(g.max()) / (H * W)
        assert float(df0.float().abs().max()) <= 1e-5 * bound and float(df1.float().abs().max()) <= 1e-5 * bound


def test_closed_form_is_autograd(cuda):
    """The header's gradient formula (reference64) against fp64 autograd through the forward formula."""
    f0, f1, w, g = make_feats(cuda, 2, 16, 5, 7, F32)
    a, b = f0.double().cpu().requires_grad_(True), f1.double().cpu().requires_grad_(True)
    na, nb = a.pow(2).sum(1, keepdim=True).sqrt(), b.pow(2).sum(1, keepdim=True).sqrt()
    out = (w.double().cpu().view(1, -1, 1, 1) * (a / (na + EPS) - b / (nb + EPS)).pow(2)).sum(1).mean(dim=(1, 2))
    da, db = torch.autograd.grad(out, [a, b], g.double().cpu())
    rout, rdf0, rdf1 = reference64(f0, f1, w, g)
    assert rel(rout, out) < 1e-14 and rel(rdf0, da) < 1e-12 and rel(rdf1, db) < 1e-12


@pytest.mark.parametrize("shape", [(2, 64, 16, 16), (2, 256, 33, 17), (1, 8, 4, 257)], ids=["v16", "s16", "v"])
def test_identical_inputs_are_exactly_zero(cuda, shape):
    for dt in (F32, BF16):
        f0, _, w, g = make_feats(cuda, *shape, dt)
        f1 = f0.clone()
        rc, out, n0, n1 = dist_forward(f0, f1, w)
        assert rc == 0
        rc, df0, df1 = dist_backward(f0, f1, w, n0, n1, g)
        assert rc == 0
        assert bool((out == 0).all()) and bool((df0 == 0).all()) and bool((df1 == 0).all())
        assert torch.equal(n0, n1)


def test_zero_norm_pixel(cuda):
    """One pixel zeroed in all channels of f1 (and another in f0): finite gradients, equal to the fp64 formula with the
    second term dropped there (torch's composition returns NaN at such a pixel)."""
    for dt, shape in ((F32, (2, 64, 16, 16)), (BF16, (2, 64, 16, 16)), (F32, (1, 3, 5, 7))):
        f0, f1, w, g = make_feats(cuda, *shape, dt)
        f1[:, :, 2, 3] = 0
        f0[0, :, 4, 1] = 0
        rc, out, n0, n1 = dist_forward(f0, f1, w)
        assert rc == 0
        rc, df0, df1 = dist_backward(f0, f1, w, n0, n1, g)
        assert rc == 0
        assert float(n1[0, 2, 3]) == 0.0 and float(n0[0, 4, 1]) == 0.0
        rout, rdf0, rdf1 = reference64(f0, f1, w, g)
        assert torch.isfinite(df0.float()).all() and torch.isfinite(df1.float()).all() and torch.isfinite(out).all()
        assert rel(out, rout) <= 1e-6
        # at the zeroed pixels the first term is all there is: -+ 2 w d / eps g / HW, about 1e10 times the others
        assert rel(df1[:, :, 2, 3], rdf1[:, :, 2, 3]) <= FLOOR[dt] and rel(df0[0, :, 4, 1], rdf0[0, :, 4, 1]) <= FLOOR[dt]
        # ... and everywhere else (those pixels masked out of both sides)
        keep = torch.ones(f0.shape, dtype=torch.float64)
        keep[:, :, 2, 3] = 0
        keep[0, :, 4, 1] = 0
        assert rel(df0.double().cpu() * keep, rdf0 * keep) <= FLOOR[dt]
        assert rel(df1.double().cpu() * keep, rdf1 * keep) <= FLOOR[dt]
        _, tdf0, tdf1 = torch_ops(f0, f1, w, g)
        assert not torch.isfinite(tdf1.float()).all()  # (the deviation recorded in DESIGN §7)


def test_null_outputs_and_reproducible(cuda):
    for shape, dt in (((2, 64, 16, 16), BF16), ((2, 256, 33, 17), F32), ((2, 5, 33, 35), F32)):
        f0, f1, w, g = make_feats(cuda, *shape, dt)
        runs = []
        for _ in range(2):
            rc, out, n0, n1 = dist_forward(f0, f1, w)
            assert rc == 0
            rc, df0, df1 = dist_backward(f0, f1, w, n0, n1, g)
            assert rc == 0
            runs.append((out, n0, n1, df0, df1))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        out, n0, n1, df0, df1 = runs[0]
        rc, none0, only1 = dist_backward(f0, f1, w, n0, n1, g, want=(False, True))
        assert rc == 0 and none0 is None and torch.equal(only1, df1)
        rc, only0, none1 = dist_backward(f0, f1, w, n0, n1, g, want=(True, False))
        assert rc == 0 and none1 is None and torch.equal(only0, df0)
        rc, out2, _, _ = dist_forward(f0, f1, w, norms=False)  # inference: no norms kept
        assert rc == 0 and torch.equal(out2, out)


def test_errors_are_reported_not_launched(cuda):
    L = nat.lib()
    f0, f1, w, g = make_feats(cuda, 2, 64, 16, 16, F32)
    p = nat.ptr
    st = nat.stream_of(cuda)
    need = L.lgm_lpips_dist_workspace_size(2, 64, 16, 16)
    assert need == 2 * 4 * 4  # one fp32 per workgroup: 4 tiles per image (64 vector items / 16, or 256 pixels / 64)
    ws = torch.empty(need, device=cuda, dtype=torch.uint8)
    out = torch.empty(2, device=cuda)
    prof = nat.KernelProfiler()
    with prof:
        # C <= 0
        rc = L.lgm_lpips_dist_forward(0, 0, 2, 0, 16, 16, EPS, p(f0), p(f1), p(w), p(out), None, None, p(ws), need, st,
                                      None)
        assert rc < 0 and b"bad shape" in L.lgm_last_error()
        rc = L.lgm_lpips_dist_backward(0, 0, 2, -1, 16, 16, EPS, p(f0), p(f1), p(w), p(out), p(out), p(g), p(f0), None,
                                       st, None)
        assert rc < 0 and b"bad shape" in L.lgm_last_error()
        # mismatched dtypes, unknown dtype
        rc, *_ = dist_forward(f0, f1, w, dt1=1)
        assert rc < 0 and b"one dtype" in L.lgm_last_error()
        rc = L.lgm_lpips_dist_forward(5, 5, 2, 64, 16, 16, EPS, p(f0), p(f1), p(w), p(out), None, None, p(ws), need, st,
                                      None)
        assert rc < 0 and b"dtype" in L.lgm_last_error()
        # null pointers (and only one of the two norms)
        for args in ((None, p(f1), p(w), p(out), None, None), (p(f0), p(f1), None, p(out), None, None),
                     (p(f0), p(f1), p(w), None, None, None), (p(f0), p(f1), p(w), p(out), p(out), None)):
            rc = L.lgm_lpips_dist_forward(0, 0, 2, 64, 16, 16, EPS, *args, p(ws), need, st, None)
            assert rc < 0 and b"null" in L.lgm_last_error()
        rc = L.lgm_lpips_dist_backward(0, 0, 2, 64, 16, 16, EPS, p(f0), p(f1), p(w), None, None, p(g), p(f0), None, st,
                                       None)
        assert rc < 0 and b"null" in L.lgm_last_error()
        # a short workspace
        rc, *_ = dist_forward(f0, f1, w, ws_bytes=need - 1)
        assert rc < 0 and b"workspace" in L.lgm_last_error()
        rc = L.lgm_lpips_dist_forward(0, 0, 2, 64, 16, 16, EPS, p(f0), p(f1), p(w), p(out), None, None, None, need, st,
                                      None)
        assert rc < 0 and b"workspace" in L.lgm_last_error()
        # a grid beyond the launch limits: sizes only, nothing is read
        rc = L.lgm_lpips_dist_forward(0, 0, 1 << 20, 1 << 9, 1 << 10, 1 << 10, EPS, None, None, None, None, None, None,
                                      None, 0, None, None)
        assert rc < 0 and b"grid" in L.lgm_last_error()
        # the input pass
        rc = L.lgm_lpips_prep_forward(0, 2, 0, 16, p(f0), None, None, None, p(f0), None, st, None)
        assert rc < 0 and b"bad shape" in L.lgm_last_error()
        rc = L.lgm_lpips_prep_forward(0, 2, 16, 16, None, None, None, None, p(f0), None, st, None)
        assert rc < 0 and b"null" in L.lgm_last_error()
        rc = L.lgm_lpips_prep_forward(0, 2, 16, 16, p(f0), p(f0), p(f0), None, p(f0), p(f0), st, None)  # mask, no bg
        assert rc < 0 and b"null" in L.lgm_last_error()
        rc = L.lgm_lpips_prep_backward(7, 2, 16, 16, p(f0), p(f0), st, None)
        assert rc < 0 and b"dtype" in L.lgm_last_error()
        rc = L.lgm_lpips_prep_backward(0, 2, 16, 16, None, p(f0), st, None)
        assert rc < 0 and b"null" in L.lgm_last_error()
        assert not prof.summary()
    prof.close()
    assert L.lgm_lpips_dist_workspace_size(2, 0, 16, 16) == 0


# ---- the input pass
PREP_SIZES = [(16, 16), (32, 16), (24, 16), (8, 16), (7, 10), (1, 4)]
SHIFT = torch.tensor([-.030, -.088, -.188], dtype=torch.float64).view(1, 3, 1, 1)
SCALE = torch.tensor([.458, .448, .450], dtype=torch.float64).view(1, 3, 1, 1)


def prep64(v, R):
    return (F.interpolate(v, (R, R), mode="bilinear", align_corners=False) * 2 - 1 - SHIFT) / SCALE


@pytest.mark.parametrize("with_gt", [True, False], ids=["gt", "pred_only"])
@pytest.mark.parametrize("S,R", PREP_SIZES, ids=lambda v: str(v))
def test_input_pass(cuda, S, R, with_gt):
    M = 2
    gen = torch.Generator().manual_seed(S * 100 + R)
    pred = torch.rand(M, 3, S, S, generator=gen)
    gt = torch.rand(M, 3, S, S, generator=gen)
    mask = (torch.rand(M, 1, S, S, generator=gen) > 0.4).float() * torch.rand(M, 1, S, S, generator=gen)
    bg = torch.rand(3, generator=gen)
    dx = torch.randn(M, 3, R, R, generator=gen)
    p64 = pred.double().requires_grad_(True)
    xp64 = prep64(p64, R)
    dp64, = torch.autograd.grad(xp64, p64, dx.double())
    xg64 = prep64(gt.double() * mask.double() + bg.double().view(1, 3, 1, 1) * (1 - mask.double()), R)
    L = nat.lib()
    pd, gd, md, bd, dxd = (t.to(cuda) for t in (pred, gt, mask, bg, dx))
    xp = torch.empty(M, 3, R, R, device=cuda)
    xg = torch.full((M, 3, R, R), 7.0, device=cuda)
    dpred = torch.empty(M, 3, S, S, device=cuda)
    st = nat.stream_of(cuda)
    prof = nat.KernelProfiler()
    with prof:
        if with_gt:
            rc = L.lgm_lpips_prep_forward(0, M, S, R, nat.ptr(pd), nat.ptr(gd), nat.ptr(md), nat.ptr(bd), nat.ptr(xp),
                                          nat.ptr(xg), st, nat.diag())
        else:
            rc = L.lgm_lpips_prep_forward(0, M, S, R, nat.ptr(pd), None, None, None, nat.ptr(xp), None, st, nat.diag())
        assert rc == 0, L.lgm_last_error()
        rc = L.lgm_lpips_prep_backward(0, M, S, R, nat.ptr(dxd), nat.ptr(dpred), st, nat.diag())
        assert rc == 0, L.lgm_last_error()
    assert set(prof.summary()) == {"k_lpips_prep", "k_lpips_prep_bwd"}
    prof.close()
    e = {"x_pred": rel(xp, xp64), "d_pred": rel(dpred, dp64)}
    if with_gt:
        e["x_gt"] = rel(xg, xg64)
    else:
        assert bool((xg == 7.0).all())  # not written
    print(f"lpips_prep S{S} R{R} gt={with_gt}: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert all(v <= 1e-6 for v in e.values()), e
    if with_gt:  # the autograd Function, and a bf16 output (one rounding of the fp32 value)
        pa = pd.clone().requires_grad_(True)
        xa, xga = _LpipsPrep.apply(pa, gd, md, bd, R, F32)
        assert torch.equal(xa, xp) and torch.equal(xga, xg) and not xga.requires_grad
        da, = torch.autograd.grad(xa, pa, dxd)
        assert torch.equal(da, dpred)
        xb, xgb = _LpipsPrep.apply(pd, gd, md, bd, R, BF16)
        assert torch.equal(xb, xp.to(BF16)) and torch.equal(xgb, xg.to(BF16))


# ---- the module
def module_pair(cuda, seed):
    torch.manual_seed(seed)
    m_cpu = random_lpips(size=32)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
    y = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
    return m_cpu, x, y


def run_module(m, x, y, fused, autocast=False):
    m.fused = fused
    ya = y.clone().requires_grad_(True)
    prof = nat.KernelProfiler()
    with prof:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            d = m(x, ya)
        gy, = torch.autograd.grad(d.float().sum(), ya)
    ran = {k for k in prof.summary() if k.startswith("k_lpips_")}
    prof.close()
    assert bool(ran) == fused, sorted(ran)  # the HIP kernels ran, or none of them
    assert d.shape == (2, 1, 1, 1)
    return d.detach().float().view(-1), gy


def test_module_fp32_fused_against_unfused(cuda):
    m_cpu, x, y = module_pair(cuda, 0)
    m = copy.deepcopy(m_cpu).to(cuda)
    da, ga = run_module(m, x.to(cuda), y.to(cuda), True)
    db, gb = run_module(m, x.to(cuda), y.to(cuda), False)
    print(f"lpips module fp32: value {rel(da, db):.3e} grad {rel(ga, gb):.3e}")
    assert rel(da, db) < 1e-5 and rel(ga, gb) < 1e-5
    assert float(da.min()) > 0
    # identical feature maps are at distance exactly 0 with exactly zero gradients, through the autograd Function
    # (two runs of the trunk's convolutions on one image need not be bitwise equal, so this is asked of the op)
    f = m.net((y.to(cuda) - m.shift.view(1, 3, 1, 1)) / m.scale.view(1, 3, 1, 1))[2].detach()
    fa, fb = f.clone().requires_grad_(True), f.clone().requires_grad_(True)
    d = lpips_distance(fa, fb, m.lins[2])
    ga, gb = torch.autograd.grad(d.sum(), [fa, fb])
    assert bool((d == 0).all()) and bool((ga == 0).all()) and bool((gb == 0).all())


def test_module_bf16_autocast_against_fp64(cuda):
    worst = 0.0
    for seed in (0, 1, 2):
        m_cpu, x, y = module_pair(cuda, seed)
        m64 = copy.deepcopy(m_cpu).double()
        y64 = y.double().requires_grad_(True)
        d64 = m64(x.double(), y64)
        g64, = torch.autograd.grad(d64.sum(), y64)
        m = copy.deepcopy(m_cpu).to(cuda)
        errs = {}
        for fused in (True, False):
            d, g = run_module(m, x.to(cuda), y.to(cuda), fused, autocast=True)
            errs[fused] = {"value": rel(d, d64.view(-1)), "grad": rel(g, g64)}
        for k in ("value", "grad"):
            r = errs[True][k] / errs[False][k]
            worst = max(worst, r)
            print(f"lpips bf16 seed {seed} {k}: fused {errs[True][k]:.3e} unfused {errs[False][k]:.3e} ratio {r:.3f}")
    print(f"lpips bf16 largest fused / unfused error ratio: {worst:.3f} (bar {BF16_RATIO_BAR})")
    assert worst <= BF16_RATIO_BAR


def test_loss_from_render_fused_against_unfused(cuda):
    """loss_from_render at S = 24 -> size 32 (the input kernel + the distance kernels) against the torch lines."""
    m_cpu, _, _ = module_pair(cuda, 3)
    m = copy.deepcopy(m_cpu).to(cuda)
    gen = torch.Generator().manual_seed(3)
    gt = torch.rand(1, 2, 3, 24, 24, generator=gen).to(cuda)
    mask = (torch.rand(1, 2, 1, 24, 24, generator=gen) > 0.5).float().to(cuda)
    bg = torch.rand(3, generator=gen).to(cuda)
    pred = torch.rand(1, 2, 3, 24, 24, generator=gen).to(cuda)
    res = {}
    for fused in (True, False):
        m.fused = fused
        pa = pred.clone().requires_grad_(True)
        prof = nat.KernelProfiler()
        with prof:
            d = m.loss_from_render(gt, mask, bg, pa)
            g, = torch.autograd.grad(d.sum(), pa)
        ran = {k for k in prof.summary() if k.startswith("k_lpips_")}
        prof.close()
        assert ({"k_lpips_prep", "k_lpips_prep_bwd"} <= ran) == fused and bool(ran) == fused, sorted(ran)
        assert d.shape == (2, 1, 1, 1)
        res[fused] = (d.detach(), g)
    print(f"loss_from_render fp32: value {rel(res[True][0], res[False][0]):.3e} grad {rel(res[True][1], res[False][1]):.3e}")
    assert rel(res[True][0], res[False][0]) < 1e-5 and rel(res[True][1], res[False][1]) < 1e-5


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_lgm_forward_with_native_lpips(cuda, mode):
    """LGM.forward with lambda_lpips = 1 and the native module (render 32 x 32 -> LPIPS at 48 x 48): loss and
    d conv.weight against the same model with fused = False on the UNet and on LPIPS."""
    opt = Options(input_size=16, splat_size=16, output_size=32, lambda_lpips=1.0, **TINY)
    torch.manual_seed(0)
    model = LGM(opt, lpips=random_lpips(size=48)).to(cuda)
    data = {k: v.to(cuda) for k, v in lgm_data(B=2).items()}
    getattr(model, mode)()
    res = {}
    for fused in (True, False):
        model.unet.fused = fused
        model.lpips_loss.fused = fused
        model.zero_grad()
        torch.manual_seed(7)  # the background drawn in training mode
        prof = nat.KernelProfiler()
        with prof:
            out = model(data)
            out["loss"].backward()
        ran = {k for k in prof.summary() if k.startswith("k_lpips_")}
        prof.close()
        assert bool(ran) == fused, sorted(ran)
        assert not any("lpips_loss" in k for k in model.state_dict())
        assert all(p.grad is None for p in model.lpips_loss.parameters())
        res[fused] = (float(out["loss"]), float(out["loss_lpips"]), model.conv.weight.grad.clone())
    (la, lpa, ga), (lb, lpb, gb) = res[True], res[False]
    print(f"lgm {mode}: loss {la:.6f} / {lb:.6f} lpips {lpa:.6f} / {lpb:.6f} d conv.weight {rel(ga, gb):.3e}")
    assert lpa > 0 and abs(la - lb) <= 1e-4 * abs(lb) and abs(lpa - lpb) <= 1e-4 * abs(lpb)
    assert rel(ga, gb) <= 1e-4
