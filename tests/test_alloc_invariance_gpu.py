"""Every native op on poisoned, red-zoned allocations (tests/alloc_guard.py).

The wrappers in lgm_amd allocate their outputs, saved statistics and workspaces with torch.empty / torch.empty_like /
nat.workspace; include/*.h promise that outputs are overwritten and that a workspace's contents do not matter. Here the
contents and the neighbourhood of each of those allocations are inputs of the test:

  * test_invariant_under_fill runs each row of ROWS three times, under guarded(0x00), guarded(0x3F) and guarded(0xFF)
    (zeros; 0.747 / a large positive int32; NaN / -1), and asserts that no output holds a NaN or Inf, that no red zone
    (4 KiB of canary bytes on either side of every allocation) was written, that the three runs guarded the same number
    of allocations (at least one), that the KernelProfiler saw the kernels the row is there for, and that the outputs
    agree across the fills: bitwise, except the gradients summed by float atomics (the render backward without
    deterministic=True), which are held to rel L2 <= 1e-5 against the 0x00 run -- the bound the suite already uses for
    two orders of the same atomic sums (test_repeated_backward_retain_graph, test_exact_culling_is_output_preserving,
    test_two_chunk_items_float_path_vs_oracle).
  * test_reference_check_under_poison calls existing checks, with their own fp64 references and bars, inside
    guarded(0xFF): invariance alone does not show that the poisoned run is right.
  * test_every_compute_entry_point_was_swept: every name of nat.SIGNATURES but the host-only ones was called by a row.

Each run prints one line (allocations and bytes guarded, red zones checked); each row one more with the largest rel
L2 between fills of its float-atomic gradients.
"""
import contextlib

import numpy as np
import pytest
import torch

from lgm_amd import _native as nat
from tests.alloc_guard import guarded
from tests.render_cases import TAN, rel_l2, scene, upstream

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0x3F, 0xFF)
ATOMIC_TOL = 1e-5
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

ROWS = []  # (id, run(cuda, monkeypatch) -> {name: tensor}, kernels, absent, atomic)
SWEPT = set()  # the C-ABI entry points the rows called
RAN = set()  # the rows that ran (the coverage test needs all of them)
_in_row = False


def row(name, kernels=(), absent=(), atomic=()):
    """Registers a row. kernels: KernelProfiler names every run must launch; absent: names it must not (the other
    path's); atomic: the outputs summed by float atomics (rel L2 <= ATOMIC_TOL instead of bitwise)."""
    def deco(fn):
        ROWS.append(pytest.param(fn, frozenset(kernels), frozenset(absent), frozenset(atomic), id=name))
        return fn
    return deco


@pytest.fixture(scope="module", autouse=True)
def record_calls():
    """nat.call, recording the entry points the rows reach (the wrappers call it as an attribute of the module)."""
    real = nat.call

    def call(name, device, *args):
        if _in_row:
            SWEPT.add(name)
        return real(name, device, *args)

    nat.call = call
    yield
    nat.call = real


@contextlib.contextmanager
def ending_the_session_on_a_gpu_fault():
    """A HIP error under poison is a finding about uninitialised memory used as an index or a count, and the device
    is not to be used after it: the session ends there instead of starting the remaining tests on the card."""
    try:
        yield
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, nothing more is started on the device: {e}", returncode=3)
        raise


def _cpu(t):
    if isinstance(t, np.ndarray):
        t = np.ascontiguousarray(t)
        return torch.from_numpy(t.view(np.int32) if t.dtype == np.uint32 else t)
    return t.detach().cpu()


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_guard_on_the_device(cuda):
    """tests/test_alloc_guard.py's two defects on device tensors (torch ops only, inside memory the guard owns): the
    store past the end is reported, the uninitialised accumulator shows in the result; so a clean row below is a
    finding about the kernels, not about the guard."""
    got = []
    for fill in FILLS:
        with guarded(fill) as g:
            acc = torch.empty(7, device=cuda)
            acc += torch.arange(7.0, device=cuda)
            t = torch.empty(5, 3, device=cuda, dtype=BF16)
            t.zero_()
            t.as_strided((16,), (1,))[15] = 1.0
            assert acc.data_ptr() % 256 == 0 and t.data_ptr() % 256 == 0
        got.append(acc.cpu())
        assert g.n_allocations == 2 and g.zones_checked == 4
        assert [(v.side, v.shape, v.dtype, v.offsets) for v in g.violations] == [("after", (5, 3), BF16, [0, 1])]
        assert "test_guard_on_the_device" in g.violations[0].site
    assert torch.equal(got[0], torch.arange(7.0)) and torch.isfinite(got[1]).all() and torch.isnan(got[2]).all()
    assert not torch.equal(got[1], got[0])


@pytest.mark.parametrize("run,kernels,absent,atomic", ROWS)
def test_invariant_under_fill(cuda, monkeypatch, request, run, kernels, absent, atomic):
    global _in_row
    name = request.node.callspec.id
    RAN.add(name)
    prof = nat.KernelProfiler()
    outs, counts = [], []
    try:
        for fill in FILLS:
            _in_row = True
            try:
                with ending_the_session_on_a_gpu_fault(), guarded(fill) as g, prof:
                    out = run(cuda, monkeypatch)
            finally:
                _in_row = False
            ran = set(prof.summary())
            prof.reset()
            print(f"{name} fill 0x{fill:02X}: {g.n_allocations} allocations, {g.n_bytes} bytes guarded, "
                  f"{g.zones_checked} red zones checked, {len(g.violations)} violated")
            g.assert_clean()
            assert kernels <= ran and not (absent & ran), f"fill 0x{fill:02X}: launched {sorted(ran)}"
            outs.append({k: _cpu(v) for k, v in out.items()})
            counts.append(g.n_allocations)
    finally:
        prof.close()
    assert counts[0] >= 1 and counts[0] == counts[1] == counts[2], counts
    assert atomic <= set(outs[0]), sorted(outs[0])
    worst = 0.0
    for fill, out in zip(FILLS, outs):
        assert set(out) == set(outs[0])
        for k, v in out.items():
            if v.is_floating_point():
                assert bool(torch.isfinite(v).all()), f"{k} under fill 0x{fill:02X} is not finite"
            if k in atomic:
                e = rel_l2(v.double().numpy(), outs[0][k].double().numpy())
                worst = max(worst, e)
                assert e <= ATOMIC_TOL, f"{k} under fill 0x{fill:02X}: rel L2 {e:.3e} against the 0x00 run"
            else:
                assert _same_bits(v, outs[0][k]), f"{k} under fill 0x{fill:02X} differs from the 0x00 run"
    if atomic:
        print(f"{name}: largest rel L2 between fills of {sorted(atomic)}: {worst:.3e}")


# ------------------------------------------------------------------------------------------------------- render
SLOT = {"k_bin", "k_sort", "k_render_fwd"}
BWD = {"k_render_bwd", "k_preproc_bwd"}
PACKED = {"k_bin_count", "k_scan"}  # the exact-count workspace: lgm_render_count_pairs, then count, scan and fill


def _render(cuda, g, cv, cvp, H, W, bg, d_img, d_dep, d_alp, **kw):
    from lgm_amd.gs import rasterize
    gd = g.to(cuda).requires_grad_(True)
    img, dep, alp = rasterize(gd, cv.to(cuda), cvp.to(cuda), bg.to(cuda), TAN, TAN, H, W, **kw)
    outs, ups = [img, alp], [d_img.to(cuda), d_alp.to(cuda)]
    if d_dep is not None:
        outs.append(dep)
        ups.append(d_dep.to(cuda))
    torch.autograd.backward(outs, ups)
    return {"image": img, "depth": dep, "alpha": alp, "d_gaussians": gd.grad}


@row("render-float-slot-needles", SLOT | BWD, PACKED | {"k_det_seed_max"}, atomic=["d_gaussians"])
def _(cuda, mp):
    """Float mode, slot workspace, backward of image, depth and alpha; stretched Gaussians make needle records, whose
    conic partials go to the fp64 side accumulators (zeroed by k_bin for needle records only)."""
    from lgm_amd.gs import forward_state
    g, cv, cvp = scene(B=2, N=2000, V=3, seed=5)
    g[:, ::10, 4] *= 20.0
    d_img, d_dep, d_alp, bg = upstream(2, 3, 64, 64)
    out = _render(cuda, g, cv, cvp, 64, 64, bg, d_img, d_dep, d_alp)
    st = forward_state(g.to(cuda), cv.to(cuda), cvp.to(cuda), TAN, TAN, 64, 64, lists=True, records=True)
    SWEPT.update(("lgm_render_tile_lists", "lgm_render_pixel_state", "lgm_render_records"))
    rects = st["rects"].reshape(-1, 2)
    vis = ((rects[:, 0] & 0xFFFF) != (rects[:, 1] & 0xFFFF)) & (st["radii"].reshape(-1) > 0)
    flag = (rects[:, 1] >> 31).astype(bool)
    assert (vis & flag).sum() > 0, "no needle record: the fp64 side accumulators are not part of this run"
    # the same decision by lgm_render_needle_flags on the stored records (into a poisoned flag buffer)
    P, Q = st["P"].reshape(-1, 4)[vis], st["Q"].reshape(-1, 4)[vis]
    abc = torch.from_numpy(np.stack([P[:, 2], P[:, 3], Q[:, 0]], 1).copy()).to(cuda)
    flags = torch.empty(len(abc), dtype=torch.uint8, device=cuda)
    nat.check(nat.lib().lgm_render_needle_flags(len(abc), nat.ptr(abc), nat.ptr(flags), nat.stream_of(cuda)),
              "lgm_render_needle_flags")
    SWEPT.add("lgm_render_needle_flags")
    assert np.array_equal(flags.cpu().numpy().astype(bool), flag[vis])
    out.update(radii=st["radii"], tile_counts=st["tile_counts"], n_contrib=st["n_contrib"], final_T=st["final_T"],
               needle_flags=flags)
    for b, per_view in enumerate(st["ids"]):
        for v, ids in enumerate(per_view):
            out[f"ids[{b}][{v}]"] = ids
    return out


@row("render-production-deterministic-40x72", SLOT | BWD | {"k_det_seed_max"}, PACKED)
def _(cuda, mp):
    g, cv, cvp = scene(N=2500, V=2, seed=2502)
    d_img, _, d_alp, bg = upstream(1, 2, 40, 72)
    return _render(cuda, g, cv, cvp, 40, 72, bg, d_img, None, d_alp, clamp=True, deterministic=True)


@row("render-packed-workspace", SLOT | BWD | PACKED | {"k_det_seed_max"})
def _(cuda, mp):
    from lgm_amd import gs
    mp.setattr(gs, "_WS_BUDGET", 0)
    g, cv, cvp = scene(N=3000, V=2, seed=5)
    d_img, d_dep, d_alp, bg = upstream(1, 2, 64, 64)
    return _render(cuda, g, cv, cvp, 64, 64, bg, d_img, d_dep, d_alp, deterministic=True)


@row("render-fused-loss", SLOT | BWD | {"k_loss_reduce", "k_det_seed_max"}, PACKED)
def _(cuda, mp):
    from lgm_amd.gs import rasterize
    from tests.test_loss_gpu import _case
    g, cv, cvp, _, gt, mask, bg, _, _ = (t.to(cuda) for t in _case(1, 2, 3000, 64, seed=3064))
    gd = g.clone().requires_grad_(True)
    img, dep, alp, loss4 = rasterize(gd, cv, cvp, bg, TAN, TAN, 64, 64, clamp=True, gt_images=gt, gt_masks=mask,
                                     deterministic=True)
    (loss4[0] + 0.5 * loss4[1] + 0.25 * loss4[2]).backward()
    assert {"lgm_render_forward_loss", "lgm_render_backward_loss"} <= SWEPT
    return {"image": img, "depth": dep, "alpha": alp, "loss4": loss4, "d_gaussians": gd.grad}


@row("render-34-views", SLOT | BWD, PACKED, atomic=["d_gaussians"])
def _(cuda, mp):
    """More views than k_preproc_bwd<true> takes (PRE_MAXV): k_preproc_bwd<false>."""
    g, cv, cvp = scene(B=1, N=400, V=34, seed=434)
    d_img, d_dep, d_alp, bg = upstream(1, 34, 32, 32)
    return _render(cuda, g, cv, cvp, 32, 32, bg, d_img, d_dep, d_alp)


@row("render-oversized-bucket", SLOT | BWD, PACKED, atomic=["d_gaussians"])
def _(cuda, mp):
    """> 8192 Gaussians on the centre tiles: the LDS-chunk + global-merge sort."""
    g, cv, cvp = scene(N=20000, V=1, seed=11, shrink=0.02, scale_mul=0.05)
    d_img, d_dep, d_alp, bg = upstream(1, 1, 64, 64)
    return _render(cuda, g, cv, cvp, 64, 64, bg, d_img, d_dep, d_alp)


@row("render-equal-depth-12000", SLOT | BWD, PACKED, atomic=["d_gaussians"])
def _(cuda, mp):
    """Every depth equal: the id-digit radix passes, on an oversized bucket."""
    g, cv, cvp = scene(N=12000, V=1, seed=12000)
    g[..., 2] = 0.0
    g[..., 0:2] *= 0.6
    d_img, d_dep, d_alp, bg = upstream(1, 1, 48, 48)
    return _render(cuda, g, cv, cvp, 48, 48, bg, d_img, d_dep, d_alp)


def _checkpoints(cuda, det):
    g, cv, cvp = scene(B=3, N=7000, V=2, seed=6, elevation=-15.0)
    d_img, _, d_alp, bg = upstream(3, 2, 72, 72, seed=8)
    return _render(cuda, g, cv, cvp, 72, 72, bg, d_img, None, d_alp, clamp=True, deterministic=det)


@row("render-checkpoint-items-float", SLOT | BWD, PACKED | {"k_det_seed_max"}, atomic=["d_gaussians"])
def _(cuda, mp):
    """72^2 with long lists: tiles that walk many chunks, backward work items from the checkpoint slots."""
    return _checkpoints(cuda, False)


@row("render-checkpoint-items-deterministic", SLOT | BWD | {"k_det_seed_max"}, PACKED)
def _(cuda, mp):
    return _checkpoints(cuda, True)


@row("render-retain-graph-deterministic", SLOT | BWD | {"k_det_seed_max"}, PACKED)
def _(cuda, mp):
    """Two backwards of one forward: the second clears what the first left (LGM_RENDER_BACKWARD_AGAIN)."""
    from lgm_amd.gs import rasterize
    g, cv, cvp = scene(N=3000, V=2, seed=5)
    gd = g.to(cuda).requires_grad_(True)
    img, _, alp = rasterize(gd, cv.to(cuda), cvp.to(cuda), torch.ones(3, device=cuda), TAN, TAN, 64, 64,
                            deterministic=True)
    w = torch.randn(img.shape, generator=torch.Generator().manual_seed(3)).to(cuda)
    loss = (img * w).sum() + alp.sum()
    (first,) = torch.autograd.grad(loss, gd, retain_graph=True)
    (second,) = torch.autograd.grad(loss, gd)
    assert first.abs().sum().item() > 0 and torch.equal(first, second)
    return {"image": img, "alpha": alp, "first": first, "second": second}


@row("render-no-gaussians", {"k_render_fwd"}, {"k_bin", "k_sort"})
def _(cuda, mp):
    from lgm_amd.gs import rasterize
    g, cv, cvp = scene(N=64, V=2, seed=3)
    bg = torch.tensor([0.1, 0.2, 0.3])
    img, dep, alp = rasterize(g[:, :0].contiguous().to(cuda), cv.to(cuda), cvp.to(cuda), bg.to(cuda), TAN, TAN, 32, 32)
    assert torch.equal(img.cpu(), bg.view(1, 1, 3, 1, 1).expand(1, 2, 3, 32, 32)) and not alp.any()
    return {"image": img, "depth": dep, "alpha": alp}


@row("render-all-culled", SLOT | BWD, PACKED, atomic=["d_gaussians"])
def _(cuda, mp):
    """Every Gaussian behind the near plane: the background, and gradients that are exactly zero."""
    g, cv, cvp = scene(N=64, V=2, seed=3)
    g[..., 0:3] = torch.tensor([0.0, 0.0, 1.45])
    d_img, d_dep, d_alp, _ = upstream(1, 2, 32, 32)
    bg = torch.tensor([0.1, 0.2, 0.3])
    out = _render(cuda, g, cv[:, :1], cvp[:, :1], 32, 32, bg, d_img[:, :1], d_dep[:, :1], d_alp[:, :1])
    assert float(out["d_gaussians"].abs().max()) == 0.0 and not out["alpha"].any()
    return out


# ------------------------------------------------------------------------------------------------ Gaussian head
def _head_row(B, V, h, w, dtype, seed):
    def run(cuda, mp):
        from lgm_amd.head import gaussian_head
        from tests.test_head import _inputs
        x, conv, d = _inputs(B, V, h, w, seed=seed, dtype=dtype)
        xg = x.to(cuda).requires_grad_(True)
        cg = torch.nn.Conv2d(14, 14, 1).to(cuda)
        cg.load_state_dict(conv.state_dict())
        out = gaussian_head(xg, cg, B, V)
        out.backward(d.to(cuda))
        return {"out": out, "dx": xg.grad, "dW": cg.weight.grad, "db": cg.bias.grad}
    row(f"head-{str(dtype)[6:]}-{B}x{V}x{h}x{w}", {"k_head_fwd", "k_head_bwd"})(run)


_head_row(2, 3, 17, 23, F32, 247)
_head_row(3, 1, 1, 1, F32, 311)
_head_row(2, 6, 40, 40, BF16, 7)


# ---------------------------------------------------------------------------------------------------- attention
def _attention_row(shape, dtype):
    def run(cuda, mp):
        from lgm_amd.attention import packed_attention
        B, L, H, D = shape
        g = torch.Generator(device="cpu").manual_seed(B * 7919 + L * 31 + H * 7 + D)
        qkv = (torch.randn((B, L, 3, H, D), generator=g) * 1.5).to(cuda, dtype)
        d_o = torch.randn((B, L, H, D), generator=g).to(cuda, dtype)
        x = qkv.clone().requires_grad_(True)
        o = packed_attention(x, D ** -0.5)
        o.backward(d_o)
        return {"o": o, "dqkv": x.grad}
    row("attention-" + "x".join(map(str, shape)) + "-" + str(dtype)[6:],
        {"k_attn_fwd", "k_attn_dq", "k_attn_dkdv"} | ({"k_attn_delta"} if dtype == F32 else set()))(run)


for _shape in ((3, 65, 2, 64), (2, 100, 3, 128), (1, 17, 1, 32)):
    for _dt in (F32, BF16, F16):
        _attention_row(_shape, _dt)


def _mva_row(case, mode):
    """The MVAttention module on its fused layout kernels; under autocast also linear.linear's k_wgrad."""
    from tests.test_attention import MVA_GN_KERNEL

    def run(cuda, mp):
        from lgm_amd.attention import MVAttention
        C, heads, frames, H, W, B = case[:6]
        groups = case[6] if len(case) > 6 else 32
        torch.manual_seed(11)
        m = MVAttention(C, heads, num_frames=frames, skip_scale=0.5 ** 0.5, groups=groups)
        with torch.no_grad():
            m.norm.weight.uniform_(0.5, 1.5)
            m.norm.bias.uniform_(-0.2, 0.2)
        gen = torch.Generator().manual_seed(12)
        x0 = torch.randn(B * frames, C, H, W, generator=gen) * 2 + 0.3
        gy = torch.randn(B * frames, C, H, W, generator=gen)
        m = m.to(cuda)
        assert m.fused
        x = x0.to(cuda).requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16, enabled=mode == "bf16_autocast"):
            y = m(x)
        y.float().backward(gy.to(cuda))
        out = {"y": y, "dx": x.grad}
        out.update({k: p.grad for k, p in m.named_parameters()})
        return out

    kernels = {MVA_GN_KERNEL[case], "k_mva_gn_coef", "k_mva_out", "k_mva_out_bwd", "k_attn_fwd"}
    row("mva-" + "x".join(map(str, case)) + "-" + mode, kernels | ({"k_wgrad"} if mode == "bf16_autocast" else set()),
        {"k_mva_gn_reg", "k_mva_gn_tok", "k_mva_stats"} - kernels)(run)


for _case in ((96, 3, 2, 7, 5, 1), (256, 8, 4, 8, 8, 2), (512, 16, 1, 46, 46, 1), (512, 16, 1, 48, 48, 1),
              (512, 16, 2, 4, 4, 1, 1)):
    for _mode in ("f32", "bf16_autocast"):
        _mva_row(_case, _mode)


# ------------------------------------------------------------------------------------------- lgm_linear_wgrad
def _wgrad_row(case, dtype):
    def run(cuda, mp):
        K, M, N, ld, want_db = case
        g = torch.Generator().manual_seed(K * 7 + M * 3 + N)
        wide = torch.randn((K, ld or M), generator=g).to(cuda, dtype)
        x = torch.randn((K, N), generator=g).to(cuda, dtype)
        dw = torch.empty((M, N), device=cuda)
        db = torch.empty((M,), device=cuda) if want_db else None
        ws, ws_bytes = nat.workspace("lgm_linear_wgrad_workspace_size", cuda, K, M, N, int(want_db))
        nat.call("lgm_linear_wgrad", cuda, nat.DTYPE_CODES[dtype], K, M, N, nat.ptr(wide), ld or M, nat.ptr(x), N,
                 nat.ptr(dw), nat.ptr(db), nat.ptr(ws), ws_bytes)
        if K == 0:
            assert not dw.any() and not db.any()
        return {"dw": dw, "db": db}
    row("linear-wgrad-" + "x".join(map(str, case[:4])) + "-" + str(dtype)[6:], {"k_wgrad"} if case[0] else set())(run)


for _case in ((1234, 200, 136, 0, True), (33, 8, 8, 0, True), (777, 96, 40, 160, True), (0, 64, 64, 0, True)):
    _wgrad_row(_case, BF16)
_wgrad_row((1234, 200, 136, 0, True), F16)


# --------------------------------------------------------------------------------------------------------- conv
def _conv_row(case, dtype):
    def run(cuda, mp):
        from lgm_amd.conv import conv2d_native
        ksize, N, Cin, Cout, H, W = case
        g = torch.Generator().manual_seed(2000 * ksize + 131 * N + 17 * Cin + 7 * Cout + 3 * H + W)
        conv = torch.nn.Conv2d(Cin, Cout, ksize, padding=(ksize - 1) // 2)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
            conv.bias.copy_(torch.randn(Cout, generator=g))
        x = torch.randn((N, Cin, H, W), generator=g).to(cuda).requires_grad_(True)
        dy = torch.randn((N, Cout, H, W), generator=g).to(cuda)
        conv = conv.to(cuda)
        with torch.autocast("cuda", dtype=dtype):
            y = conv2d_native(x, conv)
        assert y.dtype == dtype
        y.backward(dy.to(dtype))
        return {"y": y, "dx": x.grad, "dW": conv.weight.grad, "db": conv.bias.grad}
    row("conv-k%d-" % case[0] + "x".join(map(str, case[1:])) + "-" + str(dtype)[6:],
        {"k_conv_wpack", "k_conv_fwd", "k_conv_dgrad", "k_conv_wgrad"})(run)


for _case in ((3, 2, 24, 40, 10, 10), (1, 2, 70, 24, 8, 8), (3, 3, 8, 8, 1, 1), (3, 2, 28, 20, 3, 5)):
    for _dt in (BF16, F16):
        _conv_row(_case, _dt)


# ----------------------------------------------------------------------------------------------- GroupNorm+SiLU
def _gn_row(shape, xdt, ydt, family=None, form=None, mis=False):
    from tests.test_gn_silu_gpu import kernel_names

    def run(cuda, mp):
        from lgm_amd.unet import group_norm_silu
        from tests.test_gn_silu_gpu import make_inputs
        N, C, G, H, W, rs = shape
        x, gamma, beta, dy = make_inputs(cuda, N, C, H, W, G, rs, xdt, ydt, seed=3, misalign=mis)
        norm = torch.nn.GroupNorm(G, C).to(cuda)
        with torch.no_grad():
            norm.weight.copy_(gamma)
            norm.bias.copy_(beta)
        xa = x.detach().requires_grad_(True)
        assert xa.data_ptr() == x.data_ptr()
        with torch.autocast("cuda", dtype=ydt, enabled=ydt != xdt):
            y = group_norm_silu(xa, norm, {0: None, 1: "up", 2: "down"}[rs])
        assert y.dtype == ydt
        y.backward(dy)
        return {"y": y, "dx": xa.grad, "dgamma": norm.weight.grad, "dbeta": norm.bias.grad}

    name = "gn-silu-N%d_C%d_G%d_%dx%d_rs%d-" % shape + str(xdt)[6:] + "-" + str(ydt)[6:] + ("-mis" if mis else "")
    row(name, set(kernel_names(family, form)) if family else {"k_gns_bwd_coef"})(run)


# one shape per entry of test_gn_silu_gpu.SMALL, the three resamplings among them
for _shape in ((1, 32, 32, 2, 2, 2), (2, 96, 32, 6, 10, 1), (3, 64, 32, 5, 7, 0), (2, 40, 8, 4, 4, 2)):
    for _x, _y in ((F32, F32), (BF16, BF16), (F32, BF16)):
        _gn_row(_shape, _x, _y)
# one of each dispatch form of test_gn_silu_gpu.THRESHOLDS
_gn_row((1, 32, 32, 1, 4096, 0), F32, F32, "slab", "v")
_gn_row((1, 32, 32, 1, 4100, 0), F32, F32, "chunk", "v")
_gn_row((1, 32, 32, 1, 4100, 0), F32, BF16, "chunk", "v")
_gn_row((1, 32, 32, 1, 4097, 0), F32, F32, "chunk", "s")
_gn_row((2, 8, 4, 4, 6, 1), F32, F32, "slab", "s16")
_gn_row((2, 8, 4, 4, 6, 1), F32, BF16, "slab", "s16")
_gn_row((1, 96, 1, 8, 8, 0), F32, F32, "chunk", "s16", mis=True)


# -------------------------------------------------------------------------------------------------------- LPIPS
def _lpips_dist_row(case, dt):
    from tests.test_lpips_gpu import form
    (N, C, H, W), vec, lp, mis = case

    def run(cuda, mp):
        from lgm_amd.lpips import lpips_distance
        from tests.test_lpips_gpu import make_feats
        f0, f1, w, g = make_feats(cuda, N, C, H, W, dt, mis=mis)
        a, b = f0.detach().requires_grad_(True), f1.detach().requires_grad_(True)
        out = lpips_distance(a, b, w)
        out.backward(g)
        return {"out": out, "df0": a.grad, "df1": b.grad}

    row("lpips-dist-N%d_C%d_%dx%d" % (N, C, H, W) + ("_mis-" if mis else "-") + str(dt)[6:], form(vec, lp))(run)


for _case in (((1, 3, 5, 7), False, 16, False), ((2, 1, 8, 8), True, 16, False), ((2, 64, 8, 8), False, 16, True)):
    for _dt in (F32, BF16, F16):
        _lpips_dist_row(_case, _dt)


def _lpips_prep_row(S, R, with_gt):
    def run(cuda, mp):
        from lgm_amd.lpips import _LpipsPrep
        M = 2
        gen = torch.Generator().manual_seed(S * 100 + R)
        pred = torch.rand(M, 3, S, S, generator=gen).to(cuda)
        gt = torch.rand(M, 3, S, S, generator=gen).to(cuda)
        mask = ((torch.rand(M, 1, S, S, generator=gen) > 0.4).float() * torch.rand(M, 1, S, S, generator=gen)).to(cuda)
        bg = torch.rand(3, generator=gen).to(cuda)
        dx = torch.randn(M, 3, R, R, generator=gen).to(cuda)
        if with_gt:
            pa = pred.clone().requires_grad_(True)
            xp, xg = _LpipsPrep.apply(pa, gt, mask, bg, R, F32)
            d_pred, = torch.autograd.grad(xp, pa, dx)
            return {"x_pred": xp, "x_gt": xg, "d_pred": d_pred}
        xp = torch.empty(M, 3, R, R, device=cuda)  # (the module always has a gt: the ABI's gt = NULL form, directly)
        d_pred = torch.empty(M, 3, S, S, device=cuda)
        nat.call("lgm_lpips_prep_forward", cuda, 0, M, S, R, nat.ptr(pred), None, None, None, nat.ptr(xp), None)
        nat.call("lgm_lpips_prep_backward", cuda, 0, M, S, R, nat.ptr(dx), nat.ptr(d_pred))
        return {"x_pred": xp, "d_pred": d_pred}
    row(f"lpips-prep-S{S}_R{R}-" + ("gt" if with_gt else "pred_only"), {"k_lpips_prep", "k_lpips_prep_bwd"})(run)


for _S, _R in ((7, 10), (24, 16)):
    for _gt in (True, False):
        _lpips_prep_row(_S, _R, _gt)


# --------------------------------------------------------------------------------------------------------- data
def _data_row(Hs, Ws, h, So, n):
    def run(cuda, mp):
        from lgm_amd import data as D
        from tests import test_data_gpu as T
        src = T.make_src(Hs, Ws, seed=Hs + h)
        knots, nknots = T.make_knots(h, n, seed=h)
        jit = torch.rand(T.B, T.VI, 2, generator=torch.Generator().manual_seed(2)) * 2 - 1
        cams = D.data_cameras(T.make_c2w().to(cuda), T.VI, jit, 0.1, T.RADIUS, T.FOVY, T.ZNEAR, T.ZFAR)
        views = D.data_views(src.to(cuda), cams[0], knots, nknots, T.FOVY, T.VI, h, So)
        out = dict(zip(("pose_in", "cam_view", "cam_view_proj", "cam_pos", "c2w_colmap"), cams))
        out.update(zip(("input", "images_output", "masks_output"), views))
        return out
    row(f"data-{Hs}x{Ws}-h{h}-So{So}-n{n}", {"k_data_cameras", "k_data_in", "k_data_out"})(run)


_data_row(10, 14, 7, 5, 8)
_data_row(1, 1, 4, 4, 8)


# ---------------------------------------------------------------------------------------------------- optimizer
@row("optim-fused-step-and-clip", {"k_optim_sqnorm", "k_optim_reduce", "k_optim_adamw", "k_optim_scale"})
def _(cuda, mp):
    from lgm_amd import optim as O
    from tests.optim_ref import Arms
    from tests.test_optim_gpu import BIG, small_slots
    a = Arms(small_slots(), cuda, seed=3, max_norm=1.0, torch_arm=False)
    a.set_grads(a.draw(BIG), torch_arm=False)
    a.opt.step()
    out = {"grad_norm": a.opt.grad_norm}
    for i, p in enumerate(a.p_nat):
        out[f"p{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = p, a.opt.state[p]["exp_avg"], a.opt.state[p]["exp_avg_sq"]
    b = Arms(small_slots(), cuda, seed=4, max_norm=None, torch_arm=False)
    b.set_grads(b.draw(BIG), torch_arm=False)
    out["clip_norm"] = O.clip_grad_norm_(b.p_nat, 1.0)
    assert float(out["clip_norm"]) > 100  # (the clip is active: the gradients are scaled)
    out.update({f"clipped{i}": p.grad for i, p in enumerate(b.p_nat)})
    return out


# --------------------------------------------------------------------------------------------------------- mesh
MESH_DENSITY = {"k_mesh_bin_count", "k_mesh_scan_reduce", "k_mesh_scan_top", "k_mesh_scan_add", "k_mesh_bin_fill",
                "k_mesh_density"}
MESH_EXTRACT = {"k_mesh_classify", "k_mesh_emit"}
MESH_SAMPLE = {"k_mesh_sample_bin_count", "k_mesh_point_count", "k_mesh_point_fill", "k_mesh_sample"}


@row("mesh-gaussians-to-mesh-texels2", MESH_DENSITY | MESH_EXTRACT | MESH_SAMPLE | {"k_mesh_atlas"})
def _(cuda, mp):
    from lgm_amd.mesh import gaussians_to_mesh
    from tests.mesh_raster_ref import nets_gaussians
    m = gaussians_to_mesh(nets_gaussians().to(cuda), resolution=24, texels=2)
    assert m.faces.shape[0] > 0 and m.texture is not None
    return {"vertices": m.vertices, "faces": m.faces, "colors": m.colors, "uvs": m.uvs, "face_uvs": m.face_uvs,
            "texture": m.texture}


@row("mesh-sample-field-tiny", MESH_SAMPLE)
def _(cuda, mp):
    from lgm_amd.mesh import sample_field
    from tests.mesh_texture_ref import sample_cases
    g, G, mod, pts = sample_cases()["tiny"]
    sigma, rgb = sample_field(torch.from_numpy(g).to(cuda), torch.from_numpy(pts).to(cuda), G, scale_modifier=mod)
    return {"sigma": sigma, "rgb": rgb}


@row("mesh-extraction-scans-span-tiles", MESH_EXTRACT | {"k_mesh_scan_reduce", "k_mesh_scan_top", "k_mesh_scan_add"})
def _(cuda, mp):
    from lgm_amd.mesh import extract_surface
    sigma = torch.from_numpy(np.random.default_rng(5).uniform(0, 1, (48, 48, 48)).astype(np.float32)).to(cuda)
    m = extract_surface(sigma, None, 0.5)
    assert m.faces.shape[0] > 0
    return {"vertices": m.vertices, "faces": m.faces}


# -------------------------------------------------------------------------------------------------- mesh raster
MR_FORWARD = {"k_mr_project", "k_mr_vis", "k_mr_vis_big", "k_mr_shade"}
MR_BACKWARD = {"k_mr_absmax", "k_mr_scatter", "k_mr_convert"}


def _mesh_raster_row(name):
    def run(cuda, mp):
        from lgm_amd.meshraster import render_mesh
        from tests import mesh_raster_ref as R
        mesh, cv, cvp, H, W, _, _, d = R.case(name)
        m = R.on(mesh, cuda)
        p = R.param_of(m).clone().requires_grad_(True)
        out = render_mesh(R.with_param(m, p), cv.to(cuda), cvp.to(cuda), H, W, R.BG)
        g, = torch.autograd.grad((out["image"] * torch.from_numpy(d).to(cuda)).sum(), p)
        return {"image": out["image"], "alpha": out["alpha"], "depth": out["depth"], "face_id": out["face_id"],
                "d_param": g}
    row("mesh-raster-" + name, MR_FORWARD | MR_BACKWARD)(run)


_mesh_raster_row("hand_texture_40x72")  # backward to the texture
_mesh_raster_row("boxes_33x47")  # backward to the colours; boxes on both sides of the small-box switch


@row("mesh-raster-empty-mesh")  # (whatever it launches: nothing is declared)
def _(cuda, mp):
    from lgm_amd.mesh import Mesh
    from lgm_amd.meshraster import render_mesh
    from tests import mesh_raster_ref as R
    cv, cvp = R.cameras([10.0], [20.0])
    m = Mesh(torch.zeros(0, 3, device=cuda), torch.zeros(0, 3, dtype=torch.int32, device=cuda),
             torch.zeros(0, 3, device=cuda))
    out = render_mesh(m, cv.to(cuda), cvp.to(cuda), 5, 7, R.BG)
    assert bool((out["face_id"] == -1).all())
    return {k: out[k] for k in ("image", "alpha", "depth", "face_id")}


# ---------------------------------------------------------------------------------- reference checks under poison
def _ref_head(cuda, O):
    from tests.test_head import test_head_fp32_vs_torch
    test_head_fp32_vs_torch(cuda, 2, 3, 17, 23)


def _ref_wgrad(cuda, O):
    from tests.test_wgrad import test_wgrad_vs_fp64
    test_wgrad_vs_fp64(cuda, (1234, 200, 136, 0, True), BF16)


def _ref_attention(dtype, tol):
    def check(cuda, O):
        from tests.test_attention import test_packed_attention_vs_fp64
        test_packed_attention_vs_fp64(cuda, (3, 65, 2, 64), dtype, tol)
    return check


def _ref_render_parity(cuda, O):
    from tests.test_render_gpu import test_forward_backward_parity
    test_forward_backward_parity(cuda, O, 2, 2000, 3, 64, 64, 1.0)


def _ref_render_oversized(cuda, O):
    from tests.test_render_gpu import test_oversized_tile_bucket
    test_oversized_tile_bucket(cuda, O)


def _ref_mesh_raster(name):
    def check(cuda, O):
        from tests import mesh_raster_ref as R
        R.check_forward(name, cuda)
        R.check_backward(name, cuda)
    return check


def _ref_conv_fwd(cuda, O):
    from tests.test_conv_fwd import test_conv_forward_and_dgrad_vs_fp64
    test_conv_forward_and_dgrad_vs_fp64(cuda, (3, 2, 8, 16, 3, 5), BF16)


def _ref_conv_wgrad(cuda, O):
    from tests.test_conv_wgrad import test_conv_wgrad_vs_fp64
    test_conv_wgrad_vs_fp64(cuda, (3, 2, 8, 16, 3, 5), BF16)


def _ref_gn_silu(cuda, O):
    from tests.test_gn_silu_gpu import SMALL, test_small_shapes
    test_small_shapes(cuda, SMALL[0], F32, F32)


def _ref_lpips(cuda, O):
    from tests.test_lpips_gpu import ISSUE_CASES, test_distance_against_fp64
    test_distance_against_fp64(cuda, ISSUE_CASES[1], F32)


def _ref_data(cuda, O):
    from tests.test_data_gpu import test_views_against_fp64_and_torch
    test_views_against_fp64_and_torch(cuda, 1, 1, 4, 4, 8)


def _ref_mesh_density(cuda, O):
    from tests import test_mesh_gpu as T
    T._GRIDS.pop("tiny", None)  # (computed here, under the poison, not taken from an earlier test)
    T.test_density_against_fp64(cuda, "tiny")


def _ref_mesh_e2e(cuda, O):
    from tests.test_mesh_gpu import test_end_to_end_against_fp64
    test_end_to_end_against_fp64(cuda, "ragged")


def _ref_mesh_sample(cuda, O):
    from tests import test_mesh_texture_gpu as T
    T._SAMPLES.pop("tiny", None)
    T.test_sample_against_fp64(cuda, "tiny")


def _ref_optim(cuda, O):
    from tests.optim_ref import Arms
    from tests.test_optim_gpu import BIG, SMALL, small_slots
    a = Arms(small_slots(), cuda, seed=0)
    for k in range(2):
        a.step(a.draw(BIG if k % 2 == 0 else SMALL), label=f"poisoned step {k + 1}")


REFERENCE_CHECKS = {
    "head": _ref_head, "linear-wgrad": _ref_wgrad, "attention-f32": _ref_attention(F32, 1e-4),
    "attention-bf16": _ref_attention(BF16, 2e-2), "attention-f16": _ref_attention(F16, 3e-3),
    "render-parity": _ref_render_parity, "render-oversized-bucket": _ref_render_oversized,
    "mesh-raster-hand_texture_40x72": _ref_mesh_raster("hand_texture_40x72"),
    "mesh-raster-boxes_33x47": _ref_mesh_raster("boxes_33x47"), "conv-fwd-dgrad": _ref_conv_fwd,
    "conv-wgrad": _ref_conv_wgrad, "gn-silu": _ref_gn_silu, "lpips-distance": _ref_lpips, "data-views": _ref_data,
    "mesh-density": _ref_mesh_density, "mesh-end-to-end": _ref_mesh_e2e, "mesh-sample": _ref_mesh_sample,
    "optimizer": _ref_optim,
}


@pytest.mark.parametrize("name", sorted(REFERENCE_CHECKS))
def test_reference_check_under_poison(cuda, oracle_mod, name):
    """An existing check, against its own fp64 reference and with its own bars, with every allocation poisoned with
    0xFF; the red zones intact afterwards."""
    with ending_the_session_on_a_gpu_fault(), guarded(0xFF) as g:
        REFERENCE_CHECKS[name](cuda, oracle_mod)
    print(f"{name} under 0xFF: {g.n_allocations} allocations, {g.n_bytes} bytes guarded, {g.zones_checked} red zones "
          f"checked, {len(g.violations)} violated")
    assert g.n_allocations >= 1
    g.assert_clean()


# ------------------------------------------------------------------------------------------------------ coverage
# Host-only entry points: they launch nothing and write no device memory, so there is nothing to poison.
HOST_ONLY = {
    "lgm_abi_version", "lgm_last_error",
    # sizes and bounds computed from the dimensions
    "lgm_render_workspace_size", "lgm_render_workspace_size_opts", "lgm_attn_workspace_size",
    "lgm_mva_workspace_size", "lgm_mva_backward_workspace_size", "lgm_gaussian_head_workspace_size",
    "lgm_linear_wgrad_workspace_size", "lgm_conv_wgrad_workspace_size", "lgm_conv_forward_workspace_size",
    "lgm_conv_dgrad_workspace_size", "lgm_gn_silu_workspace_size", "lgm_gn_silu_backward_workspace_size",
    "lgm_lpips_dist_workspace_size", "lgm_optim_workspace_size", "lgm_mesh_density_workspace_size",
    "lgm_mesh_sample_workspace_size", "lgm_mesh_extract_workspace_size", "lgm_meshraster_workspace_size",
    "lgm_render_det_flush_limit_log2", "lgm_meshraster_unit_log2",
    # the profiler (it is what watches the rows)
    "lgm_profiler_create", "lgm_profiler_summary", "lgm_profiler_reset", "lgm_profiler_destroy",
}
# (lgm_render_tile_lists, lgm_render_pixel_state, lgm_render_records and lgm_render_needle_flags take no diag and are
# reached through lib(), not nat.call: the float-mode render row calls them and records them by hand.)


def test_every_compute_entry_point_was_swept():
    assert HOST_ONLY <= set(nat.SIGNATURES)
    assert all(n in HOST_ONLY for n in nat.SIGNATURES if "_workspace_size" in n)
    all_rows = {p.id for p in ROWS}
    if RAN != all_rows:
        pytest.skip(f"{len(all_rows - RAN)} of {len(all_rows)} rows did not run in this session")
    missing = set(nat.SIGNATURES) - HOST_ONLY - SWEPT
    assert not missing, sorted(missing)
