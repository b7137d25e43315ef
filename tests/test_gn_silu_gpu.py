"""The fused GroupNorm + SiLU (+ resample) kernels (include/lgm_norm.h, lgm_amd/csrc/gnsilu.hip) against an fp64 CPU
evaluation of the formulas of the header, with torch's own ops (F.group_norm -> F.silu -> resample and autograd
through them, same inputs, dtypes and GPU) measured next to them.

Bars: the kernel's rel-L2 error against fp64 must be <= max(2 x torch's error, floor); the floor is one output
rounding: 2^-9 for bf16 results, 2^-11 for f16 results, 1e-6 for fp32 results (dgamma / dbeta are fp32 results).
torch is itself one correct fp32 implementation with another summation order: two such differ by a factor of order one.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from lgm_amd import _native as nat
from lgm_amd._native import DTYPE_CODES as _DTYPES
from lgm_amd.unet import group_norm_silu

pytestmark = pytest.mark.gpu

NONE, UP2, DOWN2 = 0, 1, 2
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FLOOR = {F32: 1e-6, BF16: 2.0 ** -9, F16: 2.0 ** -11}

# the dispatch thresholds of gnsilu.hip, and the shapes that sit on either side of them
GNS_CHUNK, GNS_SLAB_MAX, GNS_FILL = 4096, 8192, 256


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def resample_t(a, rs):
    if rs == UP2:
        return F.interpolate(a, scale_factor=2.0, mode="nearest")
    if rs == DOWN2:
        return F.avg_pool2d(a, kernel_size=2, stride=2)
    return a


def reference64(x, gamma, beta, G, eps, rs, dy):
    """fp64 on the CPU: y, dx, dgamma, dbeta of the header's formulas for the given (already rounded) inputs."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    N, C, H, W = x64.shape
    g64 = (torch.ones(C, dtype=torch.float64) if gamma is None else gamma.detach().double().cpu()).requires_grad_(True)
    b64 = (torch.zeros(C, dtype=torch.float64) if beta is None else beta.detach().double().cpu()).requires_grad_(True)
    xr = x64.reshape(N, G, -1)
    mean = xr.mean(-1, keepdim=True)
    var = ((xr - mean) ** 2).mean(-1, keepdim=True)  # biased
    z = ((xr - mean) / torch.sqrt(var + eps)).reshape(N, C, H, W) * g64.view(1, C, 1, 1) + b64.view(1, C, 1, 1)
    y = resample_t(z * torch.sigmoid(z), rs)
    dx, dg, db = torch.autograd.grad(y, [x64, g64, b64], dy.detach().double().cpu())
    return y.detach(), dx, dg, db


def torch_ops(x, gamma, beta, G, eps, rs, dy, y_dtype):
    """torch's own ops on the GPU in the same dtypes (the parameters take x's dtype: the test's values are exactly
    representable in all three), rounded to y_dtype where that differs."""
    xt = x.detach().clone().requires_grad_(True)
    gt = None if gamma is None else gamma.detach().to(x.dtype).requires_grad_(True)
    bt = None if beta is None else beta.detach().to(x.dtype).requires_grad_(True)
    y = resample_t(F.silu(F.group_norm(xt, G, gt, bt, eps)), rs).to(y_dtype)
    wrt = [xt] + ([gt, bt] if gamma is not None else [])
    grads = torch.autograd.grad(y, wrt, dy)
    return y.detach(), grads[0], (grads[1] if gamma is not None else None), (grads[2] if gamma is not None else None)


def out_shape(N, C, H, W, rs):
    return (N, C, 2 * H, 2 * W) if rs == UP2 else (N, C, H // 2, W // 2) if rs == DOWN2 else (N, C, H, W)


def kernel_forward(x, gamma, beta, G, eps, rs, y_dtype, ws_bytes=None):
    """lgm_gn_silu_forward through the C ABI -> (rc, y, mean, rstd)."""
    N, C, H, W = x.shape
    L = nat.lib()
    y = torch.empty(out_shape(N, C, H, W, rs), device=x.device, dtype=y_dtype)
    mean = torch.empty(N, G, device=x.device)
    rstd = torch.empty(N, G, device=x.device)
    need = L.lgm_gn_silu_workspace_size(N, C, H, W, G)
    ws = torch.empty(max(need, 1), device=x.device, dtype=torch.uint8)
    rc = L.lgm_gn_silu_forward(_DTYPES[x.dtype], _DTYPES[y_dtype], N, C, H, W, G, eps, rs, nat.ptr(x), nat.ptr(gamma),
                               nat.ptr(beta), nat.ptr(y), nat.ptr(mean), nat.ptr(rstd), nat.ptr(ws),
                               need if ws_bytes is None else ws_bytes, nat.stream_of(x.device), nat.diag())
    return rc, y, mean, rstd


def kernel_backward(x, gamma, beta, G, rs, mean, rstd, dy, want=(True, True, True), ws_bytes=None):
    """lgm_gn_silu_backward through the C ABI -> (rc, dx, dgamma, dbeta); want: which of the three are not NULL."""
    N, C, H, W = x.shape
    L = nat.lib()
    dx = torch.empty_like(x) if want[0] else None
    dg = torch.empty(C, device=x.device) if want[1] else None
    db = torch.empty(C, device=x.device) if want[2] else None
    need = L.lgm_gn_silu_backward_workspace_size(N, C, H, W, G)
    ws = torch.empty(max(need, 1), device=x.device, dtype=torch.uint8)
    rc = L.lgm_gn_silu_backward(_DTYPES[x.dtype], _DTYPES[dy.dtype], N, C, H, W, G, rs, nat.ptr(x), nat.ptr(gamma),
                                nat.ptr(beta), nat.ptr(mean), nat.ptr(rstd), nat.ptr(dy), nat.ptr(dx), nat.ptr(dg),
                                nat.ptr(db), nat.ptr(ws), need if ws_bytes is None else ws_bytes,
                                nat.stream_of(x.device), nat.diag())
    return rc, dx, dg, db


def make_inputs(cuda, N, C, H, W, G, rs, xdt, ydt, seed=0, kind="randn", affine=True, misalign=False):
    gen = torch.Generator().manual_seed(seed)
    n = N * C * H * W
    base = torch.randn(n + (1 if misalign else 0), generator=gen)
    if kind == "mean100":
        base = base + 100.0
    elif kind == "tiny":
        base = base * 1e-3
    else:
        base = base * 1.5 + 0.25
    base = base.to(cuda).to(xdt)
    x = (base[1:] if misalign else base).view(N, C, H, W)  # misalign: contiguous, data pointer off by one element
    assert x.is_contiguous() and (not misalign or x.data_ptr() % 16 != 0)
    # parameters exactly representable in bf16 and f16 (multiples of 1/8)
    gamma = (torch.randint(-12, 13, (C,), generator=gen).float() / 8).to(cuda) if affine else None
    beta = (torch.randint(-8, 9, (C,), generator=gen).float() / 8).to(cuda) if affine else None
    dy = torch.randn(out_shape(N, C, H, W, rs), generator=gen).to(cuda).to(ydt)
    return x, gamma, beta, dy


def check_case(cuda, N, C, H, W, G, rs, xdt, ydt, kernels=None, eps=1e-5, **kw):
    x, gamma, beta, dy = make_inputs(cuda, N, C, H, W, G, rs, xdt, ydt, **kw)
    prof = nat.KernelProfiler()
    with prof:
        rc, y, mean, rstd = kernel_forward(x, gamma, beta, G, eps, rs, ydt)
        assert rc == 0, nat.lib().lgm_last_error()
        rc, dx, dg, db = kernel_backward(x, gamma, beta, G, rs, mean, rstd, dy)
        assert rc == 0, nat.lib().lgm_last_error()
    ran = set(prof.summary())
    prof.close()
    if kernels is not None:
        assert {k for k in ran if k.startswith("k_gns_")} == set(kernels), sorted(ran)
    ry, rdx, rdg, rdb = reference64(x, gamma, beta, G, eps, rs, dy)
    ty, tdx, tdg, tdb = torch_ops(x, gamma, beta, G, eps, rs, dy, ydt)
    rows = [("y", y, ty, ry, FLOOR[ydt]), ("dx", dx, tdx, rdx, FLOOR[xdt]),
            ("dgamma", dg, tdg, rdg, FLOOR[F32]), ("dbeta", db, tdb, rdb, FLOOR[F32])]
    bad = []
    for name, mine, theirs, ref, floor in rows:
        assert torch.isfinite(mine.float()).all(), name
        e_k = rel(mine, ref)
        e_t = rel(theirs, ref) if theirs is not None else float("nan")
        bar = max(2 * e_t, floor) if theirs is not None else floor
        print(f"gn_silu N{N} C{C} G{G} {H}x{W} rs{rs} {str(xdt)[6:]}->{str(ydt)[6:]} {kw} {name}: kernel {e_k:.3e} "
              f"torch {e_t:.3e} ratio {e_k / max(e_t, 1e-300):.2f} bar {bar:.3e}")
        if not e_k <= bar:
            bad.append((name, e_k, e_t, bar))
    # the saved statistics
    xr = x.detach().double().cpu().reshape(N, G, -1)
    m64 = xr.mean(-1)
    r64 = 1 / torch.sqrt(((xr - m64[..., None]) ** 2).mean(-1) + eps)
    assert rel(rstd, r64) < 1e-5 and float((mean.double().cpu() - m64).abs().max()) <= 1e-6 * float(
        xr.abs().max()) + 1e-7
    assert not bad, bad


DT_PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (F32, BF16)]
SMALL = [  # N, C, G, H, W, resamples
    (1, 32, 32, 2, 2, (NONE, UP2, DOWN2)),   # Cg = 1, 4 elements per group; DOWN2 -> 1 x 1
    (2, 96, 32, 6, 10, (NONE, UP2, DOWN2)),  # Cg = 3; rows of 10 are no 16-byte multiple at 16 bits
    (3, 64, 32, 5, 7, (NONE, UP2)),          # odd sizes (DOWN2: see test_odd_down2)
    (2, 40, 8, 4, 4, (NONE, UP2, DOWN2)),    # Cg = 5, groups != 32
]


@pytest.mark.parametrize("xdt,ydt", DT_PAIRS, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "N%d_C%d_G%d_%dx%d" % s[:5])
def test_small_shapes(cuda, shape, xdt, ydt):
    N, C, G, H, W, resamples = shape
    for rs in resamples:
        check_case(cuda, N, C, H, W, G, rs, xdt, ydt)


def test_odd_down2(cuda):
    """(N3, C64, G32, 5x7) with DOWN2: rc < 0 at the ABI, torch's result at the module level."""
    x, gamma, beta, _ = make_inputs(cuda, 3, 64, 5, 7, 32, NONE, F32, F32)
    rc, *_ = kernel_forward(x, gamma, beta, 32, 1e-5, DOWN2, F32)
    assert rc < 0 and b"even" in nat.lib().lgm_last_error()
    norm = nn.GroupNorm(32, 64).to(cuda)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    prof = nat.KernelProfiler()
    with prof:
        y = group_norm_silu(x, norm, "down")
    assert not prof.summary()
    prof.close()
    assert torch.equal(y, F.avg_pool2d(F.silu(norm(x)), 2, 2)) and y.shape == (3, 64, 2, 3)


def test_misaligned_pointer(cuda):
    """(N2, C4, G4, 1x3) bf16, x = base[1:]: contiguous, data pointer not 16-byte aligned -> the scalar forms."""
    for rs in (NONE, UP2):
        check_case(cuda, 2, 4, 1, 3, 4, rs, BF16, BF16, misalign=True, kernels=kernel_names("slab", "s16"))
    # a shape the vector forms would take, were the pointer aligned; and the module on the same tensor
    check_case(cuda, 2, 8, 4, 8, 4, DOWN2, BF16, BF16, misalign=True, kernels=kernel_names("slab", "s16"))
    x, gamma, beta, dy = make_inputs(cuda, 2, 8, 4, 8, 4, NONE, BF16, BF16, misalign=True)
    norm = nn.GroupNorm(4, 8).to(cuda)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    xa = x.detach().requires_grad_(True)
    y = group_norm_silu(xa, norm)
    ry, rdx, _, _ = reference64(x, gamma, beta, 4, norm.eps, NONE, dy)
    dxa, = torch.autograd.grad(y, xa, dy)
    assert rel(y, ry) < 2.0 ** -8 and rel(dxa, rdx) < 2.0 ** -8


def kernel_names(family, form):
    """The kernels one forward + backward launches: family 'slab' (one forward launch) or 'chunk' (statistics, then
    normalise); form 'v' / 's' (vector / scalar accesses) followed by the team of the elementwise passes: '16' or '64'
    lanes per plane, nothing for the whole 256-thread workgroup."""
    fwd = ["k_gns_slab_" + form[0]] if family == "slab" else ["k_gns_stats_" + form[0], "k_gns_norm_" + form]
    return fwd + ["k_gns_bwd_part_" + form, "k_gns_bwd_coef", "k_gns_bwd_dx_" + form]


# N, C, G, H, W, rs, family, form[, misaligned]. n = (C / G) H W elements per group.
# Forward: the one-launch slab form runs when n <= GNS_SLAB_MAX and (n <= GNS_CHUNK or N G >= GNS_FILL), else the
# chunked form (ceil(n / GNS_CHUNK) chunks).
# Vector forms: 16-byte aligned tensors and H W % 4 == 0 (NONE), W % 4 == 0 (UP2), W % 8 == 0 (DOWN2).
# Teams of the elementwise passes, by the items of a plane (vector: H W / 4, H (W / 4), (H / 2) (W / 8); scalar: H W,
# H W, (H / 2) (W / 2)): <= 64 items: 16 lanes; <= 256: 64 lanes; more: the workgroup.
THRESHOLDS = [
    (1, 32, 32, 1, GNS_CHUNK, NONE, "slab", "v"),           # n = one chunk, 32 workgroups: slab
    (1, 32, 32, 1, GNS_CHUNK + 4, NONE, "chunk", "v"),      # just past one chunk, chip not filled: 2 chunks, vector
    (1, 32, 32, 1, GNS_CHUNK + 1, NONE, "chunk", "s"),      # ... and the scalar forms (H W % 4 != 0)
    (7, 32, 32, 1, GNS_SLAB_MAX, NONE, "chunk", "v"),       # N G = 224 < GNS_FILL: chunked although the slab would fit
    (8, 32, 32, 1, GNS_SLAB_MAX, NONE, "slab", "v"),        # N G = 256 = GNS_FILL, n = GNS_SLAB_MAX: slab
    (8, 32, 32, 1, GNS_SLAB_MAX + 1, NONE, "chunk", "s"),   # n just past the slab: 3 chunks, the last of 1 element
    (8, 32, 32, 1, GNS_SLAB_MAX + 4, NONE, "chunk", "v"),   # ... 3 chunks, the last of 4 elements; 3 tiles per plane
    (2, 8, 4, 48, 44, NONE, "chunk", "v"),                  # Cg = 2: a group's 2 chunks straddle its two planes
    (2, 8, 4, 4, 8, UP2, "slab", "v16"), (2, 8, 4, 4, 6, UP2, "slab", "s16"),      # W % 4 == 0 / != 0
    (2, 8, 4, 4, 8, DOWN2, "slab", "v16"), (2, 8, 4, 4, 12, DOWN2, "slab", "s16"),  # W % 8 == 0 / != 0
    (1, 8, 4, 48, 48, UP2, "chunk", "v"), (1, 8, 4, 48, 46, UP2, "chunk", "s"),
    (1, 8, 4, 48, 48, DOWN2, "chunk", "v64"), (1, 8, 4, 48, 44, DOWN2, "chunk", "s"),  # 144 items; 528 items
    # team thresholds, vector forms: 64 | 65 items (16 x 16, 10 x 26) and 256 | 257 items (32 x 32, 4 x 257) ...
    (2, 8, 4, 16, 16, NONE, "slab", "v16"), (2, 8, 4, 10, 26, NONE, "slab", "v64"),
    (2, 8, 4, 32, 32, NONE, "slab", "v64"), (2, 8, 4, 4, 257, NONE, "slab", "v"),
    # ... the same under the chunked forward (one group of 64 / 16 channels: n > GNS_SLAB_MAX)
    (1, 64, 1, 16, 16, NONE, "chunk", "v16"), (1, 64, 1, 10, 26, NONE, "chunk", "v64"),
    (1, 16, 1, 32, 32, NONE, "chunk", "v64"), (1, 16, 1, 4, 257, NONE, "chunk", "v"),
    # ... and scalar forms: 63 | 64 (misaligned pointer) | 65 items, 255 | 256 (misaligned) | 257 items
    (1, 96, 1, 7, 9, NONE, "chunk", "s16"), (1, 96, 1, 8, 8, NONE, "chunk", "s16", True),
    (1, 96, 1, 5, 13, NONE, "chunk", "s64"), (1, 32, 1, 15, 17, NONE, "chunk", "s64"),
    (1, 32, 1, 16, 16, NONE, "chunk", "s64", True), (1, 32, 1, 1, 257, NONE, "chunk", "s"),
]


@pytest.mark.parametrize("case", THRESHOLDS, ids=lambda c: "N%d_C%d_G%d_%dx%d_rs%d_%s_%s" % c[:8] + ("_mis" if len(c) > 8 else ""))
def test_dispatch_thresholds(cuda, case):
    N, C, G, H, W, rs, family, form = case[:8]
    mis = len(case) > 8
    check_case(cuda, N, C, H, W, G, rs, F32, F32, kernels=kernel_names(family, form), misalign=mis)
    if (family, form[0]) in (("chunk", "v"), ("slab", "s")):
        check_case(cuda, N, C, H, W, G, rs, F32, BF16, kernels=kernel_names(family, form), misalign=mis)


@pytest.mark.parametrize("kind", ["mean100", "tiny"])
@pytest.mark.parametrize("shape", [(2, 96, 32, 6, 10), (1, 8, 4, 48, 44)], ids=["slab", "chunked"])
def test_large_mean_and_eps_dominated(cuda, shape, kind):
    """x = 100 + randn: a cancelling variance formula fails here; x = 1e-3 randn: eps dominates the variance."""
    N, C, G, H, W = shape
    for rs in (NONE, DOWN2):
        check_case(cuda, N, C, H, W, G, rs, F32, F32, kind=kind)
    check_case(cuda, N, C, H, W, G, NONE, F32, BF16, kind=kind)


def test_no_affine_and_null_outputs(cuda):
    check_case(cuda, 2, 40, 4, 4, 8, UP2, F32, F32, affine=False)
    check_case(cuda, 1, 8, 48, 44, 4, NONE, BF16, BF16, affine=False)
    x, gamma, beta, dy = make_inputs(cuda, 2, 96, 6, 10, 32, DOWN2, F32, F32)
    rc, y, mean, rstd = kernel_forward(x, gamma, beta, 32, 1e-5, DOWN2, F32)
    assert rc == 0
    rc, dx, dg, db = kernel_backward(x, gamma, beta, 32, DOWN2, mean, rstd, dy)
    assert rc == 0
    for want in [(True, False, False), (False, True, False), (False, False, True), (False, True, True),
                 (False, False, False)]:
        rc, dx2, dg2, db2 = kernel_backward(x, gamma, beta, 32, DOWN2, mean, rstd, dy, want=want)
        assert rc == 0
        for a, b in ((dx, dx2), (dg, dg2), (db, db2)):
            assert b is None or torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2, 96, 32, 6, 10, UP2), (7, 32, 32, 1, GNS_SLAB_MAX, NONE),
                                   (1, 8, 4, 48, 48, DOWN2)], ids=["slab", "chunked", "chunked_down"])
def test_bitwise_reproducible(cuda, shape):
    N, C, G, H, W, rs = shape
    x, gamma, beta, dy = make_inputs(cuda, N, C, H, W, G, rs, F32, BF16)
    runs = []
    for _ in range(2):
        rc, y, mean, rstd = kernel_forward(x, gamma, beta, G, 1e-5, rs, BF16)
        assert rc == 0
        rc, dx, dg, db = kernel_backward(x, gamma, beta, G, rs, mean, rstd, dy)
        assert rc == 0
        runs.append((y, mean, rstd, dx, dg, db))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_errors_are_reported_not_launched(cuda):
    L = nat.lib()
    x, gamma, beta, dy = make_inputs(cuda, 1, 8, 48, 44, 4, NONE, F32, F32)
    prof = nat.KernelProfiler()
    with prof:
        # C % groups != 0
        rc = L.lgm_gn_silu_forward(0, 0, 1, 8, 48, 44, 3, 1e-5, 0, nat.ptr(x), None, None, nat.ptr(x), nat.ptr(x),
                                   nat.ptr(x), None, 0, None, None)
        assert rc < 0 and b"multiple of groups" in L.lgm_last_error()
        # a grid beyond the launch limits (2^31 - 1 workgroups): sizes only, nothing is read
        rc = L.lgm_gn_silu_forward(0, 0, 1 << 20, 1 << 12, 64, 64, 32, 1e-5, 0, None, None, None, None, None, None,
                                   None, 0, None, None)
        assert rc < 0 and b"grid" in L.lgm_last_error()
        rc = L.lgm_gn_silu_backward(0, 0, 1 << 20, 1 << 12, 64, 64, 32, 0, None, None, None, None, None, None,
                                    nat.ptr(x), None, None, None, 0, None, None)
        assert rc < 0 and b"grid" in L.lgm_last_error()
        # unsupported dtype pair (bf16 x, f16 y), bad resample
        rc = L.lgm_gn_silu_forward(1, 2, 1, 8, 4, 4, 4, 1e-5, 0, None, None, None, None, None, None, None, 0, None, None)
        assert rc < 0 and b"dtype" in L.lgm_last_error()
        rc = L.lgm_gn_silu_forward(0, 0, 1, 8, 4, 4, 4, 1e-5, 3, None, None, None, None, None, None, None, 0, None, None)
        assert rc < 0 and b"resample" in L.lgm_last_error()
        # workspace too small (the chunked form needs one; the backward always does)
        need = L.lgm_gn_silu_workspace_size(1, 8, 48, 44, 4)
        assert need == 1 * 4 * 2 * 8
        rc, *_ = kernel_forward(x, gamma, beta, 4, 1e-5, NONE, F32, ws_bytes=need - 1)
        assert rc < 0 and b"workspace" in L.lgm_last_error()
        rc, y, mean, rstd = kernel_forward(x, gamma, beta, 4, 1e-5, NONE, F32)
        assert rc == 0
        ran = prof.summary()
        prof.reset()
        assert set(ran) == {"k_gns_stats_v", "k_gns_norm_v"} and all(v[0] == 1 for v in ran.values()), ran
        rc, *_ = kernel_backward(x, gamma, beta, 4, NONE, mean, rstd, dy, ws_bytes=64)
        assert rc < 0 and b"workspace" in L.lgm_last_error()
        assert not prof.summary()
    prof.close()
    assert L.lgm_gn_silu_workspace_size(8, 32, 1, GNS_SLAB_MAX, 32) == 0  # the slab form needs none
    assert L.lgm_gn_silu_backward_workspace_size(1, 8, 48, 44, 4) >= 8 * 3 * 8 + 8 * 8 + 4 * 8


def test_module_autocast_dtype_and_grads(cuda):
    """group_norm_silu: the output takes the autocast dtype; parameter gradients come back in the parameters' dtype;
    and the values equal torch's fp32 chain rounded once (what the next conv's cast does)."""
    torch.manual_seed(0)
    norm = nn.GroupNorm(32, 96).to(cuda)
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.3, 0.3)
    x = torch.randn(2, 96, 6, 8, device=cuda)
    for resample in (None, "up", "down"):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ya = group_norm_silu(xa, norm, resample)
            yb = F.silu(norm(xb))
            yb = resample_t(yb, {None: NONE, "up": UP2, "down": DOWN2}[resample])
        assert ya.dtype == torch.bfloat16 and yb.dtype == torch.float32
        assert rel(ya, yb) < 2.0 ** -8
        g = torch.randn_like(yb)
        norm.zero_grad()
        ya.backward(g.to(ya.dtype))
        ga = (xa.grad, norm.weight.grad.clone(), norm.bias.grad.clone())
        norm.zero_grad()
        yb.backward(g.to(torch.bfloat16).float())
        for a, b in zip(ga, (xb.grad, norm.weight.grad, norm.bias.grad)):
            assert a.dtype == torch.float32 and rel(a, b) < 1e-4
    assert group_norm_silu(x, norm).dtype == torch.float32
