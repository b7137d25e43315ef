"""The convolution forward and input gradient (include/lgm_conv.h, lgm_amd/csrc/conv_fwd.hip): exact-integer cases
against the fp64 convolution (equality), random cases against fp64 on the same 16-bit operands next to torch's own arm,
fp32 / 16-bit weights and bias, bias = NULL, alignment forms and the profiler labels. The argument checks run without a
GPU (nothing is launched on an error)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from lgm_amd import _native
from tests.test_conv_wgrad import CASES as WGRAD_CASES

CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
FLOOR = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}  # one output rounding
# (ksize, N, Cin, Cout, H, W): the weight gradient's list (1 x 1 images; padding along one axis only; rows shorter than a
# 16-byte group; 64-pixel planes; 9 / 14 channels; unaligned 10^2 rows; 136 -> 200 tile remainders; 64^2 planes; 130 x 20
# short rows; N = 0), a long K loop (35 K steps: split 8 ways) and Cin just past two K steps of 32
CASES = list(WGRAD_CASES) + [(3, 1, 1100, 72, 8, 8), (1, 3, 70, 8, 8, 8)]


def _p(v):
    return ctypes.c_void_p(v)


def _code(t, dt):
    return 0 if t is None else CODES[t.dtype]


def conv_forward(x, w, bias, ksize):
    """lgm_conv_forward into a NaN-filled output; x is a dense NCHW view (at any element of its storage)."""
    L = _native.lib()
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == Cin
    y = torch.full((N, Cout, H, W), float("nan"), device=x.device, dtype=x.dtype)
    ws_bytes = L.lgm_conv_forward_workspace_size(N, Cin, Cout, H, W, ksize)
    ws = torch.empty(max(ws_bytes, 1), device=x.device, dtype=torch.uint8)
    _native.check(L.lgm_conv_forward(CODES[x.dtype], CODES[w.dtype], N, Cin, Cout, H, W, ksize, _native.ptr(x),
                                     _native.ptr(w), _native.ptr(bias), _code(bias, x.dtype), _native.ptr(y),
                                     _native.ptr(ws), ws_bytes, _native.stream_of(x.device), _native.diag()),
                  "lgm_conv_forward")
    torch.cuda.synchronize()
    return y


def conv_dgrad(dy, w, ksize):
    L = _native.lib()
    N, Cout, H, W = dy.shape
    Cin = w.shape[1]
    assert dy.is_contiguous() and w.is_contiguous() and w.shape[0] == Cout
    dx = torch.full((N, Cin, H, W), float("nan"), device=dy.device, dtype=dy.dtype)
    ws_bytes = L.lgm_conv_dgrad_workspace_size(N, Cin, Cout, H, W, ksize)
    ws = torch.empty(max(ws_bytes, 1), device=dy.device, dtype=torch.uint8)
    _native.check(L.lgm_conv_dgrad(CODES[dy.dtype], CODES[w.dtype], N, Cin, Cout, H, W, ksize, _native.ptr(dy),
                                   _native.ptr(w), _native.ptr(dx), _native.ptr(ws), ws_bytes,
                                   _native.stream_of(dy.device), _native.diag()), "lgm_conv_dgrad")
    torch.cuda.synchronize()
    return dx


def truth(x, w, bias, dy, ksize):
    """fp64 on the CPU, on the same 16-bit operands: the forward, and the input gradient by autograd."""
    xx = x.detach().double().cpu().requires_grad_(True)
    ww = w.detach().double().cpu()
    y = F.conv2d(xx, ww, None if bias is None else bias.detach().double().cpu(), 1, (ksize - 1) // 2)
    y.backward(dy.detach().double().cpu())
    return y.detach(), xx.grad


def rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def operands(case, dtype, dev):
    ksize, N, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(2000 * ksize + 131 * N + 17 * Cin + 7 * Cout + 3 * H + W)
    x = torch.randn((N, Cin, H, W), generator=g).to(dev, dtype)
    dy = torch.randn((N, Cout, H, W), generator=g).to(dev, dtype)
    w = torch.randn((Cout, Cin, ksize, ksize), generator=g).to(dev, dtype)
    b = torch.randn((Cout,), generator=g).to(dev, dtype)
    return x, dy, w, b


def test_workspace_size_and_errors():
    L = _native.lib()
    fsize, dsize = L.lgm_conv_forward_workspace_size, L.lgm_conv_dgrad_workspace_size
    assert fsize(4, 64, 64, 32, 32, 3) > 0 and dsize(4, 64, 64, 32, 32, 3) > 0
    assert fsize(4, 1024, 1024, 8, 8, 3) > fsize(4, 64, 1024, 8, 8, 3)  # (the packed weight, and split partials)
    assert fsize(4, 64, 0, 32, 32, 3) == 0 and dsize(4, 0, 64, 32, 32, 3) == 0 and fsize(0, 64, 64, 32, 32, 3) == 0
    fake = _p(4096)  # never dereferenced: nothing is launched on an error

    def fwd(dtype=1, w_dtype=0, N=2, Cin=8, Cout=8, H=4, W=4, ksize=3, x=fake, w=fake, bias=None, bias_dtype=0, y=fake,
            ws=fake, ws_bytes=1 << 30):
        return L.lgm_conv_forward(dtype, w_dtype, N, Cin, Cout, H, W, ksize, x, w, bias, bias_dtype, y, ws, ws_bytes,
                                  None, None)

    def dgr(dtype=1, w_dtype=0, N=2, Cin=8, Cout=8, H=4, W=4, ksize=3, dy=fake, w=fake, dx=fake, ws=fake,
            ws_bytes=1 << 30):
        return L.lgm_conv_dgrad(dtype, w_dtype, N, Cin, Cout, H, W, ksize, dy, w, dx, ws, ws_bytes, None, None)

    for call, size, ops in ((fwd, fsize, ("x", "w", "y")), (dgr, dsize, ("dy", "w", "dx"))):
        assert call(dtype=0) < 0 and b"dtype" in L.lgm_last_error()  # fp32 activations: not this kernel
        assert call(dtype=3) < 0 and b"dtype" in L.lgm_last_error()
        assert call(w_dtype=2) < 0 and b"dtype" in L.lgm_last_error()  # fp16 weight, bf16 activations
        assert call(w_dtype=7) < 0 and b"dtype" in L.lgm_last_error()
        assert call(ksize=5) < 0 and b"ksize" in L.lgm_last_error()
        assert call(ksize=2) < 0 and b"ksize" in L.lgm_last_error()
        for neg in ("N", "Cin", "Cout", "H", "W"):
            assert call(**{neg: -1}) < 0 and b"negative" in L.lgm_last_error(), neg
        for nul in ops:
            assert call(**{nul: None}) < 0 and b"null" in L.lgm_last_error(), nul
        need = size(2, 8, 8, 4, 4, 3)
        assert need > 0
        assert call(ws_bytes=need - 1) < 0 and b"workspace" in L.lgm_last_error()
        assert call(ws=None) < 0 and b"workspace" in L.lgm_last_error()
        assert call(Cin=1 << 24, Cout=1 << 24) < 0 and b"2^31" in L.lgm_last_error()  # 2^37 weight tiles
        # nothing to do: rc 0 whatever the pointers
        nothing = {k: None for k in ops}
        assert call(N=0, ws=None, ws_bytes=0, **nothing) == 0
        assert call(H=0, ws=None, ws_bytes=0, **nothing) == 0
    assert fwd(bias=fake, bias_dtype=2) < 0 and b"dtype" in L.lgm_last_error()
    assert fwd(Cout=0, x=None, w=None, y=None, ws=None, ws_bytes=0) == 0
    assert dgr(Cin=0, dy=None, w=None, dx=None, ws=None, ws_bytes=0) == 0


# ---- exact-integer cases: operands in {-1, 0, 1}, bias in {-2 .. 2}; the reduction length * 1 + 2 stays inside the
# dtype's exact-integer range (bf16 256, f16 2048), so every product, partial sum and the rounded result are exact and
# the comparison with the fp64 convolution is equality. (dtype, ksize, reduction channels, other channels); the last
# row's 226 channels are 8 K steps: a two-way split.
EXACT = [(torch.bfloat16, 3, 28, 20), (torch.bfloat16, 1, 200, 20), (torch.float16, 3, 200, 20),
         (torch.float16, 3, 226, 72)]
SPATIAL = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 3, 5), (2, 10, 10), (3, 8, 8)]  # (N, H, W)


def _ints(shape, lo, hi, g, dev, dtype):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dev, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("spatial", SPATIAL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("row", EXACT, ids=lambda r: f"{str(r[0])[6:]}-k{r[1]}-{r[2]}")
def test_exact_integers(cuda, row, spatial):
    dtype, ksize, red, oth = row
    N, H, W = spatial
    assert red * ksize * ksize + 2 <= (256 if dtype == torch.bfloat16 else 2048)
    g = torch.Generator().manual_seed(red + 10 * H + W)
    # forward: Cin = red; input gradient: Cout = red
    x = _ints((N, red, H, W), -1, 1, g, cuda, dtype)
    w = _ints((oth, red, ksize, ksize), -1, 1, g, cuda, dtype)
    b = _ints((oth,), -2, 2, g, cuda, dtype)
    y = conv_forward(x, w, b, ksize)
    ry, _ = truth(x, w, b, torch.zeros((N, oth, H, W)), ksize)
    assert torch.equal(y.cpu(), ry.to(dtype)), float((y.double().cpu() - ry).abs().max())
    dy = _ints((N, red, H, W), -1, 1, g, cuda, dtype)
    wd = _ints((red, oth, ksize, ksize), -1, 1, g, cuda, dtype)
    dx = conv_dgrad(dy, wd, ksize)
    _, rdx = truth(torch.zeros((N, oth, H, W)), wd, None, dy, ksize)
    assert torch.equal(dx.cpu(), rdx.to(dtype)), float((dx.double().cpu() - rdx).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_one_pixel_image_outer_tap_sees_only_padding(cuda, dtype):
    """A 1 x 1 image and a weight that is one-hot at an outer tap: the output is exactly the bias (the input gradient
    exactly zero)."""
    for tap in ((0, 0), (0, 1), (2, 2), (1, 0)):
        x = torch.ones((3, 8, 1, 1), device=cuda, dtype=dtype)
        w = torch.zeros((8, 8, 3, 3), device=cuda, dtype=dtype)
        w[:, :, tap[0], tap[1]] = 1
        b = torch.arange(-2, 6, device=cuda).to(dtype)
        y = conv_forward(x, w, b, 3)
        assert torch.equal(y, b.view(1, 8, 1, 1).expand(3, 8, 1, 1)), tap
        assert torch.all(conv_dgrad(x, w, 3) == 0), tap


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d-" % c[0] + "x".join(map(str, c[1:])))
def test_conv_forward_and_dgrad_vs_fp64(cuda, case, dtype):
    """Forward and input gradient vs fp64 on the same 16-bit operands: the rel-L2 error at most max(2 x the error of
    torch's arm on the same GPU, one output rounding); NaN-filled outputs come back finite; two calls are bitwise
    equal."""
    ksize, N = case[0], case[1]
    x, dy, w, b = operands(case, dtype, cuda)
    y, dx = conv_forward(x, w, b, ksize), conv_dgrad(dy, w, ksize)
    y2, dx2 = conv_forward(x, w, b, ksize), conv_dgrad(dy, w, ksize)
    assert y.shape == dy.shape and dx.shape == x.shape
    if N == 0:
        return
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    ry, rdx = truth(x, w, b, dy, ksize)
    pad = (ksize - 1) // 2
    ty = F.conv2d(x, w, b, 1, pad)
    tdx = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1,
                                              [True, False, False])[0]
    for name, mine, theirs, ref in (("y", y, ty, ry), ("dx", dx, tdx, rdx)):
        e, et = rel(mine, ref), rel(theirs, ref)
        bar = max(2 * et, FLOOR[dtype])
        print(f"conv_fwd {case} {dtype} {name}: rel L2 kernel {e:.3e}, torch {et:.3e}, bar {bar:.3e}")
        assert e <= bar, (name, e, et)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(3, 2, 24, 40, 10, 10), (1, 2, 70, 24, 8, 8), (3, 1, 1100, 72, 8, 8)],
                         ids=["3x3", "1x1", "split"])
def test_fp32_weight_and_bias_and_null_bias(cuda, case):
    """fp32 weight / bias give the bits of the same call on their .to(dt) casts (the packing pass rounds as torch does);
    bias = NULL gives the bits of a zero bias."""
    ksize = case[0]
    for dtype in (torch.bfloat16, torch.float16):
        x, dy, _, _ = operands(case, dtype, cuda)
        g = torch.Generator().manual_seed(9)
        w32 = torch.randn((case[3], case[2], ksize, ksize), generator=g).to(cuda)
        b32 = torch.randn((case[3],), generator=g).to(cuda)
        y16 = conv_forward(x, w32.to(dtype), b32.to(dtype), ksize)
        assert torch.equal(conv_forward(x, w32, b32, ksize), y16)
        assert torch.equal(conv_forward(x, w32, b32.to(dtype), ksize), y16)
        assert torch.equal(conv_forward(x, w32.to(dtype), b32, ksize), y16)
        assert torch.equal(conv_dgrad(dy, w32, ksize), conv_dgrad(dy, w32.to(dtype), ksize))
        assert torch.equal(conv_forward(x, w32, None, ksize), conv_forward(x, w32, torch.zeros_like(b32), ksize))
        assert not torch.equal(conv_forward(x, w32, None, ksize), y16)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(3, 2, 16, 16, 16, 16), (3, 1, 8, 24, 8, 32)], ids=["2x16x16x16x16", "1x8x24x8x32"])
def test_alignment_forms_bitwise(cuda, case):
    """The same data at 16-byte aligned bases and in views one element into a flat buffer (x, dy and the 16-bit w
    shifted independently): bitwise equal outputs, and right."""
    ksize = case[0]
    x0, dy0, w0, b0 = operands(case, torch.bfloat16, cuda)

    def shifted(t, by):
        flat = torch.zeros(t.numel() + 8, device=t.device, dtype=t.dtype)
        v = flat[by:by + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 2 * by and v.is_contiguous()
        return v

    ys = [conv_forward(shifted(x0, a), shifted(w0, b), b0, ksize) for a in (0, 1) for b in (0, 1)]
    dxs = [conv_dgrad(shifted(dy0, a), shifted(w0, b), ksize) for a in (0, 1) for b in (0, 1)]
    ry, rdx = truth(x0, w0, b0, dy0, ksize)
    assert rel(ys[0], ry) < 2.0 ** -8 and rel(dxs[0], rdx) < 2.0 ** -8
    for y, dx in zip(ys[1:], dxs[1:]):
        assert torch.equal(y, ys[0]) and torch.equal(dx, dxs[0])


@pytest.mark.gpu
def test_profiler_labels(cuda):
    """k_conv_wpack and k_conv_fwd / k_conv_dgrad once per call, k_conv_fwd_reduce once more where the K range is split;
    nothing on an rc < 0 call."""
    L = _native.lib()
    prof = _native.KernelProfiler()
    x, dy, w, b = operands((3, 2, 24, 40, 10, 10), torch.bfloat16, cuda)
    with prof:
        conv_forward(x, w, b, 3)
    ran = prof.summary()
    assert {k: v[0] for k, v in ran.items()} == {"k_conv_wpack": 1, "k_conv_fwd": 1}, ran
    prof.reset()
    with prof:
        conv_dgrad(dy, w, 3)
        rc = L.lgm_conv_dgrad(1, 1, 2, 24, 40, 10, 10, 4, _native.ptr(dy), _native.ptr(w), _native.ptr(x), None, 0,
                              _native.stream_of(cuda), _native.diag())
        assert rc < 0
        rc = L.lgm_conv_forward(1, 1, 2, 24, 40, 10, 10, 3, _native.ptr(x), _native.ptr(w), None, 0, _native.ptr(dy), None,
                                0, _native.stream_of(cuda), _native.diag())
        assert rc < 0 and b"workspace" in L.lgm_last_error()
    ran = prof.summary()
    assert {k: v[0] for k, v in ran.items()} == {"k_conv_wpack": 1, "k_conv_dgrad": 1}, ran
    prof.reset()
    x, dy, w, b = operands((3, 1, 1100, 72, 8, 8), torch.bfloat16, cuda)
    with prof:
        conv_forward(x, w, b, 3)
    ran = prof.summary()
    prof.close()
    assert {k: v[0] for k, v in ran.items()} == {"k_conv_wpack": 1, "k_conv_fwd": 1, "k_conv_fwd_reduce": 1}, ran
