"""The convolution weight / bias gradient (include/lgm_conv.h, lgm_amd/csrc/conv_wgrad.hip) against fp64 on the same
16-bit operands: every border, short-plane and tail case of the kernel, both staging forms, db = NULL and the profiler
labels. The argument checks run without a GPU (nothing is launched on an error)."""
import ctypes

import pytest
import torch

from lgm_amd import _native

CODES = {torch.bfloat16: 1, torch.float16: 2}
# (N, Cin, Cout, H, W): only the centre tap is non-zero; zero padding along one axis only (both ways); rows shorter
# than one 16-byte group; 64-pixel planes (a stage spans planes and samples); conv_in's / conv_out's channel counts;
# cfg4's 10^2 level (unaligned rows, channels below one tile); more than one tile with a remainder in both channel
# dimensions; K = 8,192 (many stages, real splits); many short rows; N = 0 (zeros written)
CASES_3 = [(1, 8, 8, 1, 1), (1, 8, 8, 1, 9), (1, 8, 8, 9, 1), (2, 8, 16, 3, 5), (3, 16, 8, 8, 8), (3, 9, 14, 8, 8),
           (2, 24, 40, 10, 10), (1, 136, 200, 16, 16), (2, 64, 64, 64, 64), (1, 8, 8, 130, 20), (0, 8, 8, 4, 4)]
# small unaligned planes with channels below one tile; a full tile in Cin and half a tile in Cout
CASES_1 = [(2, 24, 40, 5, 7), (1, 128, 64, 16, 16)]
CASES = [(3,) + c for c in CASES_3] + [(1,) + c for c in CASES_1]


def _p(v):
    return ctypes.c_void_p(v)


def conv_wgrad(dy, x, ksize, want_db=True):
    """lgm_conv_wgrad into NaN-filled outputs; dy / x are dense NCHW views (at any element of their storage)."""
    L = _native.lib()
    N, Cout, H, W = dy.shape
    Cin = x.shape[1]
    assert dy.is_contiguous() and x.is_contiguous()
    dw = torch.full((Cout, Cin, ksize, ksize), float("nan"), device=dy.device)
    db = torch.full((Cout,), float("nan"), device=dy.device) if want_db else None
    ws_bytes = L.lgm_conv_wgrad_workspace_size(N, Cin, Cout, H, W, ksize, int(want_db))
    ws = torch.empty(max(ws_bytes, 1), device=dy.device, dtype=torch.uint8)
    _native.check(L.lgm_conv_wgrad(CODES[dy.dtype], N, Cin, Cout, H, W, ksize, _native.ptr(dy), _native.ptr(x),
                                   _native.ptr(dw), _native.ptr(db), _native.ptr(ws), ws_bytes,
                                   _native.stream_of(dy.device), _native.diag()), "lgm_conv_wgrad")
    torch.cuda.synchronize()
    return dw, db


def truth(dy, x, ksize):
    """fp64 on the CPU, on the same 16-bit operands."""
    d, xx = dy.detach().double().cpu(), x.detach().double().cpu()
    Cout, Cin = d.shape[1], xx.shape[1]
    rw = torch.nn.grad.conv2d_weight(xx, (Cout, Cin, ksize, ksize), d, stride=1, padding=(ksize - 1) // 2)
    return rw, d.sum((0, 2, 3))


def rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def operands(case, dtype, dev):
    ksize, N, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(1000 * ksize + 131 * N + 17 * Cin + 7 * Cout + 3 * H + W)
    dy = torch.randn((N, Cout, H, W), generator=g).to(dev, dtype)
    x = torch.randn((N, Cin, H, W), generator=g).to(dev, dtype)
    return dy, x


def test_workspace_size_and_errors():
    L = _native.lib()
    size = L.lgm_conv_wgrad_workspace_size
    assert size(4, 64, 64, 32, 32, 3, 0) > 0
    assert size(4, 64, 64, 32, 32, 3, 1) > size(4, 64, 64, 32, 32, 3, 0)
    assert size(4, 64, 0, 32, 32, 3, 1) == 0
    fake = _p(4096)  # never dereferenced: nothing is launched on an error

    def call(dtype=1, N=2, Cin=8, Cout=8, H=4, W=4, ksize=3, dy=fake, x=fake, dw=fake, db=None, ws=fake, ws_bytes=1 << 30):
        return L.lgm_conv_wgrad(dtype, N, Cin, Cout, H, W, ksize, dy, x, dw, db, ws, ws_bytes, None, None)

    assert call(dtype=0) < 0 and b"dtype" in L.lgm_last_error()  # fp32: not this kernel
    assert call(ksize=5) < 0 and b"ksize" in L.lgm_last_error()
    assert call(ksize=2) < 0 and b"ksize" in L.lgm_last_error()
    for neg in ("N", "Cin", "Cout", "H", "W"):
        assert call(**{neg: -1}) < 0 and b"negative" in L.lgm_last_error(), neg
    for nul in ("dy", "x", "dw"):
        assert call(**{nul: None}) < 0 and b"null" in L.lgm_last_error(), nul
    need = size(2, 8, 8, 4, 4, 3, 0)
    assert call(ws_bytes=need - 1) < 0 and b"workspace" in L.lgm_last_error()
    assert call(ws=None) < 0 and b"workspace" in L.lgm_last_error()
    assert call(Cin=1 << 24, Cout=1 << 24) < 0 and b"2^31" in L.lgm_last_error()  # 2^36 output tiles
    # nothing to do: rc 0 whatever the pointers
    assert call(Cin=0, dy=None, x=None, dw=None, ws=None, ws_bytes=0) == 0
    assert call(Cout=0, dy=None, x=None, dw=None, ws=None, ws_bytes=0) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d-" % c[0] + "x".join(map(str, c[1:])))
def test_conv_wgrad_vs_fp64(cuda, case, dtype):
    """dw and db vs fp64 on the same 16-bit operands: the products are exact and the sums fp32, so the error is fp32
    summation noise (rel L2 < 1e-5, test_wgrad.py's bar); NaN-filled outputs come back finite; two calls are bitwise
    equal."""
    ksize, N = case[0], case[1]
    dy, x = operands(case, dtype, cuda)
    dw, db = conv_wgrad(dy, x, ksize)
    dw2, db2 = conv_wgrad(dy, x, ksize)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    if N == 0:
        assert torch.all(dw == 0) and torch.all(db == 0)
        return
    rw, rb = truth(dy, x, ksize)
    ew, eb = rel(dw, rw), rel(db, rb)
    print(f"conv_wgrad {case} {dtype}: dw rel L2 {ew:.2e}, db {eb:.2e}")
    assert ew < 1e-5 and eb < 1e-5
    if case[4:] == (1, 1):  # a 1 x 1 image: every tap but the centre sees only padding
        off = dw.clone()
        off[:, :, 1, 1] = 0
        assert torch.all(off == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(3, 2, 16, 16, 16, 16), (3, 1, 8, 24, 8, 32)], ids=["2x16x16x16x16", "1x8x24x8x32"])
def test_alignment_forms_bitwise(cuda, case):
    """The same data at a 16-byte aligned base (16-byte loads) and in views one element into a flat buffer (element
    loads), dy and x shifted independently: dw and db bitwise equal across the four combinations, and right."""
    ksize = case[0]
    dy0, x0 = operands(case, torch.bfloat16, cuda)

    def shifted(t, by):
        flat = torch.zeros(t.numel() + 8, device=t.device, dtype=t.dtype)
        v = flat[by:by + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 2 * by and v.is_contiguous()
        return v

    outs = [conv_wgrad(shifted(dy0, a), shifted(x0, b), ksize) for a in (0, 1) for b in (0, 1)]
    rw, rb = truth(dy0, x0, ksize)
    assert rel(outs[0][0], rw) < 1e-5 and rel(outs[0][1], rb) < 1e-5
    for dw, db in outs[1:]:
        assert torch.equal(dw, outs[0][0]) and torch.equal(db, outs[0][1])


@pytest.mark.gpu
def test_db_null_and_profiler(cuda):
    """db = NULL leaves dw bitwise unchanged; the profiler sees k_conv_wgrad and k_conv_wgrad_reduce once each per
    call, and nothing on an rc < 0 call."""
    case = (3, 2, 24, 40, 10, 10)
    dy, x = operands(case, torch.bfloat16, cuda)
    prof = _native.KernelProfiler()
    with prof:
        dw, db = conv_wgrad(dy, x, 3, want_db=True)
    ran = prof.summary()
    assert ran.get("k_conv_wgrad", (0,))[0] == 1 and ran.get("k_conv_wgrad_reduce", (0,))[0] == 1, ran
    prof.reset()
    with prof:
        dw2, none = conv_wgrad(dy, x, 3, want_db=False)
        L = _native.lib()
        rc = L.lgm_conv_wgrad(1, 2, 24, 40, 10, 10, 4, _native.ptr(dy), _native.ptr(x), _native.ptr(dw2), None, None, 0,
                              _native.stream_of(cuda), _native.diag())
        assert rc < 0
    ran = prof.summary()
    prof.close()
    assert none is None and torch.equal(dw, dw2)
    assert ran["k_conv_wgrad"][0] == 1 and ran["k_conv_wgrad_reduce"][0] == 1 and len(ran) == 2, ran


@pytest.mark.gpu
def test_wrapper_raises_the_library_error(cuda):
    """A call the library refuses, made through the wrapper (lgm_amd.conv.wgrad): NativeError with the entry point's
    name and the library's own text; the error does not stick: the next, valid call is right (the bar of
    test_conv_wgrad_vs_fp64)."""
    from lgm_amd.conv import wgrad
    dy, x = operands((3, 1, 8, 8, 4, 4), torch.bfloat16, cuda)
    with pytest.raises(_native.NativeError) as err:
        wgrad(dy, x, 5, True)
    assert "lgm_conv_wgrad" in str(err.value) and "ksize must be 1 or 3" in str(err.value), str(err.value)
    dw, db = wgrad(dy, x, 3, True)
    rw, rb = truth(dy, x, 3)
    ew, eb = rel(dw, rw), rel(db, rb)
    print(f"wrapper after a refused call: dw rel L2 {ew:.2e}, db {eb:.2e}")
    assert ew < 1e-5 and eb < 1e-5
