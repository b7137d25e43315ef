"""ctypes binding of the C ABI in include/*.h (liblgm_amd.so).

There is no fallback: if the library is missing or cannot be loaded, every op raises. torch is imported first so
that the library's NEEDED libamdhip64.so.7 resolves to the HIP runtime torch already loaded (same soname), giving
one HIP runtime per process and letting device pointers and streams flow between torch and the library.

The library holds no mutable global state besides its thread-local error string: diagnostics (the kernel profiler,
the render work counters) travel with each call as an `lgm_diag` (include/lgm_common.h). The harness-side switch
for them is `diagnostics(...)` here, whose value `call` passes as every call's `diag` (None = NULL).

SIGNATURES and the constants below are hand copies of include/*.h (the package loads without the headers);
tests/test_abi.py compares them with the headers entry by entry.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import torch  # noqa: F401  (must be loaded before the HIP library, see above)

LIB_PATH = os.environ.get("LGM_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                          "liblgm_amd.so")

_c_int, _c_ll, _c_float, _c_size, _vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
_c_double = ctypes.c_double

SIGNATURES = {
    "lgm_abi_version": (_c_int, []),
    "lgm_last_error": (ctypes.c_char_p, []),
    "lgm_render_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_ll]),
    "lgm_render_workspace_size_opts": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_ll, _c_int]),
    "lgm_render_count_pairs": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _c_float, _c_float,
                                        _c_float, _vp, _c_size, _vp, _vp, _vp]),
    "lgm_render_forward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_float, _c_float,
                                    _c_float, _vp, _vp, _vp, _vp, _vp, _c_size, _c_ll, _vp, _c_int, _vp, _vp]),
    "lgm_render_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_float, _c_float,
                                     _c_float, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _c_ll, _c_int, _vp, _vp]),
    "lgm_attn_forward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _vp, _vp, _c_ll, _vp, _vp,
                                  _vp, _vp]),
    "lgm_attn_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _vp, _vp, _c_ll, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _c_ll, _vp, _c_size, _vp, _vp]),
    "lgm_attn_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_mva_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_mva_norm_tokens": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_mva_tokens_out": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_float, _vp,
                                    _vp, _vp]),
    "lgm_mva_backward_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_mva_tokens_out_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_float, _vp,
                                             _vp, _vp, _vp]),
    "lgm_mva_norm_tokens_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_render_forward_loss": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_float,
                                         _c_float, _c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _c_ll, _c_int,
                                         _vp, _vp]),
    "lgm_render_backward_loss": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_float,
                                          _c_float, _c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _c_ll,
                                          _c_int, _vp, _vp]),
    "lgm_render_tile_lists": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_size, _c_ll, _vp, _vp, _vp,
                                       _vp]),
    "lgm_render_pixel_state": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_size, _c_ll, _vp, _vp, _vp]),
    "lgm_render_records": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_size, _c_ll, _vp, _vp, _vp, _vp]),
    "lgm_render_needle_flags": (_c_int, [_c_ll, _vp, _vp, _vp]),
    "lgm_render_det_flush_limit_log2": (_c_int, [_c_int, _c_int, _c_int]),
    "lgm_gaussian_head_forward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _c_size, _vp, _vp]),
    "lgm_gaussian_head_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int]),
    "lgm_gaussian_head_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _c_size, _vp, _vp]),
    "lgm_linear_wgrad_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int]),
    "lgm_linear_wgrad": (_c_int, [_c_int, _c_int, _c_int, _c_int, _vp, _c_ll, _vp, _c_ll, _vp, _vp, _vp, _c_size,
                                  _vp, _vp]),
    "lgm_conv_wgrad_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_conv_wgrad": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_size,
                                _vp, _vp]),
    "lgm_conv_forward_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_conv_forward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int,
                                  _vp, _vp, _c_size, _vp, _vp]),
    "lgm_conv_dgrad_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_conv_dgrad": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp,
                                _c_size, _vp, _vp]),
    "lgm_gn_silu_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_gn_silu_forward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_gn_silu_backward_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "lgm_gn_silu_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_lpips_dist_workspace_size": (_c_size, [_c_int, _c_int, _c_int, _c_int]),
    "lgm_lpips_dist_forward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_lpips_dist_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp]),
    "lgm_lpips_prep_forward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lgm_lpips_prep_backward": (_c_int, [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    "lgm_data_cameras": (_c_int, [_c_int, _c_int, _c_int, _vp, _vp, _c_double, _c_double, _c_double, _c_double,
                                  _c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lgm_data_views": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp,
                                _vp, _c_double, _vp, _vp, _vp, _vp, _vp]),
    "lgm_optim_workspace_size": (_c_size, [_c_ll]),
    "lgm_optim_grad_norm": (_c_int, [_vp, _c_int, _vp, _c_ll, _c_double, _vp, _c_size, _vp, _vp, _vp]),
    "lgm_optim_adamw": (_c_int, [_vp, _c_int, _vp, _c_ll, _c_ll, _vp, _c_double, _c_double, _c_double, _c_double,
                                 _c_double, _c_double, _vp, _vp]),
    "lgm_optim_scale": (_c_int, [_vp, _c_int, _vp, _c_ll, _vp, _vp, _vp]),
    "lgm_mesh_density_workspace_size": (_c_size, [_c_ll, _c_int, _c_int, _c_int, _c_ll]),
    "lgm_mesh_density_count": (_c_int, [_vp, _c_ll, _c_float, _c_int, _c_int, _c_int, _vp, _vp, _c_float, _vp, _c_size,
                                        _vp, _vp, _vp]),
    "lgm_mesh_density": (_c_int, [_vp, _c_ll, _c_float, _c_int, _c_int, _c_int, _vp, _vp, _c_float, _c_ll, _vp, _vp, _vp,
                                  _c_size, _vp, _vp]),
    "lgm_mesh_sample_workspace_size": (_c_size, [_c_ll, _c_ll, _c_int, _c_int, _c_int, _c_ll]),
    "lgm_mesh_sample_count": (_c_int, [_vp, _c_ll, _c_float, _c_int, _c_int, _c_int, _vp, _vp, _c_float, _vp, _c_size,
                                       _vp, _vp, _vp]),
    "lgm_mesh_sample": (_c_int, [_vp, _c_ll, _c_float, _c_int, _c_int, _c_int, _vp, _vp, _c_float, _c_ll, _vp, _c_ll,
                                 _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_mesh_atlas": (_c_int, [_vp, _c_ll, _vp, _c_ll, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp]),
    "lgm_mesh_extract_workspace_size": (_c_size, [_c_int, _c_int, _c_int]),
    "lgm_mesh_count": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_float, _vp, _c_size, _vp, _vp, _vp]),
    "lgm_mesh_emit": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _c_float, _vp, _c_size, _c_ll, _c_ll, _vp, _vp,
                               _vp, _c_ll, _c_ll, _vp, _vp]),
    "lgm_meshraster_workspace_size": (_c_size, [_c_int, _c_ll, _c_ll, _c_int, _c_int, _c_int, _c_int]),
    "lgm_meshraster_unit_log2": (_c_int, [_c_int, _c_int, _c_int]),
    "lgm_meshraster_forward": (_c_int, [_vp, _c_ll, _vp, _c_ll, _vp, _c_ll, _vp, _vp, _c_int, _c_int, _vp, _vp, _vp, _c_int,
                                        _vp, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_meshraster_backward": (_c_int, [_c_ll, _vp, _c_ll, _vp, _c_ll, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp,
                                         _vp, _vp, _vp, _c_size, _vp, _vp]),
    "lgm_profiler_create": (_vp, []),
    "lgm_profiler_summary": (_c_int, [_vp, ctypes.c_char_p, _c_size]),
    "lgm_profiler_reset": (_c_int, [_vp]),
    "lgm_profiler_destroy": (None, [_vp]),
}

_lib = None


ABI_VERSION = 11
DTYPE_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # include/lgm_attn.h LGM_ATTN_F32 / _BF16 / _F16
RENDER_NO_CULL = 1  # include/lgm_render.h LGM_RENDER_NO_CULL
RENDER_CLAMP_IMAGE = 2  # include/lgm_render.h LGM_RENDER_CLAMP_IMAGE
RENDER_BACKWARD_AGAIN = 4  # include/lgm_render.h LGM_RENDER_BACKWARD_AGAIN
RENDER_DETERMINISTIC = 16  # include/lgm_render.h LGM_RENDER_DETERMINISTIC
RENDER_ANTIALIAS = 32  # include/lgm_render.h LGM_RENDER_ANTIALIAS
RENDER_SH_SHIFT = 6  # include/lgm_render.h LGM_RENDER_SH_SHIFT: the SH degree is (options >> 6) & 3
RENDER_SH_MASK = 3 << 6  # include/lgm_render.h LGM_RENDER_SH_MASK
DATA_U8 = 3  # include/lgm_data.h LGM_DATA_U8
OPTIM_CHUNK = 4096  # include/lgm_optim.h LGM_OPTIM_CHUNK


class NativeError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"lgm_amd native library not built ({LIB_PATH}); run `python -m lgm_amd.build`")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None:
                continue
            fn.restype = res
            fn.argtypes = args
        if L.lgm_abi_version() != ABI_VERSION:
            raise NativeError(f"{LIB_PATH}: ABI {L.lgm_abi_version()} != {ABI_VERSION}; rebuild (python -m lgm_amd.build)")
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().lgm_last_error()
        raise NativeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


# The calling convention of every wrapper in this package (DESIGN §1 "Calling the C ABI from Python"):
#   nat.call("lgm_x", dev, scalars..., nat.ptr(t)..., nat.ptr(ws), ws_bytes)     a compute entry point
#   ws, ws_bytes = nat.workspace("lgm_x_workspace_size", dev, dims...)            its workspace
#   nat.dtype_code(t.dtype, "x", DTYPES)                                          its dtype arguments
# Entry points that do not end in (stream, diag) -- the *_workspace_size functions, the render inspection copies, the
# profiler -- are called on lib() directly, their return code through check().

def ptr(t):
    """A tensor's address as a plain int (None: NULL), which ctypes takes for a void * parameter as it is."""
    return None if t is None else t.data_ptr()


_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(device) -> int:
    """The handle of `device`'s current stream, as an int (torch's raw getter where there is one: a
    torch.cuda.Stream object costs microseconds)."""
    index = getattr(device, "index", None)
    if _get_raw_stream is not None and isinstance(index, int):  # (a device without an index, or its name: the Stream)
        return _get_raw_stream(index)
    return torch.cuda.current_stream(device).cuda_stream


def call(name: str, device, *args):
    """The compute entry point `name`(*args, stream, diag) on `device`'s current stream; a non-zero return raises
    NativeError with `name` and the library's error text. `args` go to ctypes as they are: pointers as ptr(t)."""
    rc = getattr(lib(), name)(*args, stream_of(device), diag())
    if rc:
        check(rc, name)


def workspace(size_fn: str, device, *dims, min_bytes: int = 1):
    """(uint8 tensor, workspace_bytes) for what the library's `size_fn`(*dims) asks: max(workspace_bytes, min_bytes)
    bytes, so that the pointer is never NULL; with min_bytes=0 a zero size allocates nothing and the tensor is None."""
    ws_bytes = getattr(lib(), size_fn)(*dims)
    n = max(ws_bytes, min_bytes)
    return (torch.empty(n, dtype=torch.uint8, device=device) if n else None), ws_bytes


def dtype_code(dtype, who: str, accepted=DTYPE_CODES) -> int:
    """The C ABI's code of `dtype` (DTYPE_CODES), which must be one of `accepted`."""
    if dtype not in accepted:
        names = "/".join(str(d).replace("torch.", "") for d in accepted)
        raise NativeError(f"{who} supports {names}, got {dtype}")
    return DTYPE_CODES[dtype]


def require_device_tensor(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise NativeError(f"{name} must be a GPU tensor: lgm_amd has no CPU path (the reference's rasterizer is "
                          "GPU-only too, core/gs.py:20)")


class _Diag(ctypes.Structure):
    """include/lgm_common.h lgm_diag."""
    _fields_ = [("profiler", _vp), ("render_counters", _vp), ("det_limit_log2", ctypes.c_int)]


_diag_cur = None  # the lgm_diag every wrapper passes while a diagnostics() block is open (None: NULL)


def diag():
    """The `diag` argument for the next C-ABI call: NULL unless a diagnostics() block is open. (Harness state, not
    library state: autograd runs the backward on its own thread, so a thread-local switch would miss it.)"""
    return None if _diag_cur is None else ctypes.byref(_diag_cur)


@contextlib.contextmanager
def diagnostics(profiler=None, render_counters=None, det_limit_log2=0):
    """Inside the block, every liblgm_amd call made through this package carries these diagnostics: a
    KernelProfiler and/or a device uint64 tensor for the render work counters (include/lgm_render.h), and the
    deterministic mode's overflow-bound test hook (include/lgm_common.h)."""
    global _diag_cur
    prev = _diag_cur
    d = _Diag(profiler.h if profiler is not None else None,
              render_counters.data_ptr() if render_counters is not None else None, int(det_limit_log2))
    _diag_cur = d
    try:
        yield d
    finally:
        _diag_cur = prev


def render_counter_words(B: int, V: int, N: int, H: int, W: int) -> int:
    """uint64 words the render work-counter buffer of diagnostics(render_counters=...) must hold (csrc/render_layout.h
    cnt_words, include/lgm_render.h; tests/test_render_layout.py holds the two equal): 8 aggregate words, then 8 per
    (view, tile), 8 per binning record (B V ceil(N / 512) of them) and 4 per backward item (3 B V tiles + 16)."""
    M = B * V * ((W + 15) // 16) * ((H + 15) // 16)
    return 8 + 8 * M + 8 * B * V * ((N + 511) // 512) + 4 * (3 * M + 16)


class KernelProfiler:
    """HIP events around every kernel liblgm_amd launches (on the launching stream) while the profiler is entered
    (`with prof:` = diagnostics(profiler=prof)). summary() -> {kernel: (launches, total_ms)}."""

    def __init__(self):
        self.h = lib().lgm_profiler_create()
        self._cm = None

    def __enter__(self):
        self._cm = diagnostics(profiler=self)
        self._cm.__enter__()
        return self

    def __exit__(self, *exc):
        cm, self._cm = self._cm, None
        return cm.__exit__(*exc)

    def reset(self):
        lib().lgm_profiler_reset(self.h)

    def summary(self):
        buf = ctypes.create_string_buffer(1 << 16)
        check(lib().lgm_profiler_summary(self.h, buf, len(buf)), "lgm_profiler_summary")
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms = line.split()
            out[name] = (int(n), float(ms))
        return out

    def close(self):
        if self.h:
            lib().lgm_profiler_destroy(self.h)
            self.h = None
