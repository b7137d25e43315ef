"""Poisoned, red-zoned allocations for the tests (a helper: neither a test module nor a conftest).

`with guarded(fill) as g:` replaces torch.empty, torch.empty_like and torch.Tensor.new_empty for the duration of the
block. Every tensor they hand out on `device_type` lies in the middle of a larger uint8 allocation the guard owns:

    [ >= RED bytes of CANARY | storage bytes of `fill` | >= RED bytes of CANARY ]

with the real tensor's shape, strides and dtype. The contents of an "uninitialised" buffer thereby become an input
of the test (0x00: what a fresh block from the driver holds; 0x3F: finite garbage, 0.747 as fp32 and a large positive
int32; 0xFF: NaN in fp32/bf16/fp16 and -1 in integers), and a store past either end of a buffer lands in a red zone,
which is checked when the block exits, instead of in a neighbouring tensor.

nat.workspace allocates through torch.empty, so the C ABI's workspaces are covered with the outputs. The patch is
process-global on purpose: autograd runs the backward on its own thread.
"""
from __future__ import annotations

import contextlib
import os
import traceback

import torch

RED = 4096  # bytes of red zone on either side (a multiple of the 256-byte alignment the allocators give)
CANARY = 0xA5
ALIGN = 256

_HERE = os.path.abspath(__file__)


class Allocation:
    """One guarded allocation: the owning uint8 block, what was asked for and who asked."""

    def __init__(self, big, offset, nbytes, shape, dtype, stack):
        self.big, self.offset, self.nbytes = big, offset, nbytes  # the tensor is big[offset:offset + nbytes]
        self.shape, self.dtype, self.stack = tuple(shape), dtype, stack

    @property
    def site(self) -> str:
        """file:line (function) of the innermost caller outside this module."""
        for fr in reversed(self.stack):
            if os.path.abspath(fr.filename) != _HERE:
                return f"{fr.filename}:{fr.lineno} ({fr.name})"
        return "?"


class Violation:
    def __init__(self, alloc: Allocation, side: str, offsets):
        self.alloc, self.side, self.offsets = alloc, side, offsets
        self.shape, self.dtype, self.site = alloc.shape, alloc.dtype, alloc.site

    def __repr__(self):
        return (f"red zone {self.side} {self.dtype} {list(self.shape)} from {self.site}: "
                f"{len(self.offsets)} bytes changed, first at zone offset {self.offsets[0]}")


class Guard:
    """What a guarded() block saw. `allocations`, `n_allocations`, `n_bytes`; after the block also `violations`
    (a list of Violation) and `zones_checked`."""

    def __init__(self, fill: int, device_type: str):
        assert 0 <= fill <= 0xFF
        self.fill, self.device_type = fill, device_type
        self.allocations: list[Allocation] = []
        self.violations: list[Violation] = []
        self.zones_checked = 0

    @property
    def n_allocations(self) -> int:
        return len(self.allocations)

    @property
    def n_bytes(self) -> int:
        return sum(a.nbytes for a in self.allocations)

    def check(self):
        self.violations, self.zones_checked = [], 0
        for a in self.allocations:
            for side, zone in (("before", a.big[:a.offset]), ("after", a.big[a.offset + a.nbytes:])):
                self.zones_checked += 1
                bad = (zone != CANARY).nonzero().flatten()
                if bad.numel():
                    self.violations.append(Violation(a, side, bad.cpu().tolist()))
        return self.violations

    def assert_clean(self):
        assert not self.violations, "\n".join(map(repr, self.violations))


def _storage_nbytes(t: torch.Tensor) -> int:
    """Bytes from the tensor's first element to the end of the last one its strides reach."""
    span = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return span * t.element_size()


@contextlib.contextmanager
def guarded(fill: int, device_type: str = "cuda"):
    guard = Guard(fill, device_type)
    real_empty, real_empty_like, real_new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def wrap(t):
        if not isinstance(t, torch.Tensor) or t.device.type != device_type or t.numel() == 0 or t.is_pinned():
            return t
        n = _storage_nbytes(t)
        # ALIGN bytes of slack: the host allocator aligns to 64 bytes only, and the tensor is to be as aligned as a
        # real one, so the front red zone is RED..RED+ALIGN-1 bytes long
        big = real_empty(n + 2 * RED + ALIGN, dtype=torch.uint8, device=t.device)
        off = RED + (-(big.data_ptr() + RED)) % ALIGN
        big[:off] = CANARY
        big[off:off + n] = guard.fill
        big[off + n:] = CANARY
        out = big[off:off + n].view(t.dtype).as_strided(t.shape, t.stride())
        assert out.data_ptr() % ALIGN == 0
        guard.allocations.append(Allocation(big, off, n, t.shape, t.dtype, traceback.extract_stack()[:-2]))
        return out.requires_grad_(True) if t.requires_grad else out

    def empty(*args, **kwargs):
        if kwargs.get("out") is not None:
            return real_empty(*args, **kwargs)
        return wrap(real_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        return wrap(real_empty_like(*args, **kwargs))

    def new_empty(self, *args, **kwargs):
        return wrap(real_new_empty(self, *args, **kwargs))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield guard
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = real_empty, real_empty_like, real_new_empty
        if device_type == "cuda" and torch.cuda.is_available():
            torch.cuda.synchronize()
        guard.check()
