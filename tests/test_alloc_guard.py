"""tests/alloc_guard.py is not vacuous: on CPU tensors it reports a store past a buffer with its call site, makes an
uninitialised accumulator visible in the result, leaves a clean function alone and never leaks its patch."""
import pytest
import torch

from tests.alloc_guard import ALIGN, CANARY, RED, guarded

FILLS = (0x00, 0x3F, 0xFF)


def overrunning():
    """Writes one element past a (5, 3) buffer, through a view of its storage (inside memory the guard owns)."""
    t = torch.empty(5, 3)
    t.fill_(1.0)
    t.as_strided((16,), (1,))[15] = 7.0
    return t


def underrunning():
    t = torch.empty(4, dtype=torch.int32)
    t.zero_()
    torch.as_strided(t, (1,), (1,), t.storage_offset() - 1)[0] = 3
    return t


def accumulating():
    """Relies on a zero accumulator it never wrote."""
    acc = torch.empty(7)
    acc += torch.arange(7.0)
    return acc


def clean():
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    xl = x.contiguous(memory_format=torch.channels_last)
    a = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
    a.copy_(x)
    b = torch.empty_like(xl)  # preserve_format: channels_last strides
    b.copy_(x * 2)
    c = torch.empty_like(xl, memory_format=torch.contiguous_format)
    c.copy_(x * 3)
    d = x.new_empty(0)
    e = x.new_empty((3, 5), dtype=torch.bfloat16)
    e.copy_(torch.arange(15.0).reshape(3, 5))
    f = torch.empty((4, 6), dtype=torch.bfloat16).t()[1:3]
    f.zero_()
    g = torch.empty_like(f)  # preserve_format of a non-dense view: dense, in f's dimension order
    g.fill_(2)
    return {"a": a, "b": b, "c": c, "d": d, "e": e, "g": g}


def test_write_past_the_end_is_reported_with_its_call_site():
    with guarded(0x00, device_type="cpu") as g:
        overrunning()
    assert g.n_allocations == 1 and g.n_bytes == 60 and g.zones_checked == 2
    assert len(g.violations) == 1
    v = g.violations[0]
    assert v.side == "after" and v.shape == (5, 3) and v.dtype == torch.float32
    assert v.offsets == [0, 1, 2, 3]  # the one float behind the 15
    assert "overrunning" in v.site and "test_alloc_guard.py" in v.site
    with pytest.raises(AssertionError, match="overrunning"):
        g.assert_clean()


def test_write_before_the_start_is_reported():
    with guarded(0xFF, device_type="cpu") as g:
        underrunning()
    assert [(v.side, v.dtype) for v in g.violations] == [("before", torch.int32)]
    assert "underrunning" in g.violations[0].site


def test_uninitialised_accumulator_depends_on_the_fill():
    got = []
    for fill in FILLS:
        with guarded(fill, device_type="cpu") as g:
            got.append(accumulating().clone())
        assert g.n_allocations == 1 and not g.violations
    assert torch.equal(got[0], torch.arange(7.0))  # the benign case: zero memory hides the defect
    assert torch.isfinite(got[1]).all() and not torch.equal(got[1], got[0])  # 0x3F3F3F3F: 0.747, finite and wrong
    assert torch.isnan(got[2]).all()
    bits = [t.view(torch.int32) for t in got]
    assert not torch.equal(bits[0], bits[1]) and not torch.equal(bits[1], bits[2]) and not torch.equal(bits[0], bits[2])


def test_fill_and_canary_are_what_the_tensor_and_its_neighbourhood_hold():
    with guarded(0x3F, device_type="cpu") as g:
        t = torch.empty(3, 5, dtype=torch.int32)
        assert (t == 0x3F3F3F3F).all() and t.data_ptr() % ALIGN == 0
        a = g.allocations[0]
        assert a.offset >= RED and a.big.numel() - a.offset - a.nbytes >= RED
        assert (a.big[:a.offset] == CANARY).all() and (a.big[a.offset + a.nbytes:] == CANARY).all()
        assert a.big.data_ptr() + a.offset == t.data_ptr()


def test_clean_function_is_left_alone():
    plain = clean()
    runs = []
    for fill in FILLS:
        with guarded(fill, device_type="cpu") as g:
            runs.append(clean())
        assert not g.violations
        assert g.n_allocations == 6 and g.zones_checked == 12  # every call but new_empty(0)
    for out in runs:
        for k, ref in plain.items():
            t = out[k]
            assert t.dtype == ref.dtype and t.shape == ref.shape and t.stride() == ref.stride(), k
            for fmt in (torch.contiguous_format, torch.channels_last):
                if t.dim() == 4:
                    assert t.is_contiguous(memory_format=fmt) == ref.is_contiguous(memory_format=fmt), (k, fmt)
            assert t.data_ptr() % ALIGN == 0 or t.numel() == 0
            assert torch.equal(t.contiguous().view(torch.uint8), ref.contiguous().view(torch.uint8)), k
    assert runs[0]["a"].is_contiguous(memory_format=torch.channels_last)
    assert runs[0]["b"].is_contiguous(memory_format=torch.channels_last)
    assert runs[0]["c"].is_contiguous() and runs[0]["d"].numel() == 0


def test_other_devices_and_requires_grad():
    with guarded(0xFF, device_type="cuda") as g:  # nothing here is on that device type: all returned as they are
        torch.empty(4)
        torch.empty_like(torch.zeros(3))
    assert g.n_allocations == 0 and g.zones_checked == 0
    with guarded(0x00, device_type="cpu") as g:
        t = torch.empty(3, requires_grad=True)
        assert t.requires_grad and t.is_leaf
    assert g.n_allocations == 1


def test_patch_is_restored_also_when_the_body_raises():
    real = torch.empty, torch.empty_like, torch.Tensor.new_empty
    with guarded(0x00, device_type="cpu"):
        assert torch.empty is not real[0] and torch.empty_like is not real[1]
        assert torch.Tensor.new_empty is not real[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    with pytest.raises(ZeroDivisionError):
        with guarded(0xFF, device_type="cpu"):
            torch.empty(3)
            1 / 0
    assert torch.empty is real[0] and torch.empty_like is real[1] and torch.Tensor.new_empty is real[2]
