"""The binning kernel's instantiations against each other and against the oracle.

k_bin is compiled once per (mode, pair statistics, phase stamps). The bit-exact parity tests reach the binning through
`forward_state`, which passes a statistics pointer; every real render (`_RasterizeBatched.forward`) passes none and so
runs another instantiation, the one built for three workgroups per CU. These tests call `lgm_render_forward` with
`stats_out = NULL` and require what it leaves in its workspace -- radii, records P / Q / rects, tile counts, every
sorted list -- and its image / depth / alpha to be bitwise what the statistics build leaves, and to agree with the
oracle as tests/test_render_parity_gpu.py demands (lists identical under NO_CULL, in-order subsequences with
culling). Shapes are the smallest at which the kernel takes each of its paths: a view group of three and a short one,
a partial last workgroup, a non-square tile grid, a hit list beyond BIN_HITCAP (the second tile-test pass), packed
mode, the stamped build, and more than LDS_HIST_MAX tiles (no LDS histogram).
"""
import numpy as np
import pytest
import torch

from lgm_amd import _native
from lgm_amd.gs import count_pairs, forward_state
from tests.render_cases import TAN, scene

pytestmark = pytest.mark.gpu

BIN_HITCAP = 3072  # render_bin.hip
FIELDS = ("radii", "P", "Q", "rects", "tile_counts", "ids", "image", "depth", "alpha")


def _forward(dev, g, cv, cvp, H, W, stats, options=0, cap=0, counters=None):
    """One lgm_render_forward (with or without a statistics pointer) and the state it left, read back through the
    inspection calls. `ids`: every tile list, (view, tile)-major, concatenated."""
    L = _native.lib()
    g, cv, cvp = (t.to(dev, torch.float32).contiguous() for t in (g, cv, cvp))
    B, N, V = g.shape[0], g.shape[1], cv.shape[1]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    stream = _native.stream_of(dev)
    # (the inspection calls take no options and ask for the float mode's size; the parts they read lie at the same
    # offsets in the deterministic layout)
    ws_bytes = max(L.lgm_render_workspace_size_opts(B, V, N, H, W, cap, options),
                   L.lgm_render_workspace_size(B, V, N, H, W, cap))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    bg = torch.zeros(3, device=dev)
    image = torch.empty(B, V, 3, H, W, device=dev)
    depth = torch.empty(B, V, 1, H, W, device=dev)
    alpha = torch.empty(B, V, 1, H, W, device=dev)
    radii = torch.empty(B, V, N, dtype=torch.int32, device=dev)
    k = torch.zeros(2, dtype=torch.int64, device=dev) if stats else None
    with _native.diagnostics(render_counters=counters):
        _native.check(L.lgm_render_forward(B, V, N, H, W, _native.ptr(g), _native.ptr(cv), _native.ptr(cvp),
                                           _native.ptr(bg), TAN, TAN, 1.0, _native.ptr(image), _native.ptr(depth),
                                           _native.ptr(alpha), _native.ptr(radii), _native.ptr(ws), ws_bytes, cap,
                                           _native.ptr(k), options, stream, _native.diag()), "lgm_render_forward")
    counts = torch.empty(B * V * T, dtype=torch.int32, device=dev)
    _native.check(L.lgm_render_tile_lists(B, V, N, H, W, _native.ptr(ws), ws_bytes, cap, _native.ptr(counts), None,
                                          None, stream), "lgm_render_tile_lists")
    c64 = counts.to(torch.int64)
    offsets = (torch.cumsum(c64, 0) - c64).contiguous()
    total = int(c64.sum().item())
    ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    _native.check(L.lgm_render_tile_lists(B, V, N, H, W, _native.ptr(ws), ws_bytes, cap, _native.ptr(counts),
                                          _native.ptr(offsets), _native.ptr(ids), stream), "lgm_render_tile_lists")
    P = torch.empty(B, V, N, 4, device=dev)
    Q = torch.empty(B, V, N, 4, device=dev)
    rects = torch.empty(B, V, N, 2, dtype=torch.int32, device=dev)
    _native.check(L.lgm_render_records(B, V, N, H, W, _native.ptr(ws), ws_bytes, cap, _native.ptr(P), _native.ptr(Q),
                                       _native.ptr(rects), stream), "lgm_render_records")
    out = {"radii": radii, "P": P.view(torch.int32), "Q": Q.view(torch.int32), "rects": rects,
           "tile_counts": counts.view(B, V, T), "ids": ids[:total], "image": image.view(torch.int32),
           "depth": depth.view(torch.int32), "alpha": alpha.view(torch.int32)}
    out = {n: t.cpu().numpy() for n, t in out.items()}  # (floats compared as their bit patterns)
    if stats:
        out["K_binned"], out["K_reference"] = (int(x) for x in k.tolist())
    return out


def _same(a, b, what, fields=FIELDS):
    for n in fields:
        assert a[n].shape == b[n].shape and np.array_equal(a[n], b[n]), f"{what}: {n} differs"


def _lists(st, b, v):
    """Tile t's list of view (b, v) from a _forward result -> callable."""
    B, V, T = st["tile_counts"].shape
    c = st["tile_counts"].reshape(-1).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(c)])
    return lambda t: st["ids"][off[(b * V + v) * T + t]:off[(b * V + v) * T + t + 1]]


def _check_oracle(O, g, cv, cvp, H, W, full, culled):
    """test_render_parity_gpu.py's list agreement: `full` (NO_CULL) holds the oracle's lists, `culled` in-order
    subsequences of them; radii are the oracle's in both."""
    B, V, T = full["tile_counts"].shape
    for b in range(B):
        for v in range(V):
            gb, cb, pb = g[b].numpy(), cv[b, v].numpy(), cvp[b, v].numpy()
            pre = O.preprocess(gb, cb, pb, TAN, H, W)
            for st in (full, culled):
                assert np.array_equal(st["radii"][b, v], pre["radii"]), f"scene {b} view {v}: radii differ"
            ts, ids = O.tile_lists(gb, cb, pb, TAN, H, W)
            assert np.array_equal(full["tile_counts"][b, v], np.diff(ts)), f"scene {b} view {v}: tile counts differ"
            lf, lc = _lists(full, b, v), _lists(culled, b, v)
            for t in range(T):
                lst = ids[ts[t]:ts[t + 1]]
                assert np.array_equal(lf(t), lst), f"scene {b} view {v} tile {t}: sorted list differs"
                idx = {int(x): k for k, x in enumerate(lst)}
                ks = np.array([idx.get(int(x), -1) for x in lc(t)])
                assert np.all(ks >= 0) and np.all(np.diff(ks) > 0), \
                    f"scene {b} view {v} tile {t}: not an in-order subsequence"


def _vs_forward_state(dev, g, cv, cvp, H, W, st, no_cull):
    """The statistics build through the package's own entry (gs.forward_state) leaves the same state."""
    fs = forward_state(g.to(dev), cv.to(dev), cvp.to(dev), TAN, TAN, H, W, lists=True, no_cull=no_cull, records=True)
    assert np.array_equal(fs["radii"], st["radii"]) and np.array_equal(fs["tile_counts"], st["tile_counts"])
    assert np.array_equal(fs["P"].view(np.int32), st["P"]) and np.array_equal(fs["Q"].view(np.int32), st["Q"])
    assert np.array_equal(fs["rects"].view(np.int32), st["rects"])
    assert np.array_equal(np.concatenate([l for per in fs["ids"] for l in per]), st["ids"])
    return fs


# B = 2, V = 4: a view group of 3 and a short one of 1; N = 1,300: a partial last workgroup (3 x 512 threads);
# 64 x 48: T = 12 tiles in a 4 x 3 grid
SHAPE = dict(B=2, V=4, N=1300, H=48, W=64)


@pytest.fixture(scope="module")
def small():
    g, cv, cvp = scene(B=SHAPE["B"], N=SHAPE["N"], V=SHAPE["V"], seed=11, elevation=10.0)
    return g, cv, cvp


@pytest.fixture(scope="module")
def small_ref(cuda, small):
    """The statistics build's state for the first shape (culled and NO_CULL), computed once."""
    H, W = SHAPE["H"], SHAPE["W"]
    return {nc: _forward(cuda, *small, H, W, stats=True, options=_native.RENDER_NO_CULL if nc else 0)
            for nc in (False, True)}


def test_partial_and_short_groups(cuda, oracle_mod, small, small_ref):
    H, W = SHAPE["H"], SHAPE["W"]
    prod = _forward(cuda, *small, H, W, stats=False)
    _same(prod, small_ref[False], "production vs statistics build")
    fs = _vs_forward_state(cuda, *small, H, W, small_ref[False], no_cull=False)
    assert (fs["K_binned"], fs["K_reference"]) == (small_ref[False]["K_binned"], small_ref[False]["K_reference"])
    assert fs["K_binned"] == int(prod["tile_counts"].sum())
    _check_oracle(oracle_mod, *small, H, W, small_ref[True], prod)


def test_no_cull(cuda, oracle_mod, small, small_ref):
    H, W = SHAPE["H"], SHAPE["W"]
    prod = _forward(cuda, *small, H, W, stats=False, options=_native.RENDER_NO_CULL)
    _same(prod, small_ref[True], "NO_CULL: production vs statistics build")
    _vs_forward_state(cuda, *small, H, W, small_ref[True], no_cull=True)
    _check_oracle(oracle_mod, *small, H, W, prod, small_ref[False])
    # (culling changes the lists, never the outputs)
    _same(prod, small_ref[False], "NO_CULL vs culled", fields=("radii", "image", "depth", "alpha"))


def test_deterministic_mode(cuda, small, small_ref):
    """LGM_RENDER_DETERMINISTIC: the needle side accumulators are not zeroed and no record carries the needle flag;
    everything else is the float mode's."""
    H, W = SHAPE["H"], SHAPE["W"]
    opt = _native.RENDER_DETERMINISTIC
    prod = _forward(cuda, *small, H, W, stats=False, options=opt)
    _same(prod, _forward(cuda, *small, H, W, stats=True, options=opt), "deterministic: production vs statistics build")
    assert not (prod["rects"].view(np.uint32)[..., 1] >> 31).any()
    ref = dict(small_ref[False])
    ref["rects"] = ref["rects"].copy()
    ref["rects"][..., 1] &= 0x7FFFFFFF
    _same(prod, ref, "deterministic vs float mode (needle flags aside)")


def test_packed_mode(cuda, small, small_ref):
    """pair_capacity = the counted pairs (count pass, scan, packed emission): slot mode's lists; and the count-only
    pass still returns forward_state's two counts."""
    H, W = SHAPE["H"], SHAPE["W"]
    g, cv, cvp = small
    kb, kr = count_pairs(g.to(cuda), cv.to(cuda), cvp.to(cuda), TAN, TAN, H, W)
    assert (kb, kr) == (small_ref[False]["K_binned"], small_ref[False]["K_reference"])
    prod = _forward(cuda, *small, H, W, stats=False, cap=kb)
    _same(prod, small_ref[False], "packed production vs slot statistics build")
    _same(_forward(cuda, *small, H, W, stats=True, cap=kb), small_ref[False], "packed vs slot, statistics build")


def test_hit_list_overflow(cuda, oracle_mod):
    """One workgroup whose hits exceed BIN_HITCAP: the tile tests run a second time and emit with LDS fill ranks."""
    H = W = 128
    g, cv, cvp = scene(B=1, N=512, V=1, seed=12, scale_mul=6.0)
    ts, _ = oracle_mod.tile_lists(g[0].numpy(), cv[0, 0].numpy(), cvp[0, 0].numpy(), TAN, H, W)
    assert ts[-1] > 2 * BIN_HITCAP  # (the oracle's 3-sigma pairs; the culled count is asserted below)
    ref = {nc: _forward(cuda, g, cv, cvp, H, W, stats=True, options=_native.RENDER_NO_CULL if nc else 0)
           for nc in (False, True)}
    assert ref[True]["K_binned"] == ts[-1]
    assert ref[False]["K_binned"] > BIN_HITCAP, ref[False]["K_binned"]
    prod = {nc: _forward(cuda, g, cv, cvp, H, W, stats=False, options=_native.RENDER_NO_CULL if nc else 0)
            for nc in (False, True)}
    for nc in (False, True):
        _same(prod[nc], ref[nc], f"overflow (no_cull={nc}): production vs statistics build")
    _check_oracle(oracle_mod, g, cv, cvp, H, W, prod[True], prod[False])
    kb = ref[False]["K_binned"]
    _same(_forward(cuda, g, cv, cvp, H, W, stats=False, cap=kb), ref[False], "overflow: packed vs slot")


def test_stamps(cuda, small, small_ref):
    """diag->render_counters: every launched binning workgroup leaves non-zero, ordered stamps, and the stamped
    build leaves the unstamped one's state."""
    B, V, N, H, W = (SHAPE[k] for k in ("B", "V", "N", "H", "W"))
    M = B * V * 12
    nb_room, nwg = B * V * ((N + 511) // 512), B * ((V + 2) // 3) * ((N + 511) // 512)
    cnt = torch.zeros(_native.render_counter_words(B, V, N, H, W), dtype=torch.int64, device=cuda)
    st = _forward(cuda, *small, H, W, stats=False, counters=cnt)
    _same(st, small_ref[False], "stamped vs unstamped")
    rec = cnt[8 + 8 * M:8 + 8 * M + 8 * nb_room].view(nb_room, 8).cpu().numpy()
    assert (rec[:nwg, 0] > 0).all() and (rec[:nwg, 4] > 0).all(), "a launched workgroup left no stamp"
    assert (rec[:nwg, 0] <= rec[:nwg, 4]).all(), "start after end"
    # the three phase sums fit between start and end
    assert (rec[:nwg, 1:4] >= 0).all() and (rec[:nwg, 1:4].sum(1) <= rec[:nwg, 4] - rec[:nwg, 0]).all()
    assert not rec[nwg:].any()
    # (and with statistics: the fourth instantiation)
    cnt.zero_()
    _same(_forward(cuda, *small, H, W, stats=True, counters=cnt), small_ref[False], "stamped statistics build")
    assert (cnt[8 + 8 * M:8 + 8 * M + 8 * nwg].view(nwg, 8)[:, 0] > 0).all()


def test_no_lds_histogram_strip(cuda, oracle_mod):
    """A 16-pixel-high strip of 8,193 tiles: above LDS_HIST_MAX the kernel counts and emits through global atomics."""
    H, W = 16, 8193 * 16
    g, cv, cvp = scene(B=1, N=600, V=2, seed=13, scale_mul=0.25)
    ref = {nc: _forward(cuda, g, cv, cvp, H, W, stats=True, options=_native.RENDER_NO_CULL if nc else 0)
           for nc in (False, True)}
    assert ref[False]["tile_counts"].shape[-1] == 8193 and ref[False]["K_binned"] > 0
    prod = {nc: _forward(cuda, g, cv, cvp, H, W, stats=False, options=_native.RENDER_NO_CULL if nc else 0)
            for nc in (False, True)}
    for nc in (False, True):
        _same(prod[nc], ref[nc], f"strip (no_cull={nc}): production vs statistics build")
    _check_oracle(oracle_mod, g, cv, cvp, H, W, prod[True], prod[False])
