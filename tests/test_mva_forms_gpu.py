"""The two access forms of MVAttention's tiled layout kernels (lgm_amd/csrc/mvattn.hip: k_mva_out, k_mva_out_bwd,
k_mva_gn_part, k_mva_gn_dx, each templated on `bool VEC`) are bitwise equal.

Each C entry point runs twice on identical values: once with every tensor 16-byte aligned (mva_vec_ok: the vector
form) and once with one input contiguous but one element off alignment (the scalar form). The shape is
vector-eligible and ragged on both tile axes: C = 72 (C % 8 == 0, two channel tiles, the second of 8 channels) and
H x W = 4 x 17 (HW = 68, HW % 4 == 0, two pixel tiles, the second of 4 pixels). The backward takes mean / rstd as
given inputs, so nothing depends on which forward GroupNorm kernel ran.
"""
import pytest
import torch

from lgm_amd import _native as nat
from lgm_amd._native import DTYPE_CODES as _DTYPES

pytestmark = pytest.mark.gpu

B, F, C, H, W, G = 2, 2, 72, 4, 17, 9
HW, BF = H * W, B * F
SKIP = 0.5 ** 0.5
# the token dtypes MVAttention produces (fp32, or the autocast dtype); x / res / their gradients stay fp32
TOK_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def values():
    """CPU fp32 values shared by every case (never modified), one spare leading element each for the misaligned copy."""
    gen = torch.Generator().manual_seed(1234)
    n = BF * C * HW
    v = {k: torch.randn(n + 1, generator=gen) for k in ("tok", "chan", "res")}
    v["chan"] = v["chan"] * 2 + 0.3
    v["gamma"] = torch.rand(C, generator=gen) + 0.5
    xr = v["chan"][1:].view(BF, G, -1).double()
    v["mean"] = xr.mean(-1).float()
    v["rstd"] = (1.0 / torch.sqrt(xr.var(-1, unbiased=False) + 1e-5)).float()
    return v


def place(cuda, base, dtype, shape, misalign):
    """base[1:] as a contiguous device tensor of `shape`: 16-byte aligned, or one element off."""
    t = base.to(cuda).to(dtype)
    t = t[1:].view(shape) if misalign else t[1:].clone().view(shape)
    assert t.is_contiguous() and (t.data_ptr() % 16 != 0) == misalign
    return t


def out_like(cuda, shape, dtype):
    t = torch.full(shape, float("nan"), device=cuda, dtype=dtype)  # an element left unwritten fails torch.equal
    assert t.data_ptr() % 16 == 0
    return t


def both_forms(run):
    """run(misalign) -> {name: tensor}; every output of the vector and the scalar form must be bitwise equal."""
    vec, sca = run(False), run(True)
    assert vec.keys() == sca.keys() and vec
    for k in vec:
        assert torch.isfinite(vec[k].float()).all(), k
        assert torch.equal(vec[k], sca[k]), (k, float((vec[k].float() - sca[k].float()).abs().max()))


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("tdt", TOK_DTYPES, ids=["f32", "bf16", "f16"])
def test_tokens_out_forms_bitwise_equal(cuda, values, tdt, with_res):
    odt = torch.float32 if with_res else tdt  # as _TokensOut: promote_types(y, res), or y's without a residual

    def run(misalign):
        y = place(cuda, values["tok"], tdt, (B, F * HW, C), misalign)
        res = place(cuda, values["res"], torch.float32, (BF, C, H, W), False) if with_res else None
        out = out_like(cuda, (BF, C, H, W), odt)
        rc = nat.lib().lgm_mva_tokens_out(_DTYPES[tdt], _DTYPES[torch.float32] if with_res else 0, _DTYPES[odt], B, F, C,
                                          HW, nat.ptr(y), nat.ptr(res), SKIP, nat.ptr(out), nat.stream_of(cuda),
                                          nat.diag())
        assert rc == 0, nat.lib().lgm_last_error()
        return {"out": out}

    both_forms(run)


@pytest.mark.parametrize("with_res", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("tdt", TOK_DTYPES, ids=["f32", "bf16", "f16"])
def test_tokens_out_backward_forms_bitwise_equal(cuda, values, tdt, with_res):
    odt = torch.float32 if with_res else tdt

    def run(misalign):
        d_out = place(cuda, values["chan"], odt, (BF, C, H, W), misalign)
        d_y = out_like(cuda, (B, F * HW, C), tdt)
        d_res = out_like(cuda, (BF, C, H, W), torch.float32) if with_res else None
        rc = nat.lib().lgm_mva_tokens_out_backward(_DTYPES[odt], _DTYPES[tdt], _DTYPES[torch.float32] if with_res else 0,
                                                   B, F, C, HW, nat.ptr(d_out), SKIP if with_res else 1.0, nat.ptr(d_y),
                                                   nat.ptr(d_res), nat.stream_of(cuda), nat.diag())
        assert rc == 0, nat.lib().lgm_last_error()
        return {"d_y": d_y, **({"d_res": d_res} if with_res else {})}

    both_forms(run)


@pytest.mark.parametrize("opt", [(True, True, True), (False, True, False), (False, False, False)],
                         ids=["dres-dx-gamma", "dx", "bare"])
@pytest.mark.parametrize("tdt", TOK_DTYPES, ids=["f32", "bf16", "f16"])
def test_norm_tokens_backward_forms_bitwise_equal(cuda, values, tdt, opt):
    with_dres, with_dx, with_gamma = opt

    def run(misalign):
        L = nat.lib()
        x = place(cuda, values["chan"], torch.float32, (BF, C, H, W), False)
        d_tok = place(cuda, values["tok"], tdt, (B, F * HW, C), misalign)
        d_res = place(cuda, values["res"], torch.float32, (BF, C, H, W), False) if with_dres else None
        gamma = values["gamma"].to(cuda) if with_gamma else None
        mean, rstd = values["mean"].to(cuda), values["rstd"].to(cuda)
        dx = out_like(cuda, (BF, C, H, W), torch.float32) if with_dx else None
        dg, db = out_like(cuda, (C,), torch.float32), out_like(cuda, (C,), torch.float32)
        need = L.lgm_mva_backward_workspace_size(B, F, C, HW, G)
        ws = torch.empty(need, device=cuda, dtype=torch.uint8)
        rc = L.lgm_mva_norm_tokens_backward(_DTYPES[torch.float32], _DTYPES[tdt], B, F, C, HW, G, nat.ptr(x),
                                            nat.ptr(gamma), nat.ptr(mean), nat.ptr(rstd), nat.ptr(d_tok), nat.ptr(d_res),
                                            nat.ptr(dx), nat.ptr(dg), nat.ptr(db), nat.ptr(ws), need, nat.stream_of(cuda),
                                            nat.diag())
        assert rc == 0, L.lgm_last_error()
        return {"dgamma": dg, "dbeta": db, **({"dx": dx} if with_dx else {})}

    both_forms(run)
