"""Shared by the model-level tests (tests/test_unet_gpu.py, tests/test_lgm_step.py): a UNet configuration whose
attention runs on the flash kernels, the data builder, the staged float64 reference of one LGM training iteration,
and the switch that turns a model into upstream's torch composition on the same device.

The reference chain (fp64_chain): a float64 deepcopy of the model runs forward_gaussians on the CPU; the CPU oracle
rasterizer (oracle/raster_oracle.c, float64 build) renders them; torch computes LGM's MSE terms on its outputs
(core/models.py:145-153); loss.backward() sends the seeds through the oracle's analytic backward into the float64
model. precision=torch.float32 runs the same chain in fp32 (fp32 model, fp32 oracle): its distance from float64 is
what says whether the inputs are well conditioned."""
import contextlib
import copy

import numpy as np
import torch
import torch.nn.functional as F

from lgm_amd import Options
from lgm_amd.cameras import default_rays, orbit_cameras
from tests.render_cases import TAN, rel_l2

# 46.9 M parameters; six MVAttention blocks at C = 512 over 16 heads (head dim 32: the flash kernels) on L = 4 * 8^2 =
# 256 tokens; 3 x 3 convolutions 512 -> 512, 576 -> 512 and 1024 -> 512; GroupNorms of 64, 128, 512, 576 and 1024
MID = dict(down_channels=(64, 512), down_attention=(False, True), mid_attention=True, up_channels=(512, 64),
           up_attention=(True, False))
RENDER_GROUPS = {"mean": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11),
                 "rgb": slice(11, 14)}


def mid_options(**kw) -> Options:
    return Options(input_size=16, splat_size=16, output_size=32, **MID, **kw)


def lgm_data(cuda, B=2, Vo=2, S=32, size=16, seed=0):
    gen = torch.Generator().manual_seed(seed)
    rays = default_rays(size)  # [4, 6, size, size]
    images = torch.randn(B, 4, 3, size, size, generator=gen)
    inp = torch.cat([images, rays[None].expand(B, -1, -1, -1, -1)], dim=2)
    cv, cvp, cp = orbit_cameras(Vo, azimuth_offset=20.0)
    masks = (torch.rand(B, Vo, 1, S, S, generator=gen) > 0.5).float()
    data = {"input": inp, "cam_view": cv[None].expand(B, -1, -1, -1), "cam_view_proj": cvp[None].expand(B, -1, -1, -1),
            "cam_pos": cp[None].expand(B, -1, -1), "images_output": torch.rand(B, Vo, 3, S, S, generator=gen),
            "masks_output": masks}
    return {k: v.contiguous().to(cuda) for k, v in data.items()}


class _OracleRender(torch.autograd.Function):
    """(image unclamped, alpha) of the CPU oracle at Gaussians g [B, N, 14]; the backward is the oracle's own analytic
    one, fed the gradients autograd hands it. `rec` (a dict) receives K and, in the backward, those seeds."""

    @staticmethod
    def forward(ctx, g, cv, cvp, bg, S: int, O, f64: bool, rec: dict):
        out = O.render(g.detach().numpy(), cv, cvp, TAN, S, S, bg, f64=f64)
        ctx.args = (cv, cvp, bg, S, O, f64, rec)
        ctx.save_for_backward(g)
        rec["K"] = out["K"]
        return torch.from_numpy(out["image"]).to(g.dtype), torch.from_numpy(out["alpha"]).to(g.dtype)

    @staticmethod
    def backward(ctx, d_image, d_alpha):
        g, = ctx.saved_tensors
        cv, cvp, bg, S, O, f64, rec = ctx.args
        rec["d_image"], rec["d_alpha"] = d_image.numpy().copy(), d_alpha.numpy().copy()
        out = O.render(g.detach().numpy(), cv, cvp, TAN, S, S, bg, d_image=rec["d_image"], d_alpha=rec["d_alpha"],
                       f64=f64)
        return torch.from_numpy(out["d_gaussians"]).to(g.dtype), None, None, None, None, None, None, None


def render_loss(g, data, bg, O, f64=True):
    """LGM's loss_mse (core/models.py:145-153) on the oracle's render of g [B, N, 14] (a CPU tensor in the graph):
    (loss, dict: the loss terms as floats, `image` (clamped), `raw_image`, `alpha`, `gt_c`, `near` (the count of pixels
    within 1e-5 of a clamp bound) and `rec`, which holds K and, after loss.backward(), the seeds the oracle was fed)."""
    dt = g.dtype
    cv, cvp = (data[k].detach().cpu().numpy() for k in ("cam_view", "cam_view_proj"))
    gt, mask = data["images_output"].detach().cpu().to(dt), data["masks_output"].detach().cpu().to(dt)
    bgv = torch.as_tensor(np.asarray(bg, np.float64)).to(dt)
    rec = {}
    S = gt.shape[-1]
    raw, alpha = _OracleRender.apply(g, cv, cvp, np.asarray(bg, np.float64), S, O, f64, rec)
    near = int(((raw.detach().abs() < 1e-5) | ((raw.detach() - 1.0).abs() < 1e-5)).sum())
    image = raw.clamp(0, 1)  # core/gs.py:87 (its gradient passes where 0 <= image <= 1)
    gt_c = gt * mask + bgv.view(1, 1, 3, 1, 1) * (1 - mask)
    mse_image, mse_alpha = F.mse_loss(image, gt_c), F.mse_loss(alpha, mask)
    loss = mse_image + mse_alpha
    terms = {"loss": loss, "mse_image": mse_image, "mse_alpha": mse_alpha, "psnr": -10 * torch.log10(mse_image)}
    out = {**{k: float(v.detach()) for k, v in terms.items()}, "image": image.detach().numpy(),
           "alpha": alpha.detach().numpy(), "raw_image": raw.detach().numpy(), "gt_c": gt_c.numpy(), "near": near,
           "rec": rec}
    return loss, out


def oracle_step(g, data, bg, O):
    """The render stage alone at given Gaussians (any tensor [B, N, 14]): render_loss in float64 with its
    d_gaussians, and next to it the fp32 oracle's d_gaussians from the same float64 seeds (`d_gaussians_f32`: its
    distance from float64 sets tests.render_cases.grad_bar)."""
    g64 = g.detach().cpu().double().requires_grad_(True)
    loss, out = render_loss(g64, data, bg, O)
    assert out["near"] == 0, f"{out['near']} pixels on a clamp bound (their mask would be rounding-ambiguous)"
    loss.backward()
    out["K"] = out["rec"]["K"]
    out["d_gaussians"] = g64.grad.numpy()
    cv, cvp = (data[k].detach().cpu().numpy() for k in ("cam_view", "cam_view_proj"))
    S = out["image"].shape[-1]
    out["d_gaussians_f32"] = O.render(g64.detach().numpy(), cv, cvp, TAN, S, S, np.asarray(bg, np.float64),
                                      d_image=out["rec"]["d_image"], d_alpha=out["rec"]["d_alpha"])["d_gaussians"]
    return out


def fp64_chain(model, data, bg, O, precision=torch.float64):
    """One training iteration of `model` (an LGM with lambda_lpips = 0, any device; it is deep-copied) on the CPU in
    `precision`: the loss terms, the Gaussians, d_gaussians, d_input and every parameter's gradient by name (all
    detached CPU tensors / floats), K and the count of near-bound pixels (asserted 0)."""
    m = copy.deepcopy(model).cpu().to(precision)
    m.zero_grad()
    x = data["input"].detach().cpu().to(precision).requires_grad_(True)
    g = m.forward_gaussians(x)
    g.retain_grad()
    loss, out = render_loss(g, data, bg, O, f64=precision == torch.float64)
    assert out["near"] == 0, f"{out['near']} pixels on a clamp bound (their mask would be rounding-ambiguous)"
    loss.backward()
    out.update(K=out["rec"]["K"], gaussians=g.detach(), d_gaussians=g.grad.detach(), d_input=x.grad.detach(),
               grads={k: p.grad.detach() for k, p in m.named_parameters()})
    return out


@contextlib.contextmanager
def stock(model):
    """Upstream's torch composition on the model's own device and parameters: torch GroupNorm / SiLU / resample and
    plain nn.Conv2d in the UNet, MVAttention in torch ops around the reference's fallback attention, the head as
    core/models.py:96-117 (lgm_amd.cpu.gaussian_head_cpu: plain torch ops, whatever the device), LPIPS unfused. The
    render stays the renderer's. Everything is put back on exit."""
    import lgm_amd.models as M
    from lgm_amd.attention import MVAttention
    from lgm_amd.cpu import gaussian_head_cpu
    from lgm_amd.unet import _FallbackAttention
    mvas = [m for m in model.modules() if isinstance(m, MVAttention)]
    saved = (model.unet.fused, [(m.fused, m.attn.native_wgrad, m.attn.__class__) for m in mvas], M.gaussian_head)
    lp = getattr(model, "lpips_loss", None)
    lp_fused = getattr(lp, "fused", None)
    try:
        model.unet.fused = False
        for m in mvas:
            m.fused, m.attn.native_wgrad, m.attn.__class__ = False, False, _FallbackAttention
        M.gaussian_head = lambda x, conv, B, V: gaussian_head_cpu(x, conv.weight, conv.bias, int(B), int(V))
        if lp_fused is not None:
            lp.fused = False
        yield model
    finally:
        model.unet.fused = saved[0]
        for m, (f, nw, cls) in zip(mvas, saved[1]):
            m.fused, m.attn.native_wgrad, m.attn.__class__ = f, nw, cls
        M.gaussian_head = saved[2]
        if lp_fused is not None:
            lp.fused = lp_fused


def grouped(named_grads):
    """LGM's parameter gradients concatenated per kind of parameter: the groups of tests/test_unet_gpu.py for the
    UNet's, and the head's 1 x 1 conv as two more."""
    from tests.test_unet_gpu import grouped as unet_grouped
    out = {"head.conv.weight": named_grads["conv.weight"].detach().double().cpu().reshape(-1),
           "head.conv.bias": named_grads["conv.bias"].detach().double().cpu().reshape(-1)}
    out.update(unet_grouped({k: v for k, v in named_grads.items() if k.startswith("unet.")}))
    return out


def rel(a, b) -> float:
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else b
    return rel_l2(a, b)


def relf(a, b) -> float:
    a, b = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (a, b))
    return abs(a - b) / abs(b)
