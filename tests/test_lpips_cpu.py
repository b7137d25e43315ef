"""lgm_amd/lpips.py on the CPU: the VGG16 taps, the three weight-key spellings against synthetic state_dicts that use
those names, the torch composition (fused = False, the CPU path) against an fp64 restatement of the distance formula
of include/lgm_lpips.h, and LGM.forward + backward with the native LPIPS module."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from lgm_amd import LGM, LPIPS, Options
from lgm_amd.cameras import default_rays, orbit_cameras
from lgm_amd.lpips import CHANNELS, CONVS, SLICE_STARTS, VGG16Features, convert_state_dict
from tests.golden.make_unet_golden import TINY


def random_lpips(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LPIPS(**kw)


def distance64(f0, f1, w, eps=1e-10):
    """The formula of include/lgm_lpips.h in fp64: [N]."""
    f0, f1, w = f0.double(), f1.double(), w.double()
    a = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + eps)
    b = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + eps)
    return ((a - b).pow(2) * w.view(1, -1, 1, 1)).sum(1).mean(dim=(1, 2))


def test_tap_shapes_and_channels():
    net = VGG16Features()
    assert sum(isinstance(m, torch.nn.Conv2d) for m in net.features) == 13
    assert sum(isinstance(m, torch.nn.MaxPool2d) for m in net.features) == 4
    taps = net(torch.randn(2, 3, 32, 48))
    assert [tuple(t.shape) for t in taps] == [(2, 64, 32, 48), (2, 128, 16, 24), (2, 256, 8, 12), (2, 512, 4, 6),
                                              (2, 512, 2, 3)]
    assert tuple(t.shape[1] for t in taps) == CHANNELS
    assert all(float(t.detach().min()) >= 0 for t in taps)  # every tap follows a ReLU
    with pytest.warns(UserWarning, match="random"):
        m = LPIPS(size=32)
    assert not m.training and not any(p.requires_grad for p in m.parameters()) and m.fused
    assert all(float(w.min()) >= 0 for w in m.lins)


def synthetic_weights(seed=0):
    """(trunk in torchvision's spelling, heads in the lpips package's, the whole-module spelling) of one set of values."""
    gen = torch.Generator().manual_seed(seed)
    trunk, whole = {}, {}
    for i, cin, cout in CONVS:
        s = next(s for s in range(1, 6) if SLICE_STARTS[s - 1] <= i < SLICE_STARTS[s])
        for name, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            t = torch.randn(shape, generator=gen) * 0.05
            trunk[f"features.{i}.{name}"] = t
            whole[f"net.slice{s}.{i}.{name}"] = t
    heads = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=gen) for k, c in enumerate(CHANNELS)}
    whole.update(heads)
    whole["scaling_layer.shift"] = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    whole["scaling_layer.scale"] = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)
    return trunk, heads, whole


def test_weight_spellings_load_strictly(tmp_path):
    trunk, heads, whole = synthetic_weights()
    a = LPIPS(weights={**trunk, **heads}, size=32)  # torchvision trunk + lpips heads in one dict
    b = LPIPS(weights=[trunk, heads], size=32)      # ... as a list of two
    c = LPIPS(weights=whole, size=32)               # a whole lpips module
    path = tmp_path / "lpips_whole.pth"
    torch.save(whole, path)
    d = LPIPS(weights=str(path), size=32)
    sa = a.state_dict()
    assert torch.equal(sa["net.features.28.weight"], trunk["features.28.weight"])
    assert torch.equal(sa["lins.3"], heads["lin3.model.1.weight"].reshape(-1))
    for other in (b, c, d):
        so = other.state_dict()
        assert list(so) == list(sa) and all(torch.equal(so[k], sa[k]) for k in sa)
        assert not any(p.requires_grad for p in other.parameters()) and other._published_scaling
    x, y = torch.rand(1, 3, 32, 32) * 2 - 1, torch.rand(1, 3, 32, 32) * 2 - 1
    assert torch.equal(a(x, y), c(x, y))
    # strict: a missing tensor, an unknown key, a layer in the wrong slice and a head of the wrong shape all raise
    with pytest.raises(RuntimeError, match="Missing"):
        LPIPS(weights=trunk)
    with pytest.raises(RuntimeError, match="Missing"):
        LPIPS(weights={k: v for k, v in whole.items() if k != "net.slice3.12.bias"})
    with pytest.raises(KeyError, match="unexpected"):
        LPIPS(weights={**trunk, **heads, "classifier.0.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="unexpected"):
        LPIPS(weights={**trunk, **heads, "lin.0.model.1.weight": torch.zeros(1, 64, 1, 1)})
    with pytest.raises(KeyError, match="slice"):
        convert_state_dict({"net.slice1.5.weight": torch.zeros(128, 64, 3, 3)})
    with pytest.raises(KeyError, match="lin1"):
        convert_state_dict({"lin1.model.1.weight": torch.zeros(1, 64, 1, 1)})
    # another scaling layer loads, and keeps the input kernel (which has the published one built in) out
    e = LPIPS(weights={**whole, "scaling_layer.shift": torch.zeros(1, 3, 1, 1)}, size=32)
    assert not e._published_scaling and float(e.shift.abs().max()) == 0


def test_unfused_against_fp64_restatement():
    torch.manual_seed(0)
    m = random_lpips(size=32)
    m.fused = False
    x = torch.rand(2, 3, 32, 32) * 2 - 1
    y = (torch.rand(2, 3, 32, 32) * 2 - 1).requires_grad_(True)
    d = m(x, y)
    assert d.shape == (2, 1, 1, 1) and d.dtype == torch.float32
    gy, = torch.autograd.grad(d.sum(), y)
    m64 = random_lpips(size=32)
    m64.load_state_dict(m.state_dict())
    m64 = m64.double()
    y64 = y.detach().double().requires_grad_(True)
    sh, sc = m64.shift.view(1, 3, 1, 1), m64.scale.view(1, 3, 1, 1)
    ref = sum(distance64(f0, f1, w) for f0, f1, w in zip(m64.net((x.double() - sh) / sc), m64.net((y64 - sh) / sc),
                                                         m64.lins))
    g64, = torch.autograd.grad(ref.sum(), y64)
    assert float((d.view(-1).double() - ref).norm() / ref.norm()) < 1e-5
    assert float((gy.double() - g64).norm() / g64.norm()) < 1e-4
    # identical inputs: distance 0; and in0's trunk runs without a graph
    assert float(m(x, x).abs().max()) == 0.0
    assert not m._features(x)[0].requires_grad and m._features(y)[0].requires_grad


def lgm_data(B=1, Vo=2, S=32, size=16, seed=0):
    gen = torch.Generator().manual_seed(seed)
    rays = default_rays(size)
    images = torch.randn(B, 4, 3, size, size, generator=gen)
    cv, cvp, cp = orbit_cameras(Vo, azimuth_offset=20.0)
    return {"input": torch.cat([images, rays[None].expand(B, -1, -1, -1, -1)], dim=2).contiguous(),
            "cam_view": cv[None].expand(B, -1, -1, -1).contiguous(),
            "cam_view_proj": cvp[None].expand(B, -1, -1, -1).contiguous(), "cam_pos": cp[None].expand(B, -1, -1).contiguous(),
            "images_output": torch.rand(B, Vo, 3, S, S, generator=gen),
            "masks_output": (torch.rand(B, Vo, 1, S, S, generator=gen) > 0.5).float()}


def test_lgm_with_native_lpips_on_cpu():
    """LGM(opt, lpips=LPIPS(...)) on the CPU: construction, the state_dict rule, frozen LPIPS parameters, and
    LGM.forward + backward with the LPIPS term (loss_from_render's torch path), in training and eval mode."""
    opt = Options(input_size=16, splat_size=16, output_size=32, lambda_lpips=1.0, **TINY)
    torch.manual_seed(0)
    model = LGM(opt, lpips=random_lpips(size=32))
    plain = LGM(Options(input_size=16, splat_size=16, output_size=32, **TINY))
    assert isinstance(model.lpips_loss, LPIPS) and model.lpips_loss.size == 32
    assert list(model.state_dict()) == list(plain.state_dict())
    assert not any("lpips_loss" in k for k in model.state_dict())
    assert not any(p.requires_grad for p in model.lpips_loss.parameters())
    assert all(p.requires_grad for k, p in model.named_parameters() if not k.startswith("lpips_loss"))
    # a state_dict builds the native module too
    trunk, heads, _ = synthetic_weights()
    m2 = LGM(opt, lpips={**trunk, **heads})
    assert isinstance(m2.lpips_loss, LPIPS) and not any(p.requires_grad for p in m2.lpips_loss.parameters())
    with pytest.raises(ValueError, match="lpips"):
        LGM(opt)

    data = lgm_data()
    for mode in ("train", "eval"):
        getattr(model, mode)()
        model.zero_grad()
        torch.manual_seed(3)
        res = model(data)
        assert set(res) == {"gaussians", "images_pred", "alphas_pred", "loss", "loss_lpips", "psnr"}
        assert res["loss_lpips"].dim() == 0 and torch.isfinite(res["loss"]) and float(res["loss_lpips"]) > 0
        # the term is the reference's own lines (core/models.py:156-165) around the module, at size 32
        torch.manual_seed(3)
        bg = torch.rand(3) if mode == "train" else torch.ones(3)
        gt = data["images_output"] * data["masks_output"] + bg.view(1, 1, 3, 1, 1) * (1 - data["masks_output"])
        with torch.no_grad():
            ref = model.lpips_loss(
                F.interpolate(gt.reshape(-1, 3, 32, 32) * 2 - 1, (32, 32), mode="bilinear", align_corners=False),
                F.interpolate(res["images_pred"].reshape(-1, 3, 32, 32) * 2 - 1, (32, 32), mode="bilinear",
                              align_corners=False)).mean()
        assert abs(float(res["loss_lpips"]) - float(ref)) <= 1e-5 * abs(float(ref))
        res["loss"].backward()
        for k, p in model.named_parameters():
            if k.startswith("lpips_loss"):
                assert p.grad is None, k
            else:
                assert p.grad is not None and torch.isfinite(p.grad).all(), k
