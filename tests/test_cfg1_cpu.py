"""BASELINE config 1 end to end on the CPU (scripts/cfg1_cpu.py): the catstatue PNG as 4 views + rays, the
reference's 'big' UNet with its 16 MVAttention blocks swapped for lgm_amd's, the Gaussian head, save_ply and one
256^2 render through lgm_amd.GaussianRenderer on CPU tensors. The UNet is the reference's code and is not part of
this repository, so its stage comes from tests/golden/cfg1_unet_big*.npz (tests/golden/make_cfg1_golden.py): the
reference UNet's output on these views, and the record that the UNet with the swapped blocks returned the same
tensor (same weights, the reference's fallback attention) to fp32 rounding. Checks: the views fed in are the
recorded ones; that record; the render of the head's Gaussians equals the oracle's on the same Gaussians; the PLY
round-trips."""
import os
import sys

import numpy as np
import torch

from tests.render_cases import rel_l2

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PNG = os.path.join(GOLDEN, "catstatue_rgba.png")


def test_cfg1_big_cpu_end_to_end(tmp_path, oracle_mod):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "scripts"))
    import cfg1_cpu as H

    from tests.golden.make_cfg1_golden import sample_indices
    z = np.load(os.path.join(GOLDEN, "cfg1_unet_big.npz"))
    # the input stage: the views the recorded UNet outputs belong to
    views = H.load_views(PNG)
    assert list(views.shape) == list(z["views_shape"]) == [1, 4, 9, 256, 256]
    flat = views.numpy().reshape(-1)
    np.testing.assert_allclose(flat[sample_indices(flat.size)], z["views_sample"], rtol=0, atol=1e-6)

    # the swapped UNet == the reference UNet with its own (fallback) attention, same weights (as recorded)
    assert int(z["swapped_mvattention_blocks"]) == 16
    assert float(z["swapped_vs_reference_rel_l2"]) < 1e-5
    a = torch.from_numpy(np.stack([np.load(os.path.join(GOLDEN, f"cfg1_unet_big_v{v}.npz"))["unet_out"]
                                   for v in range(int(z["n_views"]))]))

    from lgm_amd.head import GaussianHead
    torch.manual_seed(0)
    head = GaussianHead()
    res = H.after_unet(a, head, 1, 4, str(tmp_path), int(z["swapped_mvattention_blocks"]))
    print({k: v for k, v in res.items() if k != "_frame"})
    assert res["swapped_mvattention_blocks"] == 16
    assert res["unet_out"] == [4, 14, 128, 128] and res["gaussians"] == [1, 65536, 14]
    assert res["image_finite"] and res["frame"] == [1, 256, 256, 3]

    # the harness's render vs the oracle on the same Gaussians and camera
    from lgm_amd import GaussianRenderer, Options
    from lgm_amd.cameras import cameras_from_c2w, orbit_camera, projection_matrix
    with torch.no_grad():
        g = head(a, 1, 4)
    opt = Options(output_size=256)
    pose = torch.from_numpy(orbit_camera(0, 0, radius=1.5, opengl=True)).unsqueeze(0)
    cv, cvp, cp = cameras_from_c2w(pose, projection_matrix(opt.fovy, opt.znear, opt.zfar))
    with torch.no_grad():
        out = GaussianRenderer(opt).render(g, cv[None], cvp[None], cp[None])
    o = oracle_mod.render(g.numpy(), cv[None].numpy(), cvp[None].numpy(), float(np.tan(0.5 * np.deg2rad(49.1))),
                          256, 256, np.ones(3, np.float32))
    assert rel_l2(out["image"].numpy(), np.clip(o["image"], 0, 1)) < 1e-4
    assert rel_l2(out["alpha"].numpy(), o["alpha"]) < 1e-4
    # ... and it is the frame the harness returned
    frame = (out["image"].squeeze(1).permute(0, 2, 3, 1).contiguous().float().numpy() * 255).astype(np.uint8)
    np.testing.assert_array_equal(frame, res["_frame"])

    # save_ply wrote what load_ply reads back (opacity-pruned, inverse activations round-tripped)
    back = GaussianRenderer(opt).load_ply(str(tmp_path / "catstatue.ply"))
    keep = g[0, :, 3] >= 0.005
    assert back.shape == (int(keep.sum()), 14)
