"""lgm_amd: MI355X-native (gfx950 / CDNA4) hot path of LGM -- the differentiable Gaussian-splat renderer
(drop-in for core/gs.py GaussianRenderer) and the multi-view attention (drop-in for core/attention.py
MemEffAttention and core/unet.py MVAttention), and the model around them: the UNet on fused GroupNorm+SiLU kernels
(core/unet.py), LGM (core/models.py) and its LPIPS (VGG16) loss on fused distance and input kernels, and the training-batch assembly
of the providers (core/provider_lvis.py, core/utils.py) from decoded views and poses, and the optimizer tail of the
training iteration (main.py:73, 105-109: global-norm clip and AdamW in three launches), and mesh export (convert.py's
step: the Gaussians' density on a grid and surface nets, lgm_amd.mesh; the mesh rasteriser and the texture fit against
renders of the Gaussians, lgm_amd.meshraster). Compute lives in hand-written HIP kernels behind a C ABI
(include/*.h, lgm_amd/_lib/liblgm_amd.so); this package is the host side."""
from .options import Options, preset
from .gs import GaussianRenderer, rasterize
from .unet import DownBlock, MidBlock, ResnetBlock, UNet, UpBlock, group_norm_silu
from .lpips import LPIPS
from .models import LGM
from .data import (build_batch, get_rays, grid_distortion, orbit_camera_jitter, plucker_rays, sample_grid_knots)
from .optim import AdamW, clip_grad_norm_
from .mesh import Mesh, bake_texture, density_grid, extract_surface, gaussians_to_mesh, sample_field
from .meshraster import fit_texture, mesh_psnr, render_mesh

__all__ = ["Options", "preset", "GaussianRenderer", "rasterize", "group_norm_silu", "ResnetBlock", "DownBlock",
           "MidBlock", "UpBlock", "UNet", "LGM", "LPIPS", "build_batch", "get_rays", "plucker_rays",
           "sample_grid_knots", "grid_distortion", "orbit_camera_jitter", "AdamW", "clip_grad_norm_", "Mesh",
           "density_grid", "extract_surface", "gaussians_to_mesh", "sample_field", "bake_texture", "render_mesh",
           "fit_texture", "mesh_psnr"]
__version__ = "0.1.0"
