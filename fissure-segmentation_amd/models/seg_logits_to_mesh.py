"""Drop-in for `SoftMesh` of the reference's models/seg_logits_to_mesh.py:57-116: soft segmentation logits -> one PSR indicator
grid per foreground class.  `psr_grid` is the reference's `forward` up to and including `spectral_PSR` (:76-109) on the kernels
of csrc/grid_points.hip; the last step, differentiable marching cubes (:113-115), has no kernel yet, so `forward` refuses.
`DPSRNet2` (:14-54) is not mirrored for the same reason."""
import torch
from torch import nn

from ..utils.image_utils import gaussian_differentiation
from .divroc import DiVRoC
from .dpsr_net import DPSR


class SoftMesh(nn.Module):
    def __init__(self, smoothing_sigma=10, dpsr_res=(128, 128, 128), dpsr_sigma=10, dpsr_scale=True, dpsr_shift=True,
                 exclude_background=True):
        super().__init__()
        self.smoothing_sigma = smoothing_sigma
        self.res = dpsr_res
        self.dpsr = DPSR(dpsr_res, dpsr_sigma, dpsr_scale, dpsr_shift)
        self.exclude_background = exclude_background
        self.divroc = DiVRoC.apply

    def psr_grid(self, seg_logits, coords):
        """
        :param seg_logits: (batch, num_classes, num_points)
        :param coords: (batch, 3, num_points), grid_sample's convention for the splat; as in the reference the SAME numbers are
            then read by spectral_PSR in the [0, 1] convention, so only points in [0, 1] meet its contract
        :return: (batch * n_foreground_classes, res0, res1, res2) PSR grids, classes of one item adjacent
        """
        batch_size, num_classes, num_points = seg_logits.shape
        seg_logits = seg_logits.softmax(1)
        if self.exclude_background:
            seg_logits = seg_logits[:, 1:]
            num_classes -= 1
        coords = coords.transpose(1, 2).unsqueeze(-2).unsqueeze(-2)
        seg_logits = seg_logits.reshape(*seg_logits.shape, 1, 1)
        seg_grid = self.divroc(seg_logits, coords, (batch_size, num_classes, *self.res)).transpose(-1, -3)
        # smoothing and differentiation in one Gaussian-derivative filter per axis: the approximate normal field
        grads = [gaussian_differentiation(seg_grid, self.smoothing_sigma, order=1, dim=d, padding_mode='constant', truncate=1.5)
                 for d in (2, 1, 0)]
        normals = torch.stack(grads, dim=2)
        normals = normals.view(-1, *normals.shape[2:])
        coords_repeated = coords.view(batch_size, num_points, 3).repeat_interleave(repeats=num_classes, dim=0)
        return self.dpsr.spectral_PSR(coords_repeated, normals)

    def forward(self, seg_logits, coords):
        raise NotImplementedError("SoftMesh.forward needs differentiable marching cubes (models/dpsr_utils.py:44-99 of the "
                                  "reference), which has no HIP kernel yet; SoftMesh.psr_grid returns the PSR grids it would mesh")
