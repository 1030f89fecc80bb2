"""Drop-in for the reference's models/seg_logits_to_mesh.py: `SoftMesh` (:57-116), soft segmentation logits -> one PSR indicator
grid per foreground class -> one mesh per grid, and `DPSRNet2` (:14-54), a point segmentation network followed by it.
`SoftMesh.psr_grid` is the reference's `forward` up to and including `spectral_PSR` (:76-109) on the kernels of
csrc/grid_points.hip; `SoftMesh.meshes` adds the last step (:113-116), differentiable marching cubes on
csrc/marching_cubes.hip, and returns `fissure_segmentation_amd.mesh.Meshes` with vertex normals.  `SoftMesh.forward` keeps
refusing (it would have to return pytorch3d Meshes); `DPSRNet2.forward` calls `meshes`."""
import torch
from torch import nn

from ..mesh import Meshes
from ..utils.image_utils import gaussian_differentiation
from .access_models import get_point_seg_model_class
from .divroc import DiVRoC
from .dpsr_net import DPSR
from .dpsr_utils import differentiable_marching_cubes
from .modelio import LoadableModel, store_config_args


class DPSRNet2(LoadableModel):
    """models/seg_logits_to_mesh.py:14-54: the same constructor arguments, sub-module names (`seg_net`, `seg2mesh`) and
    therefore checkpoint keys.  `forward` returns (seg_logits, Meshes of batch * (num_classes - 1) meshes, the classes of one
    item adjacent)."""

    @store_config_args
    def __init__(self, seg_net_class, k, in_features, num_classes, spatial_transformer=False, dynamic=True, image_feat_module=False,
                 normals_smoothing_sigma=10,
                 dpsr_res=(128, 128, 128), dpsr_sigma=10, dpsr_scale=True, dpsr_shift=True):
        super().__init__()
        seg_net_class = get_point_seg_model_class(seg_net_class)
        self.res = dpsr_res
        self.seg_net = seg_net_class(k=k, in_features=in_features, num_classes=num_classes,
                                     spatial_transformer=spatial_transformer, dynamic=dynamic,
                                     image_feat_module=image_feat_module)
        self.seg2mesh = SoftMesh(normals_smoothing_sigma, dpsr_res, dpsr_sigma, dpsr_scale, dpsr_shift,
                                 exclude_background=True)

    def forward(self, x):
        """
        :param x: (batch, features, points); the first 3 feature channels are the coordinates
        :return: seg_logits (batch, num_classes, points) and the reconstructed meshes (batch * (num_classes - 1))
        """
        seg_logits = self.seg_net(x)
        # limit points to the grid (augmentation may have pushed some outside).  The reference clamps x[:, :3] in place
        # (:44); the values are the same, the caller's tensor is left alone
        coords = x[:, :3].clamp(min=-1, max=1)
        return seg_logits, self.seg2mesh.meshes(seg_logits, coords)

    def predict_full_pointcloud(self, pc, sample_points=1024, n_runs_min=50):
        raise NotImplementedError("DPSRNet2.predict_full_pointcloud: the reference (:50-54) calls self.generate_meshes, a method "
                                  "it never defines, so there is nothing to mirror; use seg_net.predict_full_pointcloud and "
                                  "seg2mesh.meshes")


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

    def meshes(self, seg_logits, coords):
        """the reference's forward (:69-116) with this package's Meshes: psr_grid, then marching cubes at level 0
        -> Meshes of batch * n_foreground_classes meshes with vertices in [-1, 1] (x, y, z along the grid's last, middle and
        first axis) and vertex normals; gradients reach seg_logits through the vertices (DifferentiableMarchingCubes).  A grid
        without a zero crossing gives a mesh without vertices, which the mesh losses refuse."""
        verts, faces, normals, nv, nf = differentiable_marching_cubes(self.psr_grid(seg_logits, coords))
        return Meshes([v[:n] for v, n in zip(verts, nv)], [f[:n] for f, n in zip(faces, nf)],
                      [v[:n] for v, n in zip(normals, nv)])

    def forward(self, seg_logits, coords):
        raise NotImplementedError("SoftMesh.forward would return pytorch3d Meshes after differentiable marching cubes "
                                  "(models/dpsr_utils.py:44-99 of the reference); SoftMesh.meshes runs that step on the HIP "
                                  "kernel and returns fissure_segmentation_amd.mesh.Meshes, SoftMesh.psr_grid the PSR grids")
