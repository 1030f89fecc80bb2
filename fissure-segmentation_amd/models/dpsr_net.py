"""Drop-in for `DPSR` of the reference's models/dpsr_net.py:32-104 (differentiable Poisson surface reconstruction, Shape As
Points), 3-D.  The rasterisation of the normals and the reading of the indicator at the points are the splat / sample kernels
of csrc/grid_points.hip, the work between rfftn and irfftn (:74-87, about ten passes over the complex spectrum in the
reference) is one kernel (functional.psr_spectral_solve); the FFTs are torch's, the shift and scale (:91-103) a short torch
composition through which gradients flow as in the reference (through the offset and through |phi[0, 0, 0]|).

`DPSRNet` (:107-185): a point segmentation network, then per (item, foreground label) the points of that label -> normals
(csrc/pcl_normals.hip through functional, K = 30, constants as in the reference) -> DPSR -> marching cubes
(models/dpsr_utils.py).  The reference loops over the batch * (num_classes - 1) groups (its TODO at :146); here all groups run
at once: the points are stable-sorted by (item, label) into one packed cloud, the normals come from one launch, and the groups
go through DPSR as one batch padded with NaN points, which the splat and the sampler ignore (`lengths` keeps the shift's mean
over the real points).  Returns `fissure_segmentation_amd.mesh.Meshes`."""
import torch
from torch import nn

from .. import functional as F_hip
from ..mesh import Meshes
from .access_models import get_point_seg_model_class
from .dpsr_utils import differentiable_marching_cubes, fftfreqs, grid_interp, point_rasterize, spec_gaussian_filter
from .modelio import LoadableModel, store_config_args

NORMALS_NEIGHBOURHOOD = 30   # dpsr_net.py:174, "same as in open3d normal estimation"


class DPSR(nn.Module):
    def __init__(self, res, sig=10, scale=True, shift=True):
        """
        :param res: tuple of output field resolution, e.g. (128, 128, 128)
        :param sig: degree of gaussian smoothing
        """
        super().__init__()
        if len(res) != 3:
            raise NotImplementedError(f"DPSR: only 3-D grids are mirrored, got res {tuple(res)}")
        self.res = tuple(int(r) for r in res)
        self.sig = sig
        self.dim = len(res)
        self.denom = 1
        for r in self.res:
            self.denom *= r
        self.omega = fftfreqs(self.res, dtype=torch.float32)
        self.scale = scale
        self.shift = shift
        # kept under the reference's name for state dicts; the kernel rebuilds the same numbers from (res, sig)
        self.register_buffer("G", spec_gaussian_filter(res=self.res, sig=sig).float())

    def forward(self, V, N, lengths=None):
        """
        :param V: (batch, nv, 3) point cloud coordinates in [-1, 1]
        :param N: (batch, nv, 3) point normals
        :param lengths: None, or (batch,) numbers of real points of clouds padded with NaN coordinates (see spectral_PSR)
        :return phi: (batch, res0, res1, res2) indicator function field
        """
        assert V.shape == N.shape
        V = (V + 1) / 2
        ras_p = point_rasterize(V, N, self.res)
        return self.spectral_PSR(V, ras_p, lengths)

    def spectral_PSR(self, V, normal_field, lengths=None):
        """
        :param V: vertices of shape (batch, nv, 3) in [0, 1]
        :param normal_field: rasterized point normals of shape (batch, 3, res0, res1, res2)
        :param lengths: None (every row of V is a point), or (batch,) counts of the real points of each item: the other rows
            hold NaN coordinates, read 0 from the grid, and the shift's mean runs over the real ones only (an item of length
            0 is divided by 1)
        :return phi: (batch, res0, res1, res2) indicator function field
        """
        ras_s = torch.fft.rfftn(normal_field.float(), dim=(2, 3, 4))
        Phi = F_hip.psr_spectral_solve(ras_s, self.res, self.sig)
        phi = torch.fft.irfftn(Phi, s=self.res, dim=(1, 2, 3))
        if self.shift or self.scale:
            if self.shift:   # offset the field so that its mean over the points is 0
                fv = grid_interp(phi.unsqueeze(-1), V, batched=True).squeeze(-1)
                mean = fv.mean(dim=-1) if lengths is None else fv.sum(dim=-1) / lengths.to(fv.dtype).clamp(min=1)
                phi = phi - mean.view(-1, 1, 1, 1)
            if self.scale:
                fv0 = phi[:, 0, 0, 0]
                phi = -phi / torch.abs(fv0.view(-1, 1, 1, 1)) * 0.5
        return phi


class DPSRNet(LoadableModel):
    """models/dpsr_net.py:107-185: the same constructor arguments, sub-module names (`seg_net`, `dpsr`) and therefore config
    and checkpoint keys.  Divergences: the meshes are this package's `Meshes` (with vertex normals), the (item, label) groups
    are batched instead of looped, `forward` clamps a copy of the coordinates where the reference clamps x[:, :3] in place."""

    @store_config_args
    def __init__(self, seg_net_class, k, in_features, num_classes, spatial_transformer=False, dynamic=True, image_feat_module=False,
                 dpsr_res=(128, 128, 128), dpsr_sigma=10, dpsr_scale=True, dpsr_shift=True):
        """
        :param seg_net_class: point segmentation network, e.g. DGCNNSeg
        :param dpsr_res: tuple of output field resolution. eg., (128,128,128)
        :param dpsr_sigma: degree of gaussian smoothing
        """
        super().__init__()
        seg_net_class = get_point_seg_model_class(seg_net_class)
        self.res = dpsr_res
        self.seg_net = seg_net_class(k=k, in_features=in_features, num_classes=num_classes,
                                     spatial_transformer=spatial_transformer, dynamic=dynamic,
                                     image_feat_module=image_feat_module)
        self.dpsr = DPSR(dpsr_res, dpsr_sigma, dpsr_scale, dpsr_shift)
        self.psr_grid_to_mesh = differentiable_marching_cubes

    def forward(self, x):
        """
        :param x: input of shape (point cloud batch x features x points)
        :return: point segmentation of shape (point cloud batch x num_classes x points) and
            reconstructed meshes (batch * (num_classes - 1), the labels of one item adjacent)
        """
        seg_logits = self.seg_net(x)
        # limit points to the grid (augmentation may have pushed some outside).  The reference clamps x[:, :3] in place
        # (:137); the values are the same, the caller's tensor is left alone
        coords = x[:, :3].clamp(min=-1, max=1)
        return seg_logits, self.generate_meshes(coords, seg_logits)

    def _group_psr_grids(self, coords, seg_logits):
        """coords (B, 3, N), seg_logits (B, C, N) -> PSR grids (B (C - 1), *res) of the argmax groups, batch-major and
        label-minor, and counts (B (C - 1),) int64, the groups' sizes.  A group of fewer than 3 points has no surface: its
        grid is the constant 1 (no zero crossing).  No host read.

        The background points travel along as one extra segment per item (they get normals nobody uses): leaving them out
        would need the number of foreground points on the host."""
        B, C, N = seg_logits.shape
        groups = B * (C - 1)
        dev = coords.device
        label = seg_logits.argmax(1)                                                   # this loses the gradients (:143)
        item = torch.arange(B, device=dev).view(B, 1)
        key = torch.where(label > 0, item * (C - 1) + label - 1, groups + item).reshape(-1)
        skey, perm = torch.sort(key, stable=True)                                      # a group keeps its points' order
        sizes = torch.bincount(key, minlength=groups + B)
        ends = sizes.cumsum(0)
        pts = coords.transpose(1, 2).reshape(B * N, 3)[perm]
        normals, _, _ = F_hip._pcl_packed(pts, ends, NORMALS_NEIGHBOURHOOD, True, None, False, False)
        # (groups + B, N, 3) padded: row skey, column = rank within the segment; the background rows are cut off
        slot = skey * N + (torch.arange(B * N, device=dev) - (ends - sizes)[skey])
        V = torch.full(((groups + B) * N, 3), float("nan"), dtype=pts.dtype, device=dev).index_put((slot,), pts)
        Nrm = torch.zeros((groups + B) * N, 3, dtype=normals.dtype, device=dev).index_put((slot,), normals)
        counts = sizes[:groups]
        phi = self.dpsr(V.view(groups + B, N, 3)[:groups], Nrm.view(groups + B, N, 3)[:groups], lengths=counts)
        return torch.where((counts < 3).view(-1, 1, 1, 1), torch.ones((), dtype=phi.dtype, device=dev), phi), counts

    def generate_meshes(self, coords, seg_logits):
        """coords (B, 3, N) in [-1, 1], seg_logits (B, C, N) -> Meshes of B (C - 1) meshes (batch-major, label-minor) with
        vertex normals; a label with fewer than 3 points gives a mesh without vertices.  One host read (marching cubes')."""
        grids, _ = self._group_psr_grids(coords, seg_logits)
        verts, faces, normals, nv, nf = self.psr_grid_to_mesh(grids)
        return Meshes([v[:n] for v, n in zip(verts, nv)], [f[:n] for f, n in zip(faces, nf)],
                      [v[:n] for v, n in zip(normals, nv)])

    def compute_psr_grid(self, points):
        """
        :param points: point cloud batch of shape (B x N_pts x 3)
        :return: PSR grid of shape (B x self.res)
        """
        normals = F_hip.estimate_pointcloud_normals(
            points, neighborhood_size=min(NORMALS_NEIGHBOURHOOD, points.shape[1] - 1), disambiguate_directions=True)
        return self.dpsr(points, normals)

    def predict_full_pointcloud(self, pc, sample_points=1024, n_runs_min=50):
        seg_logits = self.seg_net.predict_full_pointcloud(pc, sample_points, n_runs_min)
        coords = pc[:, :3]  # only take the coords (always the first 3 feature channels)
        meshes = self.generate_meshes(coords, seg_logits)
        return seg_logits, meshes
