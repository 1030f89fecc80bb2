"""Drop-in for `DPSR` of the reference's models/dpsr_net.py:32-104 (differentiable Poisson surface reconstruction, Shape As
Points), 3-D.  The rasterisation of the normals and the reading of the indicator at the points are the splat / sample kernels
of csrc/grid_points.hip, the work between rfftn and irfftn (:74-87, about ten passes over the complex spectrum in the
reference) is one kernel (functional.psr_spectral_solve); the FFTs are torch's, the shift and scale (:91-103) a short torch
composition through which gradients flow as in the reference (through the offset and through |phi[0, 0, 0]|).
`DPSRNet` (:107-185) is not mirrored: it needs point-cloud normal estimation (marching cubes is in models/dpsr_utils.py)."""
import torch
from torch import nn

from .. import functional as F_hip
from .dpsr_utils import fftfreqs, grid_interp, point_rasterize, spec_gaussian_filter


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

    def forward(self, V, N):
        """
        :param V: (batch, nv, 3) point cloud coordinates in [-1, 1]
        :param N: (batch, nv, 3) point normals
        :return phi: (batch, res0, res1, res2) indicator function field
        """
        assert V.shape == N.shape
        V = (V + 1) / 2
        ras_p = point_rasterize(V, N, self.res)
        return self.spectral_PSR(V, ras_p)

    def spectral_PSR(self, V, normal_field):
        """
        :param V: vertices of shape (batch, nv, 3) in [0, 1]
        :param normal_field: rasterized point normals of shape (batch, 3, res0, res1, res2)
        :return phi: (batch, res0, res1, res2) indicator function field
        """
        ras_s = torch.fft.rfftn(normal_field.float(), dim=(2, 3, 4))
        Phi = F_hip.psr_spectral_solve(ras_s, self.res, self.sig)
        phi = torch.fft.irfftn(Phi, s=self.res, dim=(1, 2, 3))
        if self.shift or self.scale:
            if self.shift:   # offset the field so that its mean over the points is 0
                fv = grid_interp(phi.unsqueeze(-1), V, batched=True).squeeze(-1)
                phi = phi - fv.mean(dim=-1).view(-1, 1, 1, 1)
            if self.scale:
                fv0 = phi[:, 0, 0, 0]
                phi = -phi / torch.abs(fv0.view(-1, 1, 1, 1)) * 0.5
        return phi
