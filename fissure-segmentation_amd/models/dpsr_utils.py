"""Drop-in for the DPSR helpers of the reference's models/dpsr_utils.py (Shape As Points): `fftfreqs` (:104-126),
`spec_gaussian_filter` (:147-153), `grid_interp` (:156-199) and `point_rasterize` (:227-287), for 3-D grids.

`point_rasterize` and `grid_interp` run on csrc/grid_points.hip in the 'sap' convention (points in [0, 1], cubesize =
1 / (size - 1), lower corner floor(p / cubesize), upper corner fmod(ceil(p / cubesize), size)); they need GPU tensors.  Points
outside [0, 1] are outside the contract: the reference wraps negative indices round the grid, the kernels drop the corner.
The two frequency helpers are host-side table builders and stay numpy / torch.  `DifferentiableMarchingCubes` is not mirrored
yet (it needs a marching-cubes kernel)."""
import numpy as np
import torch

from .. import functional as F_hip


def fftfreqs(res, dtype=torch.float32, exact=True):
    """(R0, ..., Rn/2 + 1, n_dims): the integer frequencies of rfftn over `res` (fftfreq on every axis but the last, rfftfreq
    there; exact=False drops the last, Nyquist, entry)"""
    freqs = [torch.tensor(np.fft.fftfreq(r, d=1 / r), dtype=dtype) for r in res[:-1]]
    last = np.fft.rfftfreq(res[-1], d=1 / res[-1])
    freqs.append(torch.tensor(last if exact else last[:-1], dtype=dtype))
    return torch.stack(torch.meshgrid(*freqs, indexing="ij"), dim=-1)


def spec_gaussian_filter(res, sig):
    """(R0, ..., Rn/2 + 1, 1, 1) fp64: exp(-0.5 (2 sig |f| / res[0])^2) -- res[0] on every axis, as the reference has it"""
    omega = fftfreqs(res, dtype=torch.float64)
    dis = torch.sqrt(torch.sum(omega ** 2, dim=-1))
    return torch.exp(-0.5 * ((sig * 2 * dis / res[0]) ** 2)).unsqueeze(-1).unsqueeze(-1)


def _points3(pts, what):
    if pts.dim() != 3 or pts.shape[-1] != 3:
        raise NotImplementedError(f"{what}: only 3-D point clouds (B, N, 3) are mirrored, got {tuple(pts.shape)}")


def grid_interp(grid, pts, batched=True):
    """grid (B, D, H, W, F) read at pts (B, N, 3) in [0, 1] -> (B, N, F), trilinear; gradients to grid and pts"""
    if not batched:
        grid, pts = grid.unsqueeze(0), pts.unsqueeze(0)
    _points3(pts, "grid_interp")
    if grid.dim() != 5:
        raise ValueError(f"expected grid (B, D, H, W, F), got {tuple(grid.shape)}")
    out = F_hip.sample_grid(grid.permute(0, 4, 1, 2, 3), pts, "sap").transpose(1, 2)
    return out if batched else out.squeeze(0)


def point_rasterize(pts, vals, size):
    """vals (B, N, F) at pts (B, N, 3) in [0, 1] -> (B, F, *size), the sum of the trilinear contributions; gradients to both"""
    _points3(pts, "point_rasterize")
    if vals.dim() != 3 or vals.shape[:2] != pts.shape[:2]:
        raise ValueError(f"expected vals (B, N, F) matching pts {tuple(pts.shape)}, got {tuple(vals.shape)}")
    if len(size) != 3:
        raise NotImplementedError(f"point_rasterize: only 3-D grids are mirrored, got size {tuple(size)}")
    return F_hip.splat_to_grid(vals.transpose(1, 2), pts, size, "sap")
