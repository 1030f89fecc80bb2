"""Drop-in for the DPSR helpers of the reference's models/dpsr_utils.py (Shape As Points): `fftfreqs` (:104-126),
`spec_gaussian_filter` (:147-153), `grid_interp` (:156-199) and `point_rasterize` (:227-287), for 3-D grids.

`point_rasterize` and `grid_interp` run on csrc/grid_points.hip in the 'sap' convention (points in [0, 1], cubesize =
1 / (size - 1), lower corner floor(p / cubesize), upper corner fmod(ceil(p / cubesize), size)); they need GPU tensors.  Points
outside [0, 1] are outside the contract: the reference wraps negative indices round the grid, the kernels drop the corner.
The two frequency helpers are host-side table builders and stay numpy / torch.  `DifferentiableMarchingCubes` (:44-99) runs on
csrc/marching_cubes.hip (functional.marching_cubes) and splats its gradient with the 'torch'-mode splat, as the reference does
with DiVRoC."""
import numpy as np
import torch

from .. import functional as F_hip
from .divroc import DiVRoC


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


def _mc_padded(psr_grid):
    """marching cubes at level 0 in local coordinates -> (verts, faces, normals) padded to the longest mesh (zero rows, -1 face
    rows), num_verts, num_faces"""
    if psr_grid.dim() != 4:
        raise ValueError(f"expected psr_grid (B, D, H, W), got {tuple(psr_grid.shape)}")
    verts, faces, normals, nv, nf = F_hip.marching_cubes(psr_grid.detach(), isolevel=0.0, return_local_coords=True)
    if len(set(nv)) <= 1 and len(set(nf)) <= 1:
        B = len(nv)
        return verts.view(B, nv[0], 3), faces.view(B, nf[0], 3), normals.view(B, nv[0], 3), nv, nf
    pad = torch.nn.utils.rnn.pad_sequence
    return (pad(list(verts.split(nv)), batch_first=True), pad(list(faces.split(nf)), batch_first=True, padding_value=-1),
            pad(list(normals.split(nv)), batch_first=True), nv, nf)


def _mc_grad_grid(verts, normals, dL_dVertex, size):
    """dL/dpsr (B, D, H, W): g = -(dL/dV . n) per vertex, splatted at the vertices (:90-97).  A padded row has a zero normal
    and is masked besides, so it adds nothing; without vertices the result is a zero grid."""
    B, N = verts.shape[:2]
    real = (normals != 0).any(-1)
    g = torch.where(real, -(dL_dVertex.to(torch.float32) * normals).sum(-1), torch.zeros((), device=verts.device))
    grid = DiVRoC.apply(g.view(B, 1, N, 1, 1), verts.view(B, N, 1, 1, 3), (B, 1) + tuple(size))
    return grid.squeeze(1)


class DifferentiableMarchingCubes(torch.autograd.Function):
    """models/dpsr_utils.py:44-99 of the reference, batched: `.apply(psr_grid (B, D, H, W))` -> (verts_padded (B, max V, 3) in
    [-1, 1], faces_padded (B, max F, 3) int64 with -1 rows as padding, normals_padded (B, max V, 3)), the mesh of the level 0.
    Marching cubes has no derivative; as in Shape As Points the vertices are taken to move along their normals, dV/dpsr = -n, so
    the backward splats g = -(dL/dV . n) at the vertices into a (B, D, H, W) grid.  The reference's mix of conventions is kept:
    the vertices are in the align-corners convention (node i at 2 i / (S - 1) - 1), the splat is DiVRoC's, grid_sample's
    align_corners=False (voxel centre i at (2 i + 1) / S - 1), so a vertex's gradient lands up to half a voxel from its edge.
    Gradients of the faces and the normals are ignored, padded rows contribute nothing, any D, H, W is accepted (the reference
    assumes a cube), and an all-empty batch gives a zero gradient.  The forward reads the mesh sizes back from the device."""

    @staticmethod
    def forward(psr_grid):
        verts, faces, normals, _, _ = _mc_padded(psr_grid)
        return verts, faces, normals

    @staticmethod
    def setup_context(ctx, inputs, output):
        psr_grid = inputs[0]
        verts, faces, normals = output
        ctx.save_for_backward(verts, normals)
        ctx.mark_non_differentiable(faces)
        ctx.size = tuple(psr_grid.shape[1:])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dL_dVertex, dL_dFace, dL_dNormals):
        vert_pts, normals = ctx.saved_tensors
        return _mc_grad_grid(vert_pts, normals, dL_dVertex, ctx.size)


def differentiable_marching_cubes(psr_grid):
    """DifferentiableMarchingCubes.apply with the mesh sizes it read back: -> (verts_padded, faces_padded, normals_padded,
    num_verts, num_faces), so a caller can cut the padding off without a second host read"""
    with torch.no_grad():
        _, _, _, nv, nf = out = _mc_padded(psr_grid)
    verts, faces, normals = _MCWithMesh.apply(psr_grid, *out[:3])
    return verts, faces, normals, nv, nf


class _MCWithMesh(torch.autograd.Function):
    """the same gradient for a mesh that has already been extracted"""

    @staticmethod
    def forward(ctx, psr_grid, verts, faces, normals):
        ctx.save_for_backward(verts, normals)
        ctx.mark_non_differentiable(faces)
        ctx.size = tuple(psr_grid.shape[1:])
        return verts.clone(), faces, normals.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dL_dVertex, dL_dFace, dL_dNormals):
        vert_pts, normals = ctx.saved_tensors
        return _mc_grad_grid(vert_pts, normals, dL_dVertex, ctx.size), None, None, None
