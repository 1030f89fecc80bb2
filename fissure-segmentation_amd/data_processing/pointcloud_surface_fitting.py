"""`pointcloud_surface_fitting` of the reference's data_processing/surface_fitting.py (:42-84) and `fit_label_surfaces`, the
batched form of the per-label loop around it.  They live in a module of their own, not in this package's
data_processing/surface_fitting.py: import them from `fissure_segmentation_amd.data_processing.pointcloud_surface_fitting`.
`poisson_reconstruction`, the caller of the per-label loop, is in data_processing/poisson_reconstruction.py (on
`functional.binary_thinning`, csrc/thinning.hip), not here.  Not in scope: `regularize_fissure_segmentations` and
`fit_plane_to_fissure` of surface_fitting_optimization.py; those names are not defined.

The reference runs open3d on the CPU per label: PCA normals, orient_normals_consistent_tangent_plane(100),
octree Poisson reconstruction, crop, lung mask.  Here: normals from csrc/pcl_normals.hip (K = 30, no local disambiguation),
globally consistent signs from functional.orient_normals_consistent (csrc/mesh_cleanup.hip) with k = min(100, 64, N - 1) --
64 is what functional.knn_segment can deliver, so open3d's 100 is clamped --, the spectral Poisson solve of models/dpsr_net.py
on a 2^depth grid over the points' bounding cube enlarged by `scale`, functional.marching_cubes at level 0, then
functional.mesh_remove_vertices for the crop and the mask.  Parity with open3d's octree solver is unpinned (the library is not
available); tests/surface_fit_oracle.py and the fp64 DPSR / marching-cubes oracles are the yardsticks.  The Gaussian of the
spectral solve has sigma = 10 (DPSRNet's default, the only setting the reference pairs with this solver): a standard deviation of
10 / pi = 3.2 grid cells whatever the resolution, i.e. 5 % of the cube's side at depth 6 (64^3) and 2.5 % at depth 7 -- detail
below that scale is smoothed away, where the octree solver at depth 6 resolves about one cell.
"""
import numpy as np
import torch

from .. import functional as F_hip
from ..mesh import Meshes
from ..metrics import _device
from ..models.dpsr_utils import grid_interp, point_rasterize

NORMALS_NEIGHBOURHOOD = 30       # open3d's estimate_normals default (KDTreeSearchParamKNN(30)), as models/dpsr_net.py uses it
ORIENT_NEIGHBOURHOOD = 100       # surface_fitting.py:64; clamped to functional.knn_segment's 64
DEFAULT_SIGMA = 10               # DPSRNet's dpsr_sigma
MIN_POINTS = 4                   # surface_fitting.py:55


# ------------------------------------------------------------------ point cloud -> surface
def _psr_fields(V, N, sizes, res, sig):
    """DPSR.forward (models/dpsr_net.py) for groups padded with NaN points: V (G, n, 3) in [-1, 1], N normals, sizes the numbers
    of real points (host ints) -> phi (G, *res).  The shift's mean runs over a group's own points only, with the shape it has
    when the group is fitted alone, so a group gets the same bits alone and in a batch."""
    V01 = (V + 1) / 2
    ras_s = torch.fft.rfftn(point_rasterize(V01, N, res).float(), dim=(2, 3, 4))
    phi = torch.fft.irfftn(F_hip.psr_spectral_solve(ras_s, res, sig), s=res, dim=(1, 2, 3))
    out = []
    for g, n in enumerate(sizes):
        p = phi[g:g + 1]
        p = p - grid_interp(p.unsqueeze(-1), V01[g:g + 1, :n], batched=True).mean()
        out.append(-p / torch.abs(p[:, 0, 0, 0]).view(1, 1, 1, 1) * 0.5)
    return torch.cat(out)


def _fit_args(depth, width, spacing, mask):
    if width != 0:
        raise NotImplementedError(f"surface fitting: width = {width!r}: only the depth parameter of the octree solver has a "
                                  f"counterpart here (a 2^depth grid), width must be 0")
    depth = int(depth)
    if depth > 8:
        raise NotImplementedError(f"surface fitting: depth = {depth}: the dense grid is built up to 2^8 per axis")
    if depth < 2:
        raise ValueError(f"surface fitting: depth must be at least 2, got {depth}")
    if mask is not None and spacing is None:
        raise ValueError("surface fitting: a mask needs its spacing (sx, sy, sz)")
    return depth


def _on_gpu(a, dtype):
    if torch.is_tensor(a):
        return a.detach().to(dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(_device()).to(dtype)


def fit_label_surfaces(points, labels, num_labels, crop_to_bbox=False, mask=None, depth=6, width=0, scale=1.1,
                       mask_dilate_radius=1, spacing=None, sigma=None, first_label=1):
    """`pointcloud_surface_fitting` for every label of one labelled cloud in ONE batched pass -- one normals launch, one
    orientation call, one DPSR batch, one marching-cubes call, one clean-up -- instead of the reference's loop over the labels
    (data_processing/surface_fitting.py:99-127, train.py:262-284).

    points (N, 3) world (x, y, z), labels (N,) integer; mesh m of the result is the surface through the points with label
    first_label + m, m = 0 .. num_labels - 1 (other labels are ignored).  The remaining arguments as in
    `pointcloud_surface_fitting`; the crop box is each label's own.  A label with fewer than 4 points gives an empty mesh.  A
    label's mesh has the same bits as `pointcloud_surface_fitting` of its points alone.  numpy in means work on the current GPU.
    -> `Meshes` of num_labels meshes with vertex normals.  Host reads: the label sizes, marching cubes' totals, the clean-up's."""
    depth = _fit_args(depth, width, spacing, mask)
    G = int(num_labels)
    if G < 1:
        raise ValueError(f"num_labels must be at least 1, got {num_labels}")
    pts, lab = _on_gpu(points, torch.float32), _on_gpu(labels, torch.int64).reshape(-1)
    if pts.dim() != 2 or pts.shape[1] != 3 or lab.shape[0] != pts.shape[0]:
        raise ValueError(f"expected points (N, 3) and one label per point, got {tuple(pts.shape)} and {tuple(lab.shape)}")
    F_hip._need_gpu(pts, lab)
    dev = pts.device
    res = (2 ** depth,) * 3
    sig = DEFAULT_SIGMA if sigma is None else sigma
    with torch.no_grad():
        group = lab - int(first_label)
        group = torch.where((group >= 0) & (group < G), group, torch.full_like(group, G))
        _, perm = torch.sort(group, stable=True)                       # a label keeps its points' order
        sizes = torch.bincount(group, minlength=G + 1)[:G].tolist()    # host read: the padded batch is sized by the largest label
        fit = [n >= MIN_POINTS for n in sizes]
        ends, total = [], 0
        for n in sizes:
            total += n
            ends.append(total)
        empty = lambda dt: torch.zeros(0, 3, dtype=dt, device=dev)     # noqa: E731
        if not any(fit):
            return Meshes([empty(torch.float32)] * G, [empty(torch.int64)] * G, [empty(torch.float32)] * G)
        pts = pts[perm[:total]].contiguous()
        off = torch.tensor(ends, dtype=torch.int32).to(dev)
        normals = F_hip._pcl_packed(pts, off, NORMALS_NEIGHBOURHOOD, False, None, False, False)[0]
        k = max(2, min(ORIENT_NEIGHBOURHOOD, F_hip._lib.KNN_MAX_K, max(sizes) - 1))
        normals = F_hip.orient_normals_consistent(pts, normals, off, k)[0]
        nmax = max(sizes)
        V = torch.full((G, nmax, 3), float("nan"), dtype=torch.float32, device=dev)
        Nr = torch.zeros(G, nmax, 3, dtype=torch.float32, device=dev)
        centre = torch.zeros(G, 3, dtype=torch.float32, device=dev)
        half = torch.ones(G, dtype=torch.float32, device=dev)
        boxes = torch.zeros(G, 2, 3, dtype=torch.float32, device=dev)
        for g, (n, en) in enumerate(zip(sizes, ends)):
            if not fit[g]:
                continue
            p = pts[en - n:en]
            lo, hi = p.amin(0), p.amax(0)
            centre[g] = (lo + hi) / 2
            h = (hi - lo).max() * (float(scale) / 2)                   # half the side of the bounding cube, enlarged
            half[g] = torch.where(h > 0, h, torch.ones_like(h))        # coincident points: any cube will do
            boxes[g, 0], boxes[g, 1] = lo, hi
            # the grid's axes are (D, H, W) = (z, y, x): the solver takes the coordinates in that order
            V[g, :n] = ((p - centre[g]) / half[g]).flip(-1)
            Nr[g, :n] = normals[en - n:en].flip(-1)
        phi = _psr_fields(V, Nr, sizes, res, sig)
        phi = torch.where(torch.tensor(fit, device=dev).view(G, 1, 1, 1), phi, torch.ones((), dtype=phi.dtype, device=dev))
        verts, faces, vnormals, nv, nf = F_hip.marching_cubes(phi, isolevel=0.0, return_local_coords=True)
        vl, fl, nl, v0, f0 = [], [], [], 0, 0
        for g in range(G):
            vl.append(verts[v0:v0 + nv[g]] * half[g] + centre[g])       # local (x, y, z) in [-1, 1] -> world
            nl.append(vnormals[v0:v0 + nv[g]])
            fl.append(faces[f0:f0 + nf[g]])
            v0, f0 = v0 + nv[g], f0 + nf[g]
        meshes = Meshes(vl, fl, nl)
        if mask is not None:
            mask = _on_gpu(mask, torch.bool) if not torch.is_tensor(mask) else (mask != 0)
            if mask_dilate_radius > 0:
                mask = F_hip.binary_dilate(mask.to(dev), mask_dilate_radius)
        if crop_to_bbox or mask is not None:
            meshes = F_hip.mesh_remove_vertices(meshes, box=boxes if crop_to_bbox else None, mask=mask, spacing=spacing)
    return meshes


def pointcloud_surface_fitting(points, crop_to_bbox=False, mask=None, depth=6, width=0, scale=1.1, mask_dilate_radius=1,
                               spacing=None, sigma=None):
    """data_processing/surface_fitting.py:42-84: a surface through a point cloud (N, 3) in world (x, y, z); see the module's
    docstring for the method.  -> `Meshes` holding one mesh with vertex normals (the reference returns an open3d TriangleMesh).

    crop_to_bbox: drop what lies outside the points' bounding box (inclusive).  mask: a bool volume (D, H, W) (tensor or array;
    the reference takes a sitk.Image, whose spacing travels with it: here `spacing` (sx, sy, sz) is required), dilated by a ball of
    mask_dilate_radius, then `utils.general_utils.mask_out_verts_from_mesh`'s rule.  depth: the grid has 2^depth nodes per axis
    (depth > 8 raises NotImplementedError); width must be 0 (NotImplementedError otherwise); scale: the bounding cube's
    enlargement; sigma: the solver's Gaussian, None = 10.  Fewer than 4 points raise ValueError like the reference.  numpy in means
    work on the current GPU."""
    shape = tuple(points.shape)
    if int(np.prod(shape)) == 0 or shape[0] < MIN_POINTS:
        raise ValueError(f'Tried reconstructing mesh from {shape[0]} points. Requires at least 4.')
    _fit_args(depth, width, spacing, mask)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"expected points (N, 3), got {shape}")
    labels = torch.ones(shape[0], dtype=torch.int64, device=points.device if torch.is_tensor(points) else _device())
    return fit_label_surfaces(points, labels, 1, crop_to_bbox, mask, depth, width, scale, mask_dilate_radius, spacing, sigma)
