"""`mesh2labelmap_sampling` and `o3d_mesh_to_labelmap` of the reference's data_processing/surface_fitting.py (:19-39,
:144-169) on `functional.mesh_labelmap_cover`.  `pointcloud_surface_fitting` of that module is mirrored in
data_processing/pointcloud_surface_fitting.py (with `fit_label_surfaces`, its batched form); it is not defined here.
`poisson_reconstruction` is mirrored in data_processing/poisson_reconstruction.py (sitk.BinaryThinning is
`functional.binary_thinning`, csrc/thinning.hip); it is not defined here either.  `regularize_fissure_segmentations`, the file
I/O around it, is not in scope: that name is not defined anywhere in this package.

The reference draws 10^7 random points on every mesh and writes the label into the cell `floor(point / spacing)` of each.
That is a Monte Carlo estimate of "the cells the surface passes through", and it misses cells that the surface only clips
(1.5-3.4 % of them with 2 10^5 samples on a 24 x 20 x 28 volume).  Here every triangle is tested against every cell of its
bounding box exactly, so the result is the limit of the sampling and does not depend on a seed.  Common differences:

* the sample-count argument is accepted and ignored;
* parts of a mesh at negative coordinates are dropped (the reference's `.long()` truncates coordinates in (-1, 0) into cell 0
  and negative indices wrap around to the far side of the volume);
* later meshes overwrite earlier ones, as there; the result stays on the device.
"""
import torch

from .. import functional as F_hip
from ..metrics import _device
from .surface_fitting_optimization import _meshes_on_device


def _cover(meshes, shape, spacing_xyz, flip):
    verts, faces = _meshes_on_device(meshes, flip)
    if not verts:
        return torch.zeros(tuple(shape), dtype=torch.int64, device=_device())
    return F_hip.mesh_labelmap_cover(verts, faces, shape, tuple(spacing_xyz)[::-1])


def mesh2labelmap_sampling(meshes, output_shape, img_spacing, num_samples=10 ** 7):
    """Label map of the cells that the meshes pass through: `(verts, faces)` pairs with vertices in the axis order of the
    volume, output_shape (D, H, W), img_spacing in (x, y, z), applied reversed.  -> int64 (D, H, W) on the GPU, labels
    1 + mesh index.  `num_samples` is ignored (see the module's docstring).  Parts of a mesh outside the volume are dropped,
    where the reference raises an IndexError; a mesh without vertices or faces is skipped."""
    return _cover(meshes, output_shape, img_spacing, flip=False)


def o3d_mesh_to_labelmap(o3d_meshes, shape, spacing, n_samples=10 ** 7):
    """Label map of the cells that the meshes pass through: objects with `.vertices` / `.triangles` (open3d's TriangleMesh) or
    `(verts, faces)` pairs with vertices in (x, y, z); shape (D, H, W), spacing in (x, y, z).  The cell index is flipped into
    (z, y, x) like the reference's, parts outside the volume are dropped and empty meshes skipped, as there.  `n_samples` is
    ignored (see the module's docstring)."""
    return _cover(o3d_meshes, shape, spacing, flip=True)
