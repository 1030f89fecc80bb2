"""`mesh2labelmap_dist` of the reference's data_processing/surface_fitting_optimization.py (:332-358) on
`functional.mesh_labelmap_dist`.  The rest of that module (`Plane`, `fit_plane_to_fissure`, the plotting) is not mirrored:
those names are not defined here."""
import torch

from .. import functional as F_hip
from ..metrics import _device, _is_empty, _mesh_arrays


def _meshes_on_device(meshes, flip=False):
    """[(verts, faces) | object with .vertices / .triangles, ...] -> two lists of device tensors; an empty mesh keeps its place
    (and with it the labels of the others) as a pair of empty tensors; `flip` reverses the coordinate order of the vertices"""
    meshes = list(meshes)
    full = [None if _is_empty(m) else _mesh_arrays(m) for m in meshes]
    dev = next((m[0].device for m in full if m is not None), None) or _device()
    none = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))
    verts, faces = zip(*[none if m is None else m for m in full]) if full else ((), ())
    return [v.flip(-1) if flip else v for v in verts], list(faces)


def mesh2labelmap_dist(meshes, output_shape, img_spacing, dist_threshold=1.0, mask=None):
    """Label map from meshes by distance: voxel -> 1 + index of the nearest mesh if it is within `dist_threshold` (mm), else 0.

    meshes: `(verts, faces)` pairs (or objects with `.vertices` / `.triangles`), vertices in the axis order of the volume
    (the reference measures them against `nonzero(...) * img_spacing[::-1]`); output_shape (D, H, W); img_spacing in
    (x, y, z), applied reversed; mask (D, H, W), a tensor on the GPU: only its non-zero voxels are labelled.  -> int64 (D, H, W) on the GPU.

    One scatter over the faces of all meshes instead of a distance query per voxel and mesh.  Differences from the
    reference: the result stays on the device; a mesh without vertices or faces is skipped (open3d would raise on it) and
    the others keep their labels; with no mesh at all the result is all zero."""
    verts, faces = _meshes_on_device(meshes)
    if not verts:
        return torch.zeros(tuple(output_shape), dtype=torch.int64, device=_device())
    return F_hip.mesh_labelmap_dist(verts, faces, output_shape, tuple(img_spacing)[::-1], dist_threshold, mask)
