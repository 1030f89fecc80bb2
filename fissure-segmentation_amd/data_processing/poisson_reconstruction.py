"""`poisson_reconstruction` of the reference's data_processing/surface_fitting.py (:87-141): a fissure label volume is thinned,
every label's voxels become a point cloud, a surface is fitted through each, cleaned up and written back as a label map.  It
lives in a module of its own (like data_processing/pointcloud_surface_fitting.py); `install_reference_aliases()` folds it into
the merged `data_processing.surface_fitting`.  `regularize_fissure_segmentations`, the file I/O around it, is not mirrored.

Every stage runs on the device: `functional.binary_thinning` (csrc/thinning.hip) for sitk.BinaryThinning -- ALL labels in one
launch, as a batch of planes --, `mask_to_points`, one batched `fit_label_surfaces`, `remove_all_but_biggest_component` and
`o3d_mesh_to_labelmap`.  Differences from the reference:

* tensors in and out: `fissures` and `mask` are (D, H, W) tensors on the GPU and the spacing that a sitk.Image carries is the
  argument `spacing` (sx, sy, sz); the result is (int64 label map on the device, `Meshes` with one mesh per present label);
* the thinning rule is the one written down in csrc/thinning.hip and tests/thinning_oracle.py (parity with SimpleITK unpinned),
  the surface fit is `fit_label_surfaces`' (parity with open3d unpinned, see that module), the label map is the exact cover of
  `o3d_mesh_to_labelmap`, not a sampling;
* `return_times=True` gives a dict of synchronised stage times in seconds (`thinning`, `fitting`, `cleanup`, `labelmap`), not
  one time per label: the labels are batched, a label has no time of its own.

Kept: mesh i is written with the value i + 1 whatever its label was (labels {1, 3} give a map with {1, 2}); `right` is
`label > 1`; a label whose thinned set has fewer than 4 points raises the reference's ValueError.
"""
import time

import torch

from .. import functional as F_hip
from ..mesh import Meshes
from ..utils.general_utils import mask_to_points, remove_all_but_biggest_component
from .pointcloud_surface_fitting import MIN_POINTS, fit_label_surfaces
from .surface_fitting import o3d_mesh_to_labelmap


def poisson_reconstruction(fissures, mask, spacing, return_times=False, mask_dilate_radius=1):
    """data_processing/surface_fitting.py:87-141.  fissures: integer label volume (D, H, W) on the GPU, 0 = background; mask: the
    lung mask (D, H, W), nonzero = lung; spacing (sx, sy, sz).  -> (label map int64 (D, H, W) on the device with the values
    1..n for the n present labels in ascending order, `Meshes` of those n meshes[, times]).  See the module's docstring.
    Host reads: the labels, the point counts, and those of the stages underneath."""
    if not torch.is_tensor(fissures) or fissures.dim() != 3 or fissures.is_floating_point() or fissures.is_complex() \
            or fissures.dtype == torch.bool:
        raise ValueError(f"poisson_reconstruction: expected an integer label volume (D, H, W), got "
                         f"{tuple(fissures.shape) if torch.is_tensor(fissures) else type(fissures).__name__}")
    if not torch.is_tensor(mask) or tuple(mask.shape) != tuple(fissures.shape):
        raise ValueError(f"poisson_reconstruction: the mask must be a tensor of the volume's shape {tuple(fissures.shape)}")
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3:
        raise ValueError(f"poisson_reconstruction: spacing must be (sx, sy, sz), got {spacing!r}")
    F_hip._need_gpu(fissures, mask)
    dev = fissures.device
    times, clock = {}, [0.0]

    def lap(stage):
        if return_times:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            if stage is not None:
                times[stage] = now - clock[0]
            clock[0] = now

    def result(label_map, meshes):
        return (label_map, meshes, times) if return_times else (label_map, meshes)

    with torch.no_grad():
        lap(None)
        labels = fissures.unique()[1:].tolist()                      # (the reference drops the smallest value, surface_fitting.py:97)
        if not labels:
            times.update(thinning=0.0, fitting=0.0, cleanup=0.0, labelmap=0.0)
            return result(torch.zeros(tuple(fissures.shape), dtype=torch.int64, device=dev), Meshes([], []))
        # all labels thinned in one launch: one plane per label
        planes = torch.stack([fissures == f for f in labels])
        thinned = F_hip.binary_thinning(planes)
        points = [mask_to_points(t, spacing) for t in thinned]
        lap("thinning")
        for f, p in zip(labels, points):
            if p.shape[0] < MIN_POINTS:
                raise ValueError(f"Tried reconstructing mesh from {p.shape[0]} points. Requires at least 4. (label {f})")
        # the labels become 0..n-1 for the batched fit, whatever their values
        group = torch.cat([torch.full((p.shape[0],), i, dtype=torch.int64, device=dev) for i, p in enumerate(points)])
        meshes = fit_label_surfaces(torch.cat(points), group, len(labels), crop_to_bbox=True, mask=mask, spacing=spacing,
                                    mask_dilate_radius=mask_dilate_radius, first_label=0)
        lap("fitting")
        # keep only the largest component (that is in the correct body half): right fissures are the labels above 1
        center_x = fissures.shape[2] * spacing[0] / 2
        meshes = remove_all_but_biggest_component(meshes, right=[f > 1 for f in labels], center_x=center_x)
        lap("cleanup")
        label_map = o3d_mesh_to_labelmap(list(zip(meshes.verts_list(), meshes.faces_list())), tuple(fissures.shape), spacing)
        lap("labelmap")
    return result(label_map, meshes)
