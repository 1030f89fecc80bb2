"""Lobe filling and lobes-to-fissures with the reference's names (data_processing/find_lobes.py:17-92), tensors in, tensors
out: no SimpleITK.  Convert an image with `torch.from_numpy(sitk.GetArrayFromImage(img).astype(int))` on the way in and
`GetImageFromArray(t.cpu().numpy())` + `CopyInformation` on the way out, as the reference does around the same calls.
`find_lobes` (:95-177) goes from fissures back to lobes with the ball morphology and connected components of
csrc/morphology.hip; the mesh list it returns stays empty.  `compute_surface_mesh_marching_cubes` (:185-210) is a separate
call on csrc/marching_cubes.hip: it gives the meshes the reference's find_lobes would have appended."""
import numpy as np
import torch

from .. import functional as F_hip
from ..mesh import Meshes


def fill_lobes(lobes: torch.Tensor, mask: torch.Tensor, **solver) -> torch.Tensor:
    """find_lobes.py:17-30: sparse lobe labels (D, H, W) -> every voxel of the mask labelled by the random walker on the binary
    graph of (lobes != 0), int64 like the reference.  Keyword arguments go to the solver (tol, max_iter, ...)."""
    return F_hip.random_walk_fill(lobes, mask, **solver).long()


def lobes_to_fissures(lobes: torch.Tensor, mask: torch.Tensor, device=None, **solver):
    """find_lobes.py:33-92 for tensors: -> (fissures uint8, lobes_filled int64).  Fewer than 4 labels after filling is a
    ValueError (the reference fails on an index there)."""
    if device is not None:
        lobes, mask = lobes.to(device), mask.to(device)
    lobes_filled = F_hip.random_walk_fill(lobes, mask, **solver)
    return F_hip.lobes_to_fissures_labels(lobes_filled), lobes_filled.long()


_BALL4 = 389   # voxels of the radius-4 ball


def find_lobes(fissure_seg: torch.Tensor, lung_mask: torch.Tensor, exclude_rhf: bool = False):
    """find_lobes.py:95-177 for tensors: fissure labels and a lung mask (D, H, W) -> (lobes, [], success).  The steps are
    the reference's, each SimpleITK filter replaced by its bit-plane launch (the volume stays in bit planes from the two
    packs to the component labels):
      not_lobes = not erode(lung, 2, boundary = foreground) or (fissures != 0)      :114-119 (label 3 dropped first if exclude_rhf)
      not_lobes = dilate(closing(not_lobes, 2), 2)                                  :122-123
      lobes_mask = opening(not not_lobes, 4)                                        :127-128
      components with connectivity 6                                                :130-132
    Fewer than 4 (exclude_rhf) or 5 components: (the component image int32, [], False), as the reference returns it.
    Otherwise the largest 4 or 5 (ties: the smaller component label first) are renumbered from their centroids (:156-177):
    smaller x is right; right lobes by z: lowest 1, highest 2, (5 lobes) middle 5; left lobes: lower 3, higher 4.  Centroids
    are compared in fp64 from the exact integer sums.  -> (lobes int64, [], True); the list would hold the marching-cubes
    meshes, which are not built here.  One host read: the count and the statistics of the `target` largest components, which
    are picked on the device.  The statistics table needs no count from the host: every voxel of an opening by the radius-4 ball
    lies in a whole ball of set voxels, the ball is 6-connected, and the balls of two components are disjoint, so there are at
    most D H W / 389 components."""
    if fissure_seg.dim() != 3 or fissure_seg.shape != lung_mask.shape:
        raise ValueError(f"find_lobes: fissure_seg {tuple(fissure_seg.shape)} and lung_mask {tuple(lung_mask.shape)} must be one "
                         f"(D, H, W) shape")
    if fissure_seg.is_floating_point() or lung_mask.is_floating_point():
        raise ValueError(f"find_lobes: expected bool or integer volumes, got {fissure_seg.dtype} and {lung_mask.dtype}")
    F_hip._need_gpu(fissure_seg, lung_mask)
    target = 4 if exclude_rhf else 5
    with torch.no_grad():
        W = fissure_seg.shape[-1]
        fis = fissure_seg[None]
        if exclude_rhf:
            fis = torch.where(fis == 3, torch.zeros_like(fis), fis)
        r2, r4 = (2, 2, 2), (4, 4, 4)
        # not erode(lung, border 1) = dilate(not lung, border 0): one launch, the NOTs inside it
        not_lobes = F_hip._bits_dilate(F_hip._pack_bits(lung_mask[None]), W, r2, border=0, inv_in=True) | F_hip._pack_bits(fis)
        not_lobes = F_hip._bits_closing(not_lobes, W, r2)
        lobes_mask = F_hip._bits_dilate(not_lobes, W, r2, border=0, inv_out=True)
        lobes_mask = F_hip._bits_opening(lobes_mask, W, r4)
        labels, n_dev = F_hip._cc_bits(lobes_mask, W, 6)
        cap = max(fissure_seg.numel() // _BALL4, 1)
        stats = F_hip._stats_device(labels, cap)[0]                            # (cap, 4); the labels past n hold zeros
        k = min(target, cap)
        top = torch.sort(stats[:, 0], descending=True, stable=True).indices[:k]   # by size descending, ties by the smaller label
        host = torch.cat([n_dev.long(), top, stats[top].reshape(-1)]).cpu().numpy()   # the one host read
        n = int(host[0])
        if n < target:
            return labels[0], [], False
        order, st = host[1:1 + target], host[1 + target:].reshape(target, 4)   # old labels - 1 of the sorted labels 1..target
        centroids = st[:, 1:].astype(np.float64) / st[:, :1].astype(np.float64)   # (z, y, x)
        sort_by_x = np.argsort(centroids[:, 2], kind="stable")
        num_right = 2 if exclude_rhf else 3
        right, left = sort_by_x[:num_right], sort_by_x[num_right:]
        new = np.zeros(target, np.int64)
        left_z = np.argsort(centroids[left, 0], kind="stable")
        new[left[left_z[0]]], new[left[left_z[1]]] = 3, 4
        right_z = np.argsort(centroids[right, 0], kind="stable")
        new[right[right_z[0]]], new[right[right_z[-1]]] = 1, 2
        if not exclude_rhf:
            new[right[right_z[1]]] = 5
        lut = np.zeros(n + 1, np.int32)
        lut[order + 1] = new
        lobes = F_hip._apply_lut(labels, torch.from_numpy(lut).to(labels.device)[None], torch.int64)
    return lobes[0], [], True


def compute_surface_mesh_marching_cubes(label_img: torch.Tensor, mask_image: torch.Tensor = None, max_label: int = None,
                                        spacing=(1, 1, 1)):
    """find_lobes.py:185-210 for tensors: one surface mesh per label 1..max_label of an integer label volume (D, H, W)
    (max_label=None: the largest label, one host read), all labels in ONE batched launch sequence
    (functional.marching_cubes_labels) -> a list of one-mesh `Meshes` with vertex normals pointing out of the object.
    Vertices are in xyz order in physical units, spacing = (sx, sy, sz) = img.GetSpacing(), as the reference's are after its
    flip.  mask_image (D, H, W): only cells whose 8 voxels are in the mask are meshed (dilate the mask so that it does not cut
    the surface); this rule and the triangulation are ours, skimage's are unpinned.  A label without voxels gives a mesh without
    vertices."""
    if label_img.dim() != 3 or label_img.is_floating_point():
        raise ValueError(f"compute_surface_mesh_marching_cubes: expected an integer label volume (D, H, W), got "
                         f"{tuple(label_img.shape)} {label_img.dtype}")
    F_hip._need_gpu(label_img, mask_image)
    if max_label is None:
        max_label = int(label_img.max())
    if max_label < 1:
        return []
    verts, faces, normals, nv, nf = F_hip.marching_cubes_labels(label_img, 1, int(max_label), spacing=spacing, mask=mask_image)
    return [Meshes([v], [f], [n]) for v, f, n in zip(verts.split(nv), faces.split(nf), normals.split(nv))]
