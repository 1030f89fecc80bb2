"""Lobe filling and lobes-to-fissures with the reference's names (data_processing/find_lobes.py:17-92), tensors in, tensors
out: no SimpleITK.  Convert an image with `torch.from_numpy(sitk.GetArrayFromImage(img).astype(int))` on the way in and
`GetImageFromArray(t.cpu().numpy())` + `CopyInformation` on the way out, as the reference does around the same calls.  The
connected-component and marching-cubes parts of the reference's module (find_lobes, compute_surface_mesh_marching_cubes) are
not here."""
import torch

from .. import functional as F_hip


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
