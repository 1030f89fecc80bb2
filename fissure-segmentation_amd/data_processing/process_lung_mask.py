"""Binary lung mask -> left / right lung mask with the reference's names (data_processing/process_lung_mask.py:11-93), tensors
in, tensors out: no SimpleITK, no file I/O (the reference's `__main__` loop over a dataset is not mirrored).  Convert an
image with `torch.from_numpy(sitk.GetArrayFromImage(img))` on the way in and `GetImageFromArray(t.cpu().numpy())` +
`CopyInformation` on the way out.  Connected components, opening and statistics are the bit-plane launches of
csrc/morphology.hip, the restoration of opened-away voxels is the distance transform of csrc/edt.hip."""
import warnings

import torch

from .. import functional as F_hip
from .. import _lib


def check_left_right_lung_plausible(component_sizes, max_volume_ratio=10):
    """process_lung_mask.py:11-28, same rule, same messages, same warning: at least two components, and the largest at most
    `max_volume_ratio` times the second largest."""
    component_sizes = sorted(component_sizes, reverse=True)
    if len(component_sizes) < 2:
        print('Implausible mask: only one component.')
        return False
    ratio = component_sizes[0] / component_sizes[1]
    if ratio > max_volume_ratio:
        print(f'Implausible volume-ratio of first/second largest component: {ratio}')
        return False
    if len(component_sizes) > 2:
        print(component_sizes)
        warnings.warn(f'Found {len(component_sizes)} connected components in lung mask, but expected 2. '
                      f'Assuming the biggest 2 components are the right & left lung.')
    return True


def maybe_detach_mask(lung_mask: torch.Tensor, opening_radius: int = 3, _opened: bool = False):
    """process_lung_mask.py:31-52 for a tensor (D, H, W), bool or integer -> (components int32, n, opened): the 6-connected
    components of the mask if their sizes are plausible, otherwise those of the mask opened with the ball of `opening_radius`,
    then of radius + 2, ...  Sizes are voxel counts: the reference's physical sizes are these times the voxel volume, and
    only their ratio is used.
    Where this is NOT the reference: `functional.binary_opening` takes radii up to 8, so the chain is 3, 5, 7; when radius 9
    would be next a ValueError says that the mask could not be detached (the reference recurses without end there).  The ball
    is `functional.ball_offsets`, parity with sitkBall is unpinned.  Two host reads per round (component count, sizes)."""
    if lung_mask.dim() != 3:
        raise ValueError(f"maybe_detach_mask: expected a volume (D, H, W), got {tuple(lung_mask.shape)}")
    labels, n = F_hip.connected_components(lung_mask, 6)
    sizes = F_hip.component_stats(labels, n)[0].tolist() if n else []
    if check_left_right_lung_plausible(sizes):
        print('Done')
        return labels, n, _opened
    if opening_radius > _lib.MORPH_MAX_RADIUS:
        raise ValueError(f"maybe_detach_mask: the lung mask could not be detached into two plausible components by openings up "
                         f"to radius {opening_radius - 2} (the next, {opening_radius}, is above the largest ball, "
                         f"{_lib.MORPH_MAX_RADIUS})")
    print(f'Opening with radius {opening_radius} to detach left and right lung.')
    return maybe_detach_mask(F_hip.binary_opening(lung_mask, opening_radius), opening_radius + 2, _opened=True)


def binary_lung_mask_to_left_right(lung_mask: torch.Tensor, left_label: int = 1, right_label: int = 2) -> torch.Tensor:
    """process_lung_mask.py:55-93 for a tensor (D, H, W), bool or integer -> uint8 (D, H, W): the two largest components of
    the (maybe opened) mask, the one with the smaller centroid along the last axis (x) labelled `right_label`, the other
    `left_label`.  If an opening was needed, every voxel of the original mask gets the nearer of the two lungs
    (`functional.nearest_label`, unit spacing as the reference's scipy call, ties to the left lung as np.argmin gives label
    1), and everything outside the mask is 0.
    Where this is NOT the reference: centroids are taken in index space from the exact integer sums of `component_stats`,
    which orders them as the reference's physical centroids do only for a positive x direction and spacing; with labels other
    than 1 / 2 the reference's restoration still measures distances to the labels 1 and 2 (:85), whatever they were renamed
    to -- here the restoration runs on 1 / 2 and the renaming comes last, so non-default labels work."""
    if not (0 < int(left_label) < 256 and 0 < int(right_label) < 256 and int(left_label) != int(right_label)):
        raise ValueError(f"binary_lung_mask_to_left_right: labels must be two different values in 1..255, got {left_label!r}, "
                         f"{right_label!r}")
    components, n, opened = maybe_detach_mask(lung_mask)
    with torch.no_grad():
        two = F_hip.relabel_by_size(components, n)                                  # :59-62
        two = torch.where(two <= 2, two, torch.zeros_like(two))                      # :64-67
        sizes, sums = F_hip.component_stats(two, 2)                                  # :69-73, centroids as integer sums
        cx = sums[:, 2].double() / sizes.double()
        left_is_first = cx[0] > cx[1]                                                # smaller x is right; a tie leaves 1 right
        lut = torch.zeros(3, dtype=torch.int32, device=two.device)
        lut[1] = torch.where(left_is_first, 1, 2)
        lut[2] = torch.where(left_is_first, 2, 1)
        left_right = F_hip._apply_lut(two[None], lut[None])[0]                       # :75-78 with left = 1, right = 2
        if opened:                                                                   # :80-91
            left_right = F_hip.nearest_label(left_right, (1, 2), keep=(lung_mask != 0))
        out = torch.tensor([0, int(left_label), int(right_label)], dtype=torch.uint8, device=two.device)[left_right.long()]
    return out
