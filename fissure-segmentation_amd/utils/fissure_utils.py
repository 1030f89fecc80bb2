"""utils/fissure_utils.py of the reference for tensors: the binary fissure segmentation of the voxel CNN becomes a left / right
fissure label map (train_segmentation_net.py:75-148, after the argmax and before `poisson_reconstruction`)."""
import torch

from .image_ops import resample_equal_spacing

LEFT_LABEL, RIGHT_LABEL = 1, 2


def binary_to_fissure_segmentation(binary_fissure_seg: torch.Tensor, lr_lung_mask: torch.Tensor, spacing=None, resample_spacing=None):
    """fissure_utils.py:7-29: `binary_fissure_seg` (D, H, W), nonzero = fissure, is edited IN PLACE and returned: voxels outside
    the lungs become 0, set voxels get the label of their lung, 1 = left and 2 = right in `lr_lung_mask` (any other lung value
    leaves a set voxel as it is, like the reference).

    resample_spacing: the lung mask is first brought to that equal spacing with
    `resample_equal_spacing(..., use_nearest_neighbor=True)` (csrc/spatial.hip; on the GPU), which needs `spacing`, the mask's
    voxel spacing in the tensor's axis order -- the reference's sitk.Image carried it; ValueError without.  The resampled mask
    must have the shape of the segmentation.  With resample_spacing=None this is plain torch on any device."""
    if resample_spacing is not None:
        if spacing is None:
            raise ValueError("binary_to_fissure_segmentation: resample_spacing needs the lung mask's `spacing`")
        lr_lung_mask, _ = resample_equal_spacing(lr_lung_mask, spacing, target_spacing=resample_spacing, use_nearest_neighbor=True)
    lung = lr_lung_mask.to(binary_fissure_seg.device)
    if tuple(lung.shape) != tuple(binary_fissure_seg.shape):
        raise ValueError(f"binary_to_fissure_segmentation: lung mask {tuple(lung.shape)} for a segmentation "
                         f"{tuple(binary_fissure_seg.shape)}")
    binary_fissure_seg[lung == 0] = 0                            # discard non lung voxels
    binary_fissure_seg[torch.logical_and(binary_fissure_seg, lung == LEFT_LABEL)] = LEFT_LABEL
    binary_fissure_seg[torch.logical_and(binary_fissure_seg, lung == RIGHT_LABEL)] = RIGHT_LABEL
    return binary_fissure_seg
