"""Drop-in for the filtering part of the reference's utils/image_utils.py (:6-50).  `filter_1d` and `smooth` are the same
ATen calls as the reference's and run wherever their input is (the fused kernels of csrc/volume.hip carry their own copy of
this smoothing and never call them); `nms` is the HIP window maximum (fsg_nms_keypoints) and needs a GPU tensor."""
import torch
from torch.nn import functional as F

from .. import functional as F_hip


def filter_1d(img, weight, dim, padding_mode='replicate'):
    """image_utils.py:6-19: cross-correlate (B, C, D, H, W) with the 1-D `weight` along spatial axis `dim` (0, 1, 2)"""
    B, C, D, H, W = img.shape
    N = weight.shape[0]
    padding = [0] * 6
    padding[4 - 2 * dim] = padding[5 - 2 * dim] = N // 2
    view = [1] * 5
    view[dim + 2] = -1
    return F.conv3d(F.pad(img.reshape(B * C, 1, D, H, W), padding, mode=padding_mode), weight.view(view)).view(B, C, D, H, W)


def smooth(img, sigma):
    """image_utils.py:22-35: separable Gaussian, N = 2 ceil(1.5 sigma) + 1 taps, axes 0, 1, 2, replicate padding"""
    weight = F_hip.gaussian_taps(sigma).to(img.device)
    for dim in range(3):
        img = filter_1d(img, weight, dim)
    return img


def nms(data: torch.Tensor, kernel_size: int):
    """image_utils.py:38-50: the window maximum used for non-maximum suppression, (B, 1, D, H, W) -> same shape.  Even kernels
    reach one voxel further forward than backward; NaN propagates through a window."""
    return F_hip.nms_max(data, kernel_size)
