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


def gaussian_derivative_taps(sigma, order=0, truncate=4.0):
    """image_utils.py:53-58: the taps scipy.ndimage builds for a Gaussian (derivative) filter, radius int(truncate sigma + 0.5),
    computed without scipy in fp64 and rounded to fp32: phi(x) = exp(-x^2 / (2 sigma^2)) normalised to sum 1, times the
    polynomial q_order(x), q_0 = 1, q_{n+1} = q_n' - x q_n / sigma^2 (not reversed: the reference takes scipy's kernel as it is and
    cross-correlates) -> (2 r + 1,)"""
    sigma = float(sigma)
    if order < 0 or sigma <= 0:
        raise ValueError(f"need order >= 0 and sigma > 0, got order {order}, sigma {sigma}")
    radius = int(truncate * sigma + 0.5)
    x = torch.arange(-radius, radius + 1, dtype=torch.float64)
    phi = torch.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    q = [1.0]                                    # coefficients of q_n, lowest power first
    for _ in range(order):
        dq = [k * q[k] for k in range(1, len(q))] + [0.0, 0.0]
        xq = [0.0] + [-c / (sigma * sigma) for c in q]
        q = [a + b for a, b in zip(dq + [0.0] * (len(xq) - len(dq)), xq)]
    poly = sum(c * x ** k for k, c in enumerate(q))
    return (poly * phi).float()


def gaussian_differentiation(img, sigma, order, dim, padding_mode='replicate', truncate=4.0):
    """image_utils.py:61-64: Gaussian smoothing and `order`-fold differentiation along spatial axis `dim` of (B, C, D, H, W)
    in one 1-D filter (a torch convolution, like `filter_1d`)"""
    weight = gaussian_derivative_taps(sigma, order, truncate).to(img.device)
    return filter_1d(img, weight, dim, padding_mode)
