"""Hessian-based fissure enhancement with the reference's names (data_processing/fissure_enhancement.py:30-220), tensors in,
tensors out: no SimpleITK, no CSV of fissure statistics.  The filter is one fused launch (csrc/fissure_enhance.hip) over the
whole volume; `hessian_matrix` and `fissure_filter` are kept as plain torch for callers that want the intermediate tensors
(nothing on the hot path does)."""
import torch
from torch import nn

from .. import functional as F_hip
from ..utils.image_utils import filter_1d


class HessianEnhancementFilter(nn.Module):
    """fissure_enhancement.py:30-99.  `gaussian_smoothing_sigma` is accepted and has no effect, as in the reference: its
    forward smooths the image into `img_smooth` and never uses it (:49-54).  The derivation sigma is at most 1."""

    def __init__(self, fissure_mu, fissure_sigma, gaussian_smoothing_sigma=1., gaussian_derivation_sigma=1.):
        super().__init__()
        self.fissure_mu = float(fissure_mu)
        self.fissure_sigma = float(fissure_sigma)
        self.gaussian_smoothing_sigma = float(gaussian_smoothing_sigma)
        self.gaussian_derivation_sigma = float(gaussian_derivation_sigma)
        F_hip.fissure_enhance_check_sigma(self.gaussian_derivation_sigma)

    def forward(self, img, return_intermediate=False, mask=None):
        """img (1, 1, D, H, W) -> F (1, 1, D, H, W), or (F, P, hu_weights) with P and hu_weights (D, H, W) as the reference
        returns them; `mask` (the shape of img) multiplies F by (mask != 0) in the same launch"""
        out = F_hip.fissure_enhance(img, self.fissure_mu, self.fissure_sigma, self.gaussian_derivation_sigma, mask=mask,
                                    return_intermediate=return_intermediate)
        if not return_intermediate:
            return out
        return out[0], out[1].squeeze(), out[2].squeeze()


def hessian_matrix(img: torch.Tensor, sigma: float):
    """fissure_enhancement.py:102-125 in plain torch: img (1, 1, D, H, W) -> (D, H, W, 3, 3).  Needs 36 bytes per voxel; the
    fused filter never forms it."""
    k1 = F_hip.gaussian_derivative_taps(sigma, 1).to(img.device)
    k2 = F_hip.gaussian_derivative_taps(sigma, 2).to(img.device)
    img = img.float()
    H = torch.zeros(*img.shape[2:], 3, 3, device=img.device)
    for a in range(3):
        H[..., a, a] = filter_1d(img, k2, a)[0, 0]
        for b in range(a + 1, 3):
            H[..., a, b] = H[..., b, a] = filter_1d(filter_1d(img, k1, a), k1, b)[0, 0]
    return H


def fissure_filter(img, hessian_lambda1, hessian_lambda2, fissure_mu, fissure_sigma, return_intermediate=False):
    """fissure_enhancement.py:149-180 for tensors: planeness of the two dominant eigenvalues times the HU weight"""
    a1, a2 = hessian_lambda1.abs(), hessian_lambda2.abs()
    neg = hessian_lambda1 < 0
    P = torch.zeros_like(hessian_lambda1)
    P[neg] = (a1[neg] - a2[neg]) / (a1[neg] + a2[neg])
    hu_weights = torch.exp(-((img - fissure_mu) ** 2) / (2 * fissure_sigma ** 2))
    F = hu_weights * P
    return (F, P, hu_weights) if return_intermediate else F


def hessian_based_enhancement_torch(img: torch.Tensor, fissure_mu: float, fissure_sigma: float, device=None,
                                    gaussian_smoothing_sigma=1., gaussian_derivation_sigma=1.):
    """fissure_enhancement.py:128-146: img (D, H, W) (leading singleton axes allowed) -> (D, H, W), the whole volume in one
    launch.  Deviation: on a GPU the reference blends overlapping 64^3 patches with a Gaussian, because its (D, H, W, 3, 3)
    tensor does not fit; the whole-volume result returned here is what its own CPU branch returns, without patch borders."""
    img = img.squeeze()
    img = img.view(1, 1, *img.shape).float()
    if device is not None:
        img = img.to(device)
    filt = HessianEnhancementFilter(fissure_mu, fissure_sigma, gaussian_smoothing_sigma, gaussian_derivation_sigma)
    return filt(img).squeeze()


def get_enhanced_fissure_image(img, mask, fissure_mu, fissure_sigma):
    """fissure_enhancement.py:201-220 for tensors: img, mask (1, 1, D, H, W) on the GPU -> the enhanced image with everything
    outside the lung mask set to 0, (1, 1, D, H, W).  The fissure statistics are arguments, not a CSV file."""
    return F_hip.fissure_enhance(img, fissure_mu, fissure_sigma, 1.0, mask=mask)
