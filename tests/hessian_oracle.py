"""Oracle of the Hessian fissure enhancement: a restatement in torch on the CPU of the reference's
data_processing/fissure_enhancement.py:47-99, 149-180 (filter), :213-214 (lung mask) and
data_processing/keypoint_extraction.py:134-141 (smoothing, top-k, threshold), runnable in fp32 and fp64.  The taps are
computed as the reference computes them (scipy's Gaussian kernel, cast to fp32) and then cast, so an fp64 run differs from an
fp32 run by the rounding of the arithmetic alone.  The seeded inputs are those of tests/frontend_oracle.py.

tests/golden/hessian_enhance.npz holds what the REAL reference returned for the golden volumes; tests/test_hessian_cpu.py
holds this file to it.  The smoothing taps are ITK's documented discrete Gaussian (exp(-t) I_k(t)); SimpleITK itself is not
available to pin them."""
import numpy as np
import torch
import torch.nn.functional as F
from scipy.ndimage._filters import _gaussian_kernel1d
from scipy.special import ive

import frontend_oracle as fo

MU, SIGMA_HU = -400.0, 250.0
BLOCK_VALUE = -1000.0
RADIUS = 4                                   # of the derivative taps at sigma 1
DISCRETE_GAUSSIAN_VAR1 = (0.008174, 0.050050, 0.208375, 0.466801, 0.208375, 0.050050, 0.008174)
KPT_CASES = (("golden", 500), ("large", 20000), ("large", 200000))   # (volume, K)
THRESHOLD = 0.2


# ------------------------------------------------------------------ seeded inputs
def volume(name, block=None):
    """'golden' | 'large' | 'e2e' -> (img (1, 1, D, H, W) fp32, mask (1, 1, D, H, W) bool); `block`: None, 0.0 or -1000.0, the
    value of a constant corner block (frontend_oracle.ct_volume's constant_block, with another constant)"""
    seed, shape = {"golden": (fo.GOLDEN_SEED, fo.GOLDEN_SHAPE), "large": (fo.LARGE_SEED, fo.LARGE_SHAPE),
                   "e2e": (fo.E2E_SEED, fo.E2E_SHAPE)}[name]
    img = fo.ct_volume(seed, shape, constant_block=block is not None)
    if block is not None:
        d, h, w = shape
        assert bool((img[0, 0, : d // 3, : h // 3, : w // 3] == 0).all())
        img[0, 0, : d // 3, : h // 3, : w // 3] = block
    return img, fo.box_mask(shape)


def constant_support(img, radius=RADIUS):
    """voxels whose whole (2 radius + 1)^3 stencil support (replicate padding) is constant -> (D, H, W) bool"""
    p = F.pad(img.double(), (radius,) * 6, mode="replicate")
    k = 2 * radius + 1
    return (F.max_pool3d(p, k, stride=1) == -F.max_pool3d(-p, k, stride=1))[0, 0]


# ------------------------------------------------------------------ filter
def derivative_taps(sigma, order, truncate=4.0):
    """utils/image_utils.py:53-58 -> fp32"""
    return torch.from_numpy(_gaussian_kernel1d(float(sigma), order, int(truncate * float(sigma) + 0.5))).float()


def hessian(img, sigma=1.0):
    """fissure_enhancement.py:81-99: (1, 1, D, H, W) -> (D, H, W, 3, 3) in img's dtype"""
    k1, k2 = derivative_taps(sigma, 1), derivative_taps(sigma, 2)
    H = torch.zeros(*img.shape[2:], 3, 3, dtype=img.dtype, device=img.device)
    for a in range(3):
        H[..., a, a] = fo.filter_1d(img, k2, a)[0, 0]
        for b in range(a + 1, 3):
            H[..., a, b] = H[..., b, a] = fo.filter_1d(fo.filter_1d(img, k1, a), k1, b)[0, 0]
    return H


def enhance(img, mu=MU, sigma_hu=SIGMA_HU, sigma=1.0, mask=None):
    """-> (F, P, hu_weights), each (D, H, W) in img's dtype; F is multiplied by the mask when one is given"""
    ev = torch.linalg.eigvalsh(hessian(img, sigma))
    ev = torch.gather(ev, -1, torch.argsort(ev.abs(), dim=-1, descending=True))
    l1, l2 = ev[..., 0], ev[..., 1]
    P = torch.zeros_like(l1)
    neg = l1 < 0
    P[neg] = (l1[neg].abs() - l2[neg].abs()) / (l1[neg].abs() + l2[neg].abs())
    hw = torch.exp(-((img[0, 0] - mu) ** 2) / (2 * sigma_hu ** 2))
    Fv = hw * P
    if mask is not None:
        Fv = Fv * mask[0, 0].to(Fv.dtype)
    return Fv, P, hw


# ------------------------------------------------------------------ keypoints
def discrete_gaussian_taps(variance, max_error=0.01, max_width=32):
    """ITK's GaussianOperator as documented: exp(-t) I_k(t), terms until the sum reaches 1 - max_error, normalised -> fp32"""
    half = [ive(0, variance)]
    while half[0] + 2 * sum(half[1:]) < 1 - max_error and 2 * len(half) + 1 <= max_width:
        half.append(ive(len(half), variance))
    full = np.array(half[:0:-1] + half)
    return torch.from_numpy(full / full.sum()).float()


def smooth(vol, taps):
    """(1, 1, D, H, W), three tap vectors (z, y, x) -> separable smoothing, axes 0, 1, 2, replicate padding"""
    for ax in range(3):
        vol = fo.filter_1d(vol, taps[ax], ax)
    return vol


def select(smoothed, thresh=THRESHOLD, K=20000):
    """keypoint_extraction.py:138-140 with a defined order: the K largest voxels, those above thresh -> (K', 3) int64 (z, y,
    x) by value descending, ties by linear index ascending"""
    v = smoothed.flatten()
    order = torch.sort(v, descending=True, stable=True).indices[:K]
    order = order[v[order] > thresh]
    D, H, W = smoothed.shape[-3:]
    return torch.stack([order // (H * W), (order // W) % H, order % W], 1)


def ambiguity(s64, s32, thresh, K):
    """-> (tau, ambiguous (D, H, W) bool, selected count): voxels of the fp64 field within tau = 10 x the fp32 oracle's maximum
    absolute error of the threshold or of the K-th largest value (when the volume has more than K voxels above thresh)"""
    v = s64.flatten()
    tau = 10 * float((s32.double() - s64).abs().max())
    above = v[v > thresh]
    amb = (s64 - thresh).abs() <= tau
    if above.numel() > K:
        kth = torch.sort(above, descending=True).values[K - 1]
        amb |= (s64 - kth).abs() <= tau
    return tau, amb[0, 0], min(K, above.numel())
