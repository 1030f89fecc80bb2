"""Image front end: Foerstner keypoints, MIND (csrc/volume.hip); Hessian fissure enhancement (csrc/fissure_enhance.hip)."""
import ctypes

import torch

from .. import _lib
from .._launch import _f32c, _need_gpu, _p, launch


# ------------------------------------------------------------------ image front end: Foerstner keypoints, MIND (csrc/volume.hip)
def gaussian_taps(sigma):
    """the taps of utils/image_utils.py:25-29 (N = 2 ceil(1.5 sigma) + 1, normalised in fp32), computed the same way, on the
    host -> (N,) fp32 CPU tensor"""
    s = torch.tensor([float(sigma)])
    n = int(torch.ceil(s * 3.0 / 2.0).long().item()) * 2 + 1
    w = torch.exp(-torch.pow(torch.linspace(-(n // 2), n // 2, n), 2) / (2 * torch.pow(s, 2)))
    w /= w.sum()
    return w


def _host_floats(t):
    vals = [float(v) for v in t.tolist()]
    return (ctypes.c_float * len(vals))(*vals), len(vals)


def _host_ints(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int * len(vals))(*vals)


def _volume(img, what="img"):
    """(B, 1, D, H, W) -> contiguous fp32 and its four sizes"""
    if img.dim() != 5 or img.shape[1] != 1:
        raise ValueError(f"expected {what} (B, 1, D, H, W), got {tuple(img.shape)}")
    v = _f32c(img)
    return v, (v.shape[0], v.shape[2], v.shape[3], v.shape[4])


def foerstner_distinctiveness(img, sigma):
    """data_processing/foerstner.py:62-73 in one launch (fsg_foerstner_dist_f32): img (B, 1, D, H, W) -> (B, 1, D, H, W).
    NaN where the smoothed structure tensor is singular, like the reference."""
    _need_gpu(img)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        w, n = _host_floats(gaussian_taps(sigma))
        out = torch.empty_like(v)
        launch(v.device, "fsg_foerstner_dist_f32", _p(v), B, D, H, W, w, n, _p(out))
    return out


def _mask_bytes(mask, shape):
    if mask is None:
        return None
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the volume {tuple(shape)}")
    return (mask != 0).to(torch.uint8).contiguous()


def nms_max(data, kernel_size):
    """utils/image_utils.py:38-50 (fsg_nms_keypoints): window maximum with the reference's asymmetric padding for even
    kernels; NaN propagates.  data (B, 1, D, H, W) -> same shape"""
    _need_gpu(data)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(data, "data")
        out = torch.empty_like(v)
        launch(v.device, "fsg_nms_keypoints", _p(v), None, B, D, H, W, int(kernel_size), 0.0, _p(out), None)
    return out


def nms_keypoint_flags(dist, mask, d, thresh):
    """foerstner.py:90-107 without the nonzero: eroded(mask) & (window max == dist) & (dist >= thresh) -> (B, 1, D, H, W) bool"""
    _need_gpu(dist, mask)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(dist, "dist")
        m = _mask_bytes(mask, v.shape)
        flags = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
        launch(v.device, "fsg_nms_keypoints", _p(v), _p(m), B, D, H, W, int(d), float(thresh), None, _p(flags))
    return flags.bool()


def _mind_tables(shifts, outch):
    nch = len(shifts)
    flat = [int(v) for pair in shifts for voxel in pair for v in (voxel if isinstance(voxel, (tuple, list)) else (voxel,))]
    return nch, _host_ints(flat), _host_ints(outch if outch is not None else range(nch))


def mind_mean(img, dilation, sigma, shifts, box):
    """statistics pass (fsg_mind_stats_f32): the mean over the batch volume of mean_c(ssd_c - min_c ssd_c) -> (1,) fp32 on the
    device.  `shifts`: per channel the two voxel offsets ((dz, dy, dx), (dz, dy, dx)) in {-1, 0, 1}; with `box`, per channel two
    27-bit subsets of the 3 x 3 x 3 stencil whose sums are compared."""
    _need_gpu(img)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        nch, sh, _ = _mind_tables(shifts, None)
        w, n = _host_floats(gaussian_taps(sigma))
        ws = _lib.workspace("fsg_mind_stats", B, D, H, W, device=v.device)
        mean = torch.empty(1, dtype=torch.float32, device=v.device)
        launch(v.device, "fsg_mind_stats_f32", _p(v), B, D, H, W, int(dilation), nch, int(box), sh, w, n, _p(ws), _p(mean))
    return mean


def mind_volume(img, dilation, sigma, shifts, outch, box, mean=None):
    """statistics + evaluation pass for the whole volume -> (B, nch, D, H, W)"""
    _need_gpu(img)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        if mean is None:
            mean = mind_mean(v, dilation, sigma, shifts, box)
        nch, sh, oc = _mind_tables(shifts, outch)
        w, n = _host_floats(gaussian_taps(sigma))
        out = torch.empty(B, nch, D, H, W, dtype=torch.float32, device=v.device)
        launch(v.device, "fsg_mind_eval_f32", _p(v), B, D, H, W, int(dilation), nch, int(box), sh, oc, w, n, _p(mean), _p(out))
    return out


def mind_keypoints(img, kp, dilation, sigma, shifts, outch, box, mean=None):
    """statistics pass + evaluation at kp (K, 3) voxel indices (z, y, x) of ONE volume -> (nch, K); the feature volume is
    never written"""
    _need_gpu(img, kp)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        if B != 1:
            raise ValueError("mind_keypoints: one volume at a time")
        if kp.dim() != 2 or kp.shape[1] != 3 or kp.is_floating_point():
            raise ValueError(f"expected kp (K, 3) integer voxel indices, got {tuple(kp.shape)} {kp.dtype}")
        nch, sh, oc = _mind_tables(shifts, outch)
        K = kp.shape[0]
        out = torch.empty(nch, K, dtype=torch.float32, device=v.device)
        if K == 0:
            return out
        kpc = kp.detach().to(torch.int64).contiguous()
        lo, hi = kpc.amin(0).tolist(), kpc.amax(0).tolist()
        if min(lo) < 0 or any(h >= s for h, s in zip(hi, (D, H, W))):
            raise ValueError(f"keypoints span {lo}..{hi}, outside the volume {(D, H, W)}")
        if mean is None:
            mean = mind_mean(v, dilation, sigma, shifts, box)
        w, n = _host_floats(gaussian_taps(sigma))
        launch(v.device, "fsg_mind_eval_kp_f32", _p(v), D, H, W, int(dilation), nch, int(box), sh, oc, w, n, _p(mean), _p(kpc), K,
               _p(out))
    return out


# ------------------------------------------------------------------ Hessian fissure enhancement (csrc/fissure_enhance.hip)
MAX_TAP_RADIUS = _lib.ENHANCE_MAX_TAP_RADIUS   # of the derivative taps (derivation sigma <= 1) and of the keypoint smoothing taps


def gaussian_derivative_taps(sigma, order, truncate=4.0):
    """utils/image_utils.py:53-58 (scipy's Gaussian kernel of derivative `order`, radius int(truncate sigma + 0.5)), computed
    the same way in fp64 on the host and cast -> (2 radius + 1,) fp32 CPU tensor"""
    import numpy as np
    sigma, order = float(sigma), int(order)
    if not sigma > 0 or order < 0:
        raise ValueError(f"gaussian_derivative_taps: sigma {sigma} must be positive and order {order} non-negative")
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    if order > 0:   # q <- q' + q p', p' = -x / sigma^2, applied to the coefficients of q `order` times
        exponents = np.arange(order + 1)
        q = np.zeros(order + 1)
        q[0] = 1
        step = np.diag(exponents[1:], 1) + np.diag(np.ones(order) / -(sigma * sigma), -1)
        for _ in range(order):
            q = step.dot(q)
        phi = (x[:, None] ** exponents).dot(q) * phi
    return torch.from_numpy(phi).float()


def discrete_gaussian_taps(variance, max_error=0.01, max_width=32, spacing=None):
    """the operator of ITK's DiscreteGaussianImageFilter as ITK documents it (GaussianOperator): coefficients exp(-t) I_k(t),
    t the variance in voxels, terms added until their sum reaches 1 - max_error (or the width reaches max_width), then
    normalised.  `variance` is a number or one per axis (z, y, x); with `spacing` (z, y, x) it is physical and becomes
    variance / spacing^2 per axis (useImageSpacing).  -> three fp32 CPU tensors (z, y, x).  Parity with SimpleITK itself is
    not pinned by a test; pass explicit taps to `smooth_threshold` to use SimpleITK's."""
    from scipy.special import ive
    var = [float(variance)] * 3 if not hasattr(variance, "__len__") else [float(v) for v in variance]
    sp = [1.0] * 3 if spacing is None else [float(s) for s in spacing]
    if len(var) != 3 or len(sp) != 3 or min(var) < 0 or min(sp) <= 0:
        raise ValueError(f"discrete_gaussian_taps: variance {variance} / spacing {spacing} must be three non-negative / positive numbers")
    taps = []
    for v, s in zip(var, sp):
        t = v / (s * s)
        half = [float(ive(0, t))]
        total = half[0]
        while total < 1.0 - max_error and 2 * len(half) + 1 <= max_width:
            half.append(float(ive(len(half), t)))
            total += 2 * half[-1]
        full = half[:0:-1] + half
        taps.append((torch.tensor(full, dtype=torch.float64) / total).float())
    return tuple(taps)


def _odd_taps(t, what):
    t = torch.as_tensor(t, dtype=torch.float32).detach().cpu().flatten()
    if t.numel() % 2 == 0 or t.numel() > 2 * MAX_TAP_RADIUS + 1:
        raise ValueError(f"{what}: {t.numel()} taps; the kernel takes an odd number, at most {2 * MAX_TAP_RADIUS + 1} "
                         f"(radius {MAX_TAP_RADIUS})")
    return t


def fissure_enhance_check_sigma(derivation_sigma):
    """the derivative taps of `derivation_sigma` must fit the kernel's radius (1..4): -> (k1, k2) fp32 CPU tensors"""
    k1, k2 = gaussian_derivative_taps(derivation_sigma, 1), gaussian_derivative_taps(derivation_sigma, 2)
    if k1.numel() > 2 * MAX_TAP_RADIUS + 1 or k1.numel() < 3:
        raise ValueError(f"fissure_enhance: derivation sigma {derivation_sigma} gives a tap radius of {k1.numel() // 2}; the "
                         f"kernel takes 1..{MAX_TAP_RADIUS} (sigma <= 1)")
    return k1, k2


def fissure_enhance(img, fissure_mu, fissure_sigma, derivation_sigma=1.0, mask=None, return_intermediate=False):
    """HessianEnhancementFilter.forward + fissure_filter (data_processing/fissure_enhancement.py:47-99, 149-180) in one launch
    (fsg_fissure_enhance_f32): img (B, 1, D, H, W) -> F of the same shape, times (mask != 0) when a mask of that shape is
    given; with `return_intermediate` -> (F, planeness, HU weight).  The derivation sigma is at most 1 (tap radius 4)."""
    k1, k2 = fissure_enhance_check_sigma(derivation_sigma)
    if not float(fissure_sigma) > 0:
        raise ValueError(f"fissure_enhance: fissure_sigma {fissure_sigma} must be positive")
    _need_gpu(img, mask)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        if mask is not None and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous() and mask.shape == v.shape:
            m = mask.view(torch.uint8)          # the kernel tests the byte against 0: no dense conversion pass
        else:
            m = _mask_bytes(mask, v.shape)
        out = torch.empty_like(v)
        P, hw = (torch.empty_like(v), torch.empty_like(v)) if return_intermediate else (None, None)
        w1, n = _host_floats(k1)
        w2, _ = _host_floats(k2)
        launch(v.device, "fsg_fissure_enhance_f32", _p(v), _p(m), B, D, H, W, w1, w2, n, float(fissure_mu), float(fissure_sigma),
               _p(out), _p(P), _p(hw))
    return (out, P, hw) if return_intermediate else out


def smooth_threshold(vol, taps, thresh, return_flags=True):
    """fsg_smooth_threshold_f32: vol (B, 1, D, H, W) smoothed separably with `taps` = (taps_z, taps_y, taps_x) (odd counts,
    radius <= 4; axis order 0, 1, 2; replicate padding) -> (values, flags): the smoothed value where it exceeds `thresh` and 0
    elsewhere, and that comparison as (B, 1, D, H, W) bool (values alone with return_flags=False)"""
    if len(taps) != 3:
        raise ValueError("smooth_threshold: expected three tap vectors (z, y, x)")
    host = [_host_floats(_odd_taps(t, f"smooth_threshold: axis {ax}")) for ax, t in enumerate(taps)]
    _need_gpu(vol)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(vol, "vol")
        out = torch.empty_like(v)
        flags = torch.empty(v.shape, dtype=torch.uint8, device=v.device) if return_flags else None
        launch(v.device, "fsg_smooth_threshold_f32", _p(v), B, D, H, W, host[0][0], host[0][1], host[1][0], host[1][1], host[2][0],
               host[2][1], float(thresh), _p(out), _p(flags))
    return (out, flags.view(torch.bool)) if return_flags else out   # the kernel writes 0 or 1: a view, not a pass
