"""From a volume and a lung mask to the point cloud of the point networks (the tensor part of the reference's
data_processing/keypoint_extraction.py and point_features.py:163-203), tensors in, tensors out: no SimpleITK, no files."""
import torch

from ..utils.general_utils import ALIGN_CORNERS, kpts_to_grid, sample_patches_at_kpts
from .. import functional as F_hip
from . import foerstner
from .point_features import image_patch_features, mind_at_keypoints

MAX_KPTS = 20000            # the reference's cap on the size of a cloud
FEATURE_MODES = (None, 'mind', 'mind_ssc', 'image')
ENHANCEMENT_FEATURE_MODES = FEATURE_MODES + ('enhancement',)   # of enhancement_point_cloud
HU_AIR, HU_WATER = -1000.0, 0.0   # 'image' patches are scaled so that air is -1 and water +1 (reference: normalize_img, max_val=0)


def limit_keypoints(kp, max_num_kpts=MAX_KPTS):
    """-> (kp, index): at most `max_num_kpts` rows of kp, drawn without replacement when there are more, and the row
    indices that were kept (on kp's device when drawn; all rows, in order, otherwise)"""
    n = kp.shape[0]
    if n <= max_num_kpts:
        return kp, torch.arange(n)
    index = torch.randperm(n, device=kp.device)[:max_num_kpts]
    return kp[index], index


def foerstner_point_cloud(img, mask, spacing=(1, 1, 1), sigma=0.5, threshold=1e-8, nms_kernel=5, feature_mode=None):
    """img, mask (1, 1, D, H, W) on the GPU, spacing (z, y, x) -> (C, K) fp32: rows 0..2 the keypoints in grid coordinates
    (x, y, z) in [-1, 1], then the features of `feature_mode` (None: none, 'mind': 6, 'mind_ssc': 12, 'image': the 125
    voxels of a 5^3 patch, intensities mapped linearly so that -1000 HU is -1 and 0 HU is +1 as the reference does for this
    mode).  At most MAX_KPTS keypoints (a random subset beyond that).  The result, with a batch axis in front, is what
    `predict_full_pointcloud` takes."""
    if feature_mode not in FEATURE_MODES:
        raise ValueError(f'unknown feature_mode {feature_mode!r}: expected one of {FEATURE_MODES}')
    kp = foerstner.foerstner_kpts(img, mask, sigma=sigma, d=nms_kernel, thresh=threshold)
    kp, _ = limit_keypoints(kp)
    points = keypoints_to_grid(kp, img.shape[2:], spacing)
    if feature_mode is None:
        return points.contiguous()
    if feature_mode == 'image':
        feat = image_patch_features(img.float(), points.transpose(0, 1), patch_size=5)
        feat = (feat - HU_AIR) / (HU_WATER - HU_AIR) * 2 - 1
    else:
        feat = mind_at_keypoints(img, kp, dilation=1, sigma=0.8, ssc=feature_mode == 'mind_ssc')
    return torch.cat([points, feat], dim=0).contiguous()


def hessian_enhancement_kpts(enhanced, min_threshold=0.2, max_kpts=MAX_KPTS, spacing=(1, 1, 1), taps=None):
    """keypoint_extraction.py:134-141: enhanced (1, 1, D, H, W) on the GPU -> (K', 3) int64 voxel indices (z, y, x) of the at
    most `max_kpts` largest voxels of the smoothed image that exceed `min_threshold`, by value descending, ties by linear
    voxel index ascending.  The smoothing is ITK's discrete Gaussian of physical variance 1 (`spacing` (z, y, x) turns it
    into voxel variances) from `functional.discrete_gaussian_taps`, or explicit `taps` = (taps_z, taps_y, taps_x).  One
    launch smooths and thresholds; `select_candidates` compacts the candidates and sorts only them."""
    if enhanced.dim() != 5 or enhanced.shape[0] != 1:
        raise ValueError(f'expected one volume (1, 1, D, H, W), got {tuple(enhanced.shape)}')
    if taps is None:
        taps = F_hip.discrete_gaussian_taps(1.0, spacing=spacing)
    values, flags = F_hip.smooth_threshold(enhanced, taps, min_threshold)
    return select_candidates(values[0, 0], flags[0, 0], max_kpts)


def select_candidates(values, flags, max_kpts=MAX_KPTS):
    """values (D, H, W), flags (D, H, W) bool, any device -> (K', 3) int64 (z, y, x): the flagged voxels, at most `max_kpts`
    of them, by value descending, ties by linear voxel index ascending.  The volume is compacted once (`torch.nonzero` of the
    flat flags, which lists linear indices in ascending order) and only the candidates are sorted, stably."""
    D, H, W = values.shape
    lin = torch.nonzero(flags.reshape(-1)).squeeze(1)
    order = torch.sort(values.reshape(-1)[lin], descending=True, stable=True).indices[:int(max_kpts)]
    lin = lin[order]
    return torch.stack([lin // (H * W), (lin // W) % H, lin % W], dim=1)


def enhancement_point_cloud(img, mask, fissure_mu, fissure_sigma, spacing=(1, 1, 1), min_threshold=0.2, feature_mode=None):
    """`foerstner_point_cloud` for the reference's 'enhancement' keypoint mode: img, mask (1, 1, D, H, W) on the GPU ->
    (C, K) fp32, rows 0..2 the keypoints of `hessian_enhancement_kpts` on the lung-masked enhanced image in grid
    coordinates (x, y, z), then the features of `feature_mode`: those of FEATURE_MODES, or 'enhancement', the 125 voxels of a
    5^3 patch of the masked, unsmoothed enhanced image, not normalised (point_features.py:182-199)."""
    if feature_mode not in ENHANCEMENT_FEATURE_MODES:
        raise ValueError(f'unknown feature_mode {feature_mode!r}: expected one of {ENHANCEMENT_FEATURE_MODES}')
    enhanced = F_hip.fissure_enhance(img, fissure_mu, fissure_sigma, 1.0, mask=mask)
    kp = hessian_enhancement_kpts(enhanced, min_threshold=min_threshold, spacing=spacing)
    points = keypoints_to_grid(kp, img.shape[2:], spacing)
    if feature_mode is None:
        return points.contiguous()
    if feature_mode == 'enhancement':
        feat = image_patch_features(enhanced, points.transpose(0, 1), patch_size=5)
    elif feature_mode == 'image':
        feat = image_patch_features(img.float(), points.transpose(0, 1), patch_size=5)
        feat = (feat - HU_AIR) / (HU_WATER - HU_AIR) * 2 - 1
    else:
        feat = mind_at_keypoints(img, kp, dilation=1, sigma=0.8, ssc=feature_mode == 'mind_ssc')
    return torch.cat([points, feat], dim=0).contiguous()


def cnn_keypoints_from_softmax(softmax_pred, mask, spacing=(1, 1, 1), feat_patch=5):
    """keypoint_extraction.py:101-118: softmax_pred (1, K, D, H, W), mask (D, H, W) bool -> (kp (N, 3) int64, features
    (feat_patch^3, N)): the voxels inside the mask whose largest score is not the background's, as (z, y, x) indices times the
    spacing (truncated, as the reference stores them), and around each the feat_patch^3 patch of the summed foreground scores"""
    fissure_points = (softmax_pred.argmax(1)[0] != 0) & mask
    sp = torch.tensor(tuple(spacing), dtype=torch.float32, device=softmax_pred.device)
    kp = torch.nonzero(fissure_points) * sp
    if kp.shape[0] == 0:
        return kp.long(), torch.zeros(feat_patch ** 3, 0, dtype=softmax_pred.dtype, device=softmax_pred.device)
    extent = torch.tensor(tuple(fissure_points.shape), device=kp.device) * sp
    kp_grid = kpts_to_grid(kp.flip(-1), extent, align_corners=ALIGN_CORNERS)
    foreground = softmax_pred[:, 1:].sum(1, keepdim=True)
    features = sample_patches_at_kpts(foreground, kp_grid, feat_patch).reshape(kp.shape[0], -1).transpose(0, 1)
    return kp.long(), features


def cnn_point_cloud(models, img, mask, spacing=(1, 1, 1), feat_patch=5):
    """The reference's third keypoint mode, kp_mode='cnn' (`get_cnn_keypoints`, keypoint_extraction.py:87-131), tensors in,
    tensors out: `models` one `MobileNetASPP` in eval mode or a list of them (the fold models), img (1, 1, D, H, W) on the GPU
    at the networks' resolution, mask (1, 1, D, H, W) | (D, H, W) the lung mask, spacing (z, y, x).  Each model's
    `predict_all_patches` gives softmax scores; -> `cnn_keypoints_from_softmax` of them: (kp, features) for one model, two
    lists for several.  File reading, the cross-validation split lookup and the argument files are the caller's."""
    single = isinstance(models, torch.nn.Module)
    models = [models] if single else list(models)
    if not models:
        raise ValueError('cnn_point_cloud: no model given')
    if img.dim() != 5 or img.shape[0] != 1:
        raise ValueError(f'expected one volume (1, 1, D, H, W), got {tuple(img.shape)}')
    mask = mask.reshape(img.shape[2:]).to(device=img.device, dtype=torch.bool)
    kps, feats = [], []
    for model in models:
        with torch.no_grad():
            softmax_pred = model.predict_all_patches(img)
        kp, feat = cnn_keypoints_from_softmax(softmax_pred, mask, spacing, feat_patch)
        kps.append(kp)
        feats.append(feat)
    return (kps, feats) if len(models) > 1 else (kps[0], feats[0])


def keypoints_to_grid(kp, shape, spacing=(1, 1, 1)):
    """voxel indices kp (K, 3) (z, y, x) of a volume with `shape` (D, H, W) and voxel `spacing` (z, y, x) -> (3, K) grid
    coordinates (x, y, z): physical positions over the physical extent, as the reference stores its coordinate features"""
    sp = torch.tensor(spacing, dtype=torch.float32, device=kp.device)
    extent = torch.tensor(tuple(shape), device=kp.device) * sp
    return kpts_to_grid((kp * sp).flip(-1), extent, align_corners=ALIGN_CORNERS).transpose(0, 1)
