"""Foerstner keypoints with the reference's names (data_processing/foerstner.py:7-108).  `distinctiveness` is one fused
launch and `foerstner_kpts` two launches plus `torch.nonzero` on the device; the structure-tensor helpers are kept as plain
torch for callers that want the intermediate tensors (nothing on the hot path does)."""
import torch

from .. import functional as F_hip
from ..utils.image_utils import smooth


def structure_tensor(img, sigma):
    """(B, C, D, H, W) -> (B, C (C + 1) / 2, D, H, W): the smoothed products of channel pairs (p, q), p <= q, row-major"""
    C = img.shape[1]
    pairs = [(p, q) for p in range(C) for q in range(p, C)]
    return torch.cat([smooth((img[:, p] * img[:, q])[:, None], sigma) for p, q in pairs], dim=1)


def invert_structure_tensor_only_trace(struct):
    """struct (B, 6, D, H, W) holds the symmetric 3 x 3 tensor [[s0, s1, s2], [s1, s3, s4], [s2, s4, s5]] per voxel ->
    (B, 3, D, H, W), the diagonal of its inverse: diagonal cofactors over the determinant, the determinant expanded along
    the first row, the reciprocal of the determinant taken first (the operation order fsg_foerstner_dist_f32 follows)"""
    s0, s1, s2, s3, s4, s5 = struct.unbind(1)
    cof00 = s3 * s5 - s4 * s4
    cof01 = - s1 * s5 + s2 * s4
    cof02 = s1 * s4 - s2 * s3
    cof11 = s0 * s5 - s2 * s2
    cof22 = s0 * s3 - s1 * s1
    det = s0 * cof00 + s1 * cof01 + s2 * cof02
    return (1. / det)[:, None] * torch.stack([cof00, cof11, cof22], dim=1)


def distinctiveness(img, sigma):
    """foerstner.py:62-73: (B, 1, D, H, W) -> (B, 1, D, H, W) on the GPU (fsg_foerstner_dist_f32)"""
    return F_hip.foerstner_distinctiveness(img, sigma)


def foerstner_kpts(img, mask, sigma=1.4, d=9, thresh=1e-8):
    """foerstner.py:76-108: img, mask (1, 1, D, H, W) -> (K, 3) int64 voxel indices (z, y, x) in torch.nonzero's order.
    Two properties of the reference are kept: the erosion of the mask looks at the six face neighbours only (never at the
    voxel itself), and a NaN distinctiveness (constant regions) suppresses every keypoint whose window contains it."""
    dist = F_hip.foerstner_distinctiveness(img, sigma)
    flags = F_hip.nms_keypoint_flags(dist, mask, d, thresh)
    return torch.nonzero(flags)[:, 2:]
