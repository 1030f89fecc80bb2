"""Image features at keypoints with the reference's names (data_processing/point_features.py:86-199): MIND / MIND-SSC
descriptors on the GPU (csrc/volume.hip) and image patches (plain torch)."""
import torch

from .. import functional as F_hip
from ..utils.general_utils import sample_patches_at_kpts

SIX_NEIGHBOURHOOD = ((0, 1, 1), (1, 1, 0), (1, 0, 1), (1, 1, 2), (2, 1, 1), (1, 2, 1))   # point_features.py:102-107
SSC_ORDER = (6, 8, 1, 11, 2, 10, 0, 7, 9, 4, 5, 3)   # point_features.py:148: output channel j is pair SSC_ORDER[j]


def mind_shift_tables(ssc=True):
    """-> (shifts, outch, box), derived from the six-neighbourhood as the reference derives its convolution kernels
    (point_features.py:109-132).
    ssc: shifts[c] = ((dz, dy, dx), (dz, dy, dx)), the two voxels whose squared difference is channel c as offsets in
    {-1, 0, 1} -- the pairs (i, j), i > j, of neighbours at squared distance 2, in row-major order of (i, j); outch[c] is
    where channel c goes in the output (SSC_ORDER); box False.
    not ssc: box True and shifts[c] = (first, second), two 27-bit subsets of the 3 x 3 x 3 stencil (bit (kz * 3 + ky) * 3 +
    kx) whose SUMS are compared.  They are the reference's kernels as it builds them: the first is all ones, and the second
    is filled by indexing a (6, 3, 3, 3) tensor with the three coordinate columns, which addresses (channel, z, y) and sets
    whole rows along x -- channels 3..5 stay empty.  Reproduced as it is, because features computed with it exist."""
    six = torch.tensor(SIX_NEIGHBOURHOOD)
    if ssc:
        dist = (six[:, None, :] - six[None, :, :]).pow(2).sum(-1)
        x, y = torch.meshgrid(torch.arange(6), torch.arange(6), indexing="ij")
        mask = (x > y).view(-1) & (dist == 2).view(-1)
        first = six.unsqueeze(1).repeat(1, 6, 1).view(-1, 3)[mask]
        second = six.unsqueeze(0).repeat(6, 1, 1).view(-1, 3)[mask]
        outch = [0] * len(SSC_ORDER)
        for j, c in enumerate(SSC_ORDER):
            outch[c] = j
        shifts = [(tuple(int(v) - 1 for v in a), tuple(int(v) - 1 for v in b)) for a, b in zip(first.tolist(), second.tolist())]
        return shifts, outch, False
    mshift1 = torch.ones(6, 3, 3, 3)
    mshift2 = torch.zeros(6, 3, 3, 3)
    mshift2[six[:, 0], six[:, 1], six[:, 2]] = 1
    bits = 2 ** torch.arange(27, dtype=torch.long)
    shifts = [(int((mshift1[c].flatten().long() * bits).sum()), int((mshift2[c].flatten().long() * bits).sum())) for c in range(6)]
    return shifts, list(range(6)), True


def mind(img: torch.Tensor, dilation: int = 1, sigma: float = 0.8, ssc: bool = True):
    """point_features.py:86-150: (B, 1, D, H, W) -> (B, 12 | 6, D, H, W), the reference's channel order.  Two passes over
    the image: one for the global mean of the clamp, one that writes the features."""
    shifts, outch, box = mind_shift_tables(ssc)
    return F_hip.mind_volume(img, dilation, sigma, shifts, outch, box)


def mind_at_keypoints(img, kp, dilation=1, sigma=0.8, ssc=True):
    """`mind(img, ...)[0][:, kp[:, 0], kp[:, 1], kp[:, 2]]`, bitwise, without writing the feature volume: img (1, 1, D, H, W),
    kp (K, 3) int64 voxel indices (z, y, x) -> (12 | 6, K)"""
    shifts, outch, box = mind_shift_tables(ssc)
    return F_hip.mind_keypoints(img, kp, dilation, sigma, shifts, outch, box)


def image_patch_features(img, kp_grid, patch_size=5):
    """the 'image' / 'enhancement' branch of point_features.py:196-199: img (1, 1, D, H, W), kp_grid (K, 3) grid coordinates
    (x, y, z) -> (patch_size ** 3, K)"""
    patches = sample_patches_at_kpts(img, kp_grid, patch_size)
    return patches[0].flatten(start_dim=1).transpose(0, 1)
