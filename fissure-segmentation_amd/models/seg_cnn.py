"""The 3-D voxel segmentation CNN of the reference (models/seg_cnn.py): `MobileNetASPP` = MobileNet3D backbone, ASPP at quarter
resolution, a three-convolution head at half resolution, x2 trilinear up-sampling; and its patch-based inference
`predict_all_patches`.  Constructor arguments, `config` and the 200 state_dict keys are the reference's, so its checkpoints load
through `LoadableModel.load`.

Eval mode: the backbone runs through the fused block kernel (`functional.mbconv3d`, one launch per block), ASPP and head through
torch's `conv3d` with their BatchNorms folded, one item at a time -- torch picks a convolution algorithm by shape, so this keeps an
item's result independent of how many items travel with it.  The folded weights are computed on the first eval call and kept until
`train()`, `load_state_dict()` or a move of the module (writing into a parameter in place while in eval mode is not noticed).
Training mode: the plain torch composition of the same graph with batch-statistics BatchNorm and dropout; gradients come from
autograd.  The reference's activation checkpointing and its prints are not mirrored."""
import math

import torch
from torch import nn
from torch.nn import functional as F

from .. import functional as F_hip
from .aspp_3d import ASPP, fold_conv_bn
from .mobilenet import MobileNet3D
from .modelio import LoadableModel, store_config_args


def get_patch_starts(img_size, min_overlap, patch_size):
    """per axis the corners of the fewest equally spaced patches that cover the axis with at least `min_overlap` (a fraction of
    the patch) between neighbours; [0] where the patch is not shorter than the axis (the patch is padded later)"""
    starts = []
    for dim, patch in zip(img_size, list(patch_size)):
        if patch >= dim:
            starts.append([0])
            continue
        stride = patch - patch * min_overlap
        steps = math.ceil((dim - patch * min_overlap) / stride)
        overlap = (steps * patch - dim) / (steps - 1)
        starts.append([math.floor(s * (patch - overlap) + 0.5) for s in range(steps)])
    return starts


def get_necessary_padding(img_dimensions, out_shape):
    """the argument of `F.pad` (last axis first, (front, back) per axis) that grows img_dimensions to out_shape, the larger half
    of an odd difference in front; None when nothing is missing"""
    pad = []
    for have, want in zip(reversed(tuple(img_dimensions)), reversed(tuple(out_shape))):
        missing = max(want - have, 0)
        pad += [missing - missing // 2, missing // 2]
    return pad if any(pad) else None


def maybe_pad_img_patch(img, patch_shape):
    pad = get_necessary_padding(img.shape[2:], patch_shape)
    return img if pad is None else F.pad(img, pad, mode='replicate')


def maybe_crop_after_padding(img, orig_dimensions):
    """undo `maybe_pad_img_patch`: the part of img (B, C, ...) that held the original extents"""
    pad = get_necessary_padding(orig_dimensions, img.shape[2:])
    if pad is None:
        return img
    nd = img.dim() - 2
    index = [slice(None), slice(None)]
    for axis in range(nd):
        front, back = pad[2 * (nd - 1 - axis)], pad[2 * (nd - 1 - axis) + 1]
        index.append(slice(front, img.shape[2 + axis] - back))
    return img[tuple(index)]


def gaussian_weight_map(patch_size, sigma_scale=1 / 4.):
    """What the reference builds with scipy.ndimage.gaussian_filter(impulse at p // 2, sigma = p * sigma_scale per axis,
    mode='constant'), zeros replaced by the smallest non-zero value: the outer product of the three truncated (4 sigma),
    normalised 1-D kernels shifted to the centre.  fp64, on the CPU, shape `patch_size`."""
    axes = []
    for p in patch_size:
        sigma = p * sigma_scale
        radius = int(4.0 * sigma + 0.5)
        offs = torch.arange(-radius, radius + 1, dtype=torch.float64)
        kernel = torch.exp(-0.5 / (sigma * sigma) * offs ** 2)
        kernel = kernel / kernel.sum()
        line = torch.zeros(p, dtype=torch.float64)
        idx = torch.arange(p) - p // 2 + radius           # the kernel tap that lands on each cell
        ok = (idx >= 0) & (idx <= 2 * radius)
        line[ok] = kernel[idx[ok]]
        axes.append(line)
    wmap = axes[0]
    for line in axes[1:]:
        wmap = wmap.unsqueeze(-1) * line
    if bool((wmap == 0).any()):
        wmap[wmap == 0] = wmap[wmap != 0].min()
    return wmap


class MobileNetASPP(LoadableModel):
    @store_config_args
    def __init__(self, num_classes, patch_size=(128, 128, 128)):
        super().__init__()
        self.num_classes = num_classes
        self.backbone = MobileNet3D()
        self.aspp = ASPP(64, (2, 4, 8, 16), 128)
        self.head = nn.Sequential(nn.Conv3d(128 + 16, 64, 1, bias=False), nn.BatchNorm3d(64), nn.ReLU(),
                                  nn.Conv3d(64, 64, 3, padding=1, bias=False), nn.BatchNorm3d(64), nn.ReLU(),
                                  nn.Conv3d(64, num_classes, 1))
        self.patch_size = patch_size
        self._folded = None
        self._weight_map = None

    # ------------------------------------------------------------------ the folded eval-mode weights
    def train(self, mode=True):
        self._folded = None
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self._folded = None
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._folded = self._weight_map = None
        return super()._apply(fn, *args, **kwargs)

    def folded(self):
        if self._folded is None:
            with torch.no_grad():
                head = [fold_conv_bn(self.head[0], self.head[1]), fold_conv_bn(self.head[3], self.head[4]),
                        (self.head[6].weight.detach().float().contiguous(), self.head[6].bias.detach().float().contiguous())]
                self._folded = dict(backbone=self.backbone.fold(), aspp=self.aspp.fold(), head=head)
        return self._folded

    # ------------------------------------------------------------------ forward
    def _check_input(self, x):
        if x.dim() != 5 or x.shape[1] != 1:
            raise ValueError(f"MobileNetASPP: expected (B, 1, D, H, W), got {tuple(x.shape)}")
        if any(n % 4 for n in x.shape[2:]):
            raise ValueError(f"MobileNetASPP.forward: every spatial extent must be a multiple of 4, got {tuple(x.shape[2:])} "
                             f"(predict_all_patches pads any volume)")
        if not x.is_cuda:
            raise RuntimeError("fissure_segmentation_amd runs on the GPU only (got a CPU tensor); the CPU restatement of the "
                               "voxel CNN is tests/seg_cnn_oracle.py")

    def half_res_logits(self, x, folded=None):
        """eval mode: x (B, 1, D, H, W) -> the head's output (B, num_classes, D/2, H/2, W/2), before the final up-sampling"""
        fd = self.folded() if folded is None else folded
        with torch.no_grad():
            x1, x2 = self.backbone.forward_fused(x.float(), fd["backbone"])
            out = []
            for i in range(x.shape[0]):          # item by item: see the module docstring
                y = self.aspp.forward_folded(x2[i:i + 1], fd["aspp"])
                y = torch.cat([x1[i:i + 1], F.interpolate(y, scale_factor=2)], dim=1)
                y = F.relu(F.conv3d(y, *fd["head"][0]))
                y = F.relu(F.conv3d(y, *fd["head"][1], padding=1))
                out.append(F.conv3d(y, *fd["head"][2]).contiguous())
            return torch.cat(out, dim=0)

    def forward(self, x):
        self._check_input(x)
        if self.training:
            x1, x2 = self.backbone(x)
            y = torch.cat([x1, F.interpolate(self.aspp(x2), scale_factor=2)], dim=1)
            y = self.head(y)
        else:
            y = self.half_res_logits(x)
        return F.interpolate(y, scale_factor=2, mode='trilinear', align_corners=False)

    # ------------------------------------------------------------------ patch-based inference
    def gaussian_map(self, device):
        """the importance map of a patch, fp32 on `device` (built once per patch size and device)"""
        wm = self._weight_map
        if wm is None or tuple(wm.shape) != tuple(self.patch_size) or wm.device != torch.device(device):
            self._weight_map = wm = gaussian_weight_map(self.patch_size).to(device=device, dtype=torch.float32)
        return wm

    def predict_all_patches(self, img, min_overlap=0.5, use_gaussian=True, patch_batch=4):
        """img (B, 1, D, H, W) on the GPU, any extents -> softmax scores (B, num_classes, D, H, W): the volume is covered by
        patches of `patch_size` with at least `min_overlap` between neighbours (an axis shorter than the patch is
        replicate-padded), each patch's softmax is weighted (Gaussian importance map, or 1) and added up, and the normalised sum
        goes through the softmax a second time, as in the reference.  `patch_batch` patches travel through the network
        together; the result does not depend on it.  Eval mode only: the kernels under it are inference kernels."""
        if self.training:
            raise RuntimeError("predict_all_patches runs the fused inference kernels: call eval() first")
        patch = tuple(int(p) for p in self.patch_size)
        if img.dim() != 5 or img.shape[1] != 1 or len(patch) != 3:
            raise ValueError(f"predict_all_patches: expected (B, 1, D, H, W) and a 3-D patch size, got {tuple(img.shape)}, {patch}")
        if any(p % 4 for p in patch):
            raise ValueError(f"predict_all_patches: every patch extent must be a multiple of 4, got {patch}")
        if not 0 <= min_overlap < 1:
            raise ValueError("predict_all_patches: min_overlap must lie in [0, 1)")
        if int(patch_batch) < 1:
            raise ValueError("predict_all_patches: patch_batch must be >= 1")
        if not img.is_cuda:
            raise RuntimeError("fissure_segmentation_amd runs on the GPU only (got a CPU tensor)")
        B = img.shape[0]
        starts = get_patch_starts(img.shape[2:], min_overlap, patch)
        entries = [(b, z, y, x) for z in starts[0] for y in starts[1] for x in starts[2] for b in range(B)]
        folded = self.folded()
        wmap = self.gaussian_map(img.device) if use_gaussian else None
        img = img.float()
        out_sum = torch.zeros(B, self.num_classes, *img.shape[2:], dtype=torch.float32, device=img.device)
        out_weight = torch.zeros(B, 1, *img.shape[2:], dtype=torch.float32, device=img.device)
        for first in range(0, len(entries), int(patch_batch)):
            group = entries[first:first + int(patch_batch)]
            patches = torch.cat([maybe_pad_img_patch(img[b:b + 1, :, z:z + patch[0], y:y + patch[1], x:x + patch[2]], patch)
                                 for b, z, y, x in group], dim=0)
            logits = self.half_res_logits(patches, folded)
            F_hip.patch_accumulate(logits, group, patch, out_sum, out_weight, wmap)
        return F_hip.patch_finalize(out_sum, out_weight)
