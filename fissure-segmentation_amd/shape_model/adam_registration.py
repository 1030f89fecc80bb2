"""Dense deformable registration of two CT volumes by Adam instance optimisation -- the tensor-level part of the reference's
shape_model/adam_registration.py.  MIND-SSC and one-hot label features of the moving image are sampled on a half-resolution
displacement grid; the cost is their squared difference to the fixed features, with a diffusion regulariser and a triple box
("B-spline") smoothing of the parameter; 50 Adam steps; the fitted field is carried to full resolution to move keypoints and
warp the image and the labels.

One iteration of :106-124 is four launches here and no host read: functional.reg_smooth3 of the parameter, the fused
objective (sampling, cost, regulariser and the gradient with respect to the field in one gather, csrc/dense_reg.hip), the same
smoothing of that gradient (the operator is its own adjoint), and the flat Adam update of csrc/adam.hip.  The buffers belong to
an `InstanceOptimisation`, nothing is allocated inside the loop, and the loop can be captured into one hipGraph on one stream.

The reference's quirks are kept:
* the parameter starts at the identity (or affine) GRID COORDINATES, not at zero (:97-102) -- numbers in [-1, 1] that the
  loop then reads as a displacement;
* `fitted_grid` is the smoothed field of the last EVALUATED iterate, i.e. of the parameter before the last Adam step (:126);
* the displacement is scaled by (S - 1) / 2 beside align_corners=False (:115-117, :132).
Not reproduced: reading files (SimpleITK), the TRE print-out and the plots.  One deliberate difference: the labels that
`adam_registration` warps are the MOVING ones, pulled onto the fixed grid like the image (the reference's :164 pulls the fixed
fissures through the same fixed-grid field, which moves them away from the moving ones)."""
import collections

import torch
from torch.nn import functional as F

from .. import _lib
from .. import functional as F_hip
from ..data_processing.point_features import mind

GRID_SP = 2


def _combined_labels(lobes, fissures):
    """:82-83: fissure labels are stacked behind the lobe labels"""
    return lobes + torch.where(fissures != 0, fissures + lobes.max(), fissures)


def registration_features(img, mask, lobes, fissures, num_labels=None):
    """:37-46, :81-91.  img, mask, lobes, fissures (B, 1, H, W, D) on the GPU, the image in HU -> (features packed by
    functional.reg_pack_features (B, H/2, W/2, D/2, Cp) fp16, C): the one-hot combined lobe + fissure labels, nearest-resized to
    the half-resolution grid, then the masked MIND-SSC descriptors of the image + 1000 (our HIP `mind`), average-pooled by
    GRID_SP.  num_labels: the one-hot width (default: the largest label + 1, as F.one_hot infers it -- a pair of volumes
    must agree on it)."""
    for t, name in ((img, "img"), (mask, "mask"), (lobes, "lobes"), (fissures, "fissures")):
        if not torch.is_tensor(t) or t.dim() != 5 or t.shape[1] != 1 or t.shape != img.shape:
            raise ValueError(f"expected {name} (B, 1, H, W, D) like img, got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if min(img.shape[2:]) < 3 * GRID_SP:
        raise ValueError(f"every image axis must be >= {3 * GRID_SP} (a grid axis of 3 at GRID_SP = {GRID_SP}), got "
                         f"{tuple(img.shape[2:])}")
    F_hip._need_gpu(img, mask, lobes, fissures)
    H, W, D = img.shape[2:]
    with torch.no_grad():
        mind_ = mask.float() * mind(img.float() + 1000, ssc=True)      # important that scans are in HU
        mind_ = F.avg_pool3d(mind_, GRID_SP, stride=GRID_SP)
        labels = _combined_labels(lobes, fissures).long()
        labels = F.one_hot(labels, -1 if num_labels is None else int(num_labels)).transpose(-1, 1).squeeze(-1).float()
        labels = F.interpolate(labels, size=(H // GRID_SP, W // GRID_SP, D // GRID_SP), mode='nearest')
        feat = torch.cat([labels.half(), mind_.half()], dim=1)
        return F_hip.reg_pack_features(feat), feat.shape[1]


class InstanceOptimisation:
    """The state of one run of :93-124 for a batch of B pairs: the parameter (B, 3, Hg, Wg, Dg), its smoothed field, the two
    gradients, Adam's moments and step, the loss history.  `iterate(first, count)` launches iterations first .. first + count - 1
    on the current stream (4 entry-point launches each) and returns nothing; it reads nothing back and allocates nothing, so
    it may run under torch.cuda.graph."""

    def __init__(self, feat_fix, feat_mov, channels=None, affine_pre_reg=None, iters=50, lambda_weight=.65, lr=1., cost_scale=12.):
        if not torch.is_tensor(feat_fix) or feat_fix.dim() != 5:
            raise ValueError("feat_fix must be packed features (B, Hg, Wg, Dg, Cp) (functional.reg_pack_features)")
        B, Hg, Wg, Dg = feat_fix.shape[:4]
        if int(iters) < 1:
            raise ValueError(f"iters must be >= 1, got {iters}")
        dev = feat_fix.device
        theta = torch.eye(3, 4).unsqueeze(0) if affine_pre_reg is None else torch.as_tensor(affine_pre_reg, dtype=torch.float32)
        if theta.dim() == 2:
            theta = theta.unsqueeze(0)
        if tuple(theta.shape[1:]) != (3, 4) or theta.shape[0] not in (1, B):
            raise ValueError(f"affine_pre_reg must be (3, 4) or ({B}, 3, 4), got {tuple(theta.shape)}")
        if min(Hg, Wg, Dg) < 3:
            raise ValueError(f"every grid axis must be >= 3, got {(Hg, Wg, Dg)}")
        self.channels = F_hip._reg_features_check(B, (Hg, Wg, Dg), dev, feat_fix, feat_mov, channels)
        F_hip._need_gpu(feat_fix, feat_mov)
        grid0 = F.affine_grid(theta.to(dev).float().expand(B, 3, 4), (B, 1, Hg, Wg, Dg), align_corners=False)
        self.param = grid0.permute(0, 4, 1, 2, 3).float().contiguous()      # grid COORDINATES as the start (:97-102)
        self.feat_fix, self.feat_mov = feat_fix.contiguous(), feat_mov.contiguous()
        self.disp, self.grad, self.param_grad = (torch.empty_like(self.param) for _ in range(3))
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.param), torch.zeros_like(self.param)
        self.state = torch.zeros(2, dtype=torch.float32, device=dev)         # { step, ticket } of fsg_adam_flat_f32
        self.history = torch.zeros(int(iters), B, 2, dtype=torch.float32, device=dev)
        self.ws = _lib.workspace("fsg_reg_objective", B, Hg, Wg, Dg, device=dev)
        self.iters, self.lambda_weight, self.lr, self.cost_scale = int(iters), float(lambda_weight), float(lr), float(cost_scale)

    def iterate(self, first=0, count=None):
        count = self.iters - first if count is None else count
        if first < 0 or count < 0 or first + count > self.iters:
            raise ValueError(f"iterations {first} .. {first + count - 1} do not fit the history of {self.iters}")
        B, _, Hg, Wg, Dg = self.param.shape
        P = F_hip._p
        with torch.cuda.device(self.param.device):
            for it in range(first, first + count):
                s = F_hip._stream()
                _lib.call("fsg_reg_smooth3_f32", P(self.param), B, 3, Hg, Wg, Dg, P(self.disp), s)
                F_hip._reg_objective_raw(self.disp, self.feat_fix, self.feat_mov, self.channels, self.lambda_weight, self.cost_scale,
                                         self.grad, self.history[it], self.ws)
                _lib.call("fsg_reg_smooth3_f32", P(self.grad), B, 3, Hg, Wg, Dg, P(self.param_grad), s)   # self-adjoint
                _lib.call("fsg_adam_flat_f32", P(self.param), P(self.param_grad), P(self.exp_avg), P(self.exp_avg_sq),
                          P(self.state), self.param.numel(), self.lr, None, 0.9, 0.999, 1e-8, 0.0, s)

    @property
    def fitted_grid(self):
        """the smoothed field of the last evaluated iterate (:126)"""
        return self.disp


def adam_instance_optimisation(feat_fix, feat_mov, affine_pre_reg=None, iters=50, lambda_weight=.65, lr=1., channels=None):
    """:93-126.  feat_fix, feat_mov: packed features (B, Hg, Wg, Dg, Cp) fp16 with `channels` real channels (default Cp);
    affine_pre_reg (3, 4) or (B, 3, 4) or None (identity) -> (fitted_grid (B, 3, Hg, Wg, Dg) fp32, channel c along axis c in
    grid voxels * (S - 1) / S as the reference scales it; loss history (iters, B, 2) fp32 = { cost, reg } of every evaluated
    iterate, on the device).  No host synchronisation inside."""
    run = InstanceOptimisation(feat_fix, feat_mov, channels, affine_pre_reg, iters, lambda_weight, lr)
    run.iterate()
    return run.fitted_grid, run.history


def displacement_field(fitted_grid, shape):
    """:127-132.  fitted_grid (B, 3, Hg, Wg, Dg) -> (B, 3, H, W, D), shape = (H, W, D): times GRID_SP, trilinear upsample
    (align_corners=False), three box passes (functional.reg_smooth3), then divided by (S - 1) / 2 and flipped, so that channel
    0 is grid_sample's x (along D)."""
    try:
        shape = tuple(int(s) for s in shape)
    except TypeError:
        shape = ()
    if len(shape) != 3 or min(shape) < 3:
        raise ValueError(f"shape must be three sizes (H, W, D), each >= 3, got {shape}")
    F_hip._reg_field(fitted_grid, "fitted_grid", 3)
    F_hip._need_gpu(fitted_grid)
    with torch.no_grad():
        disp_hr = F.interpolate(fitted_grid.float() * GRID_SP, size=shape, mode='trilinear', align_corners=False)
        disp_smooth = F_hip.reg_smooth3(disp_hr)
        scale = torch.tensor([s - 1 for s in shape], dtype=torch.float32, device=fitted_grid.device).view(1, 3, 1, 1, 1)
        return torch.flip(disp_smooth / scale * 2, [1])


Registration = collections.namedtuple("Registration", "disp keypts_fix keypts_moved warped warped_labels fitted_grid history")


def adam_registration(img_fix, img_mov, mask_fix, mask_mov, fissures_fix, fissures_mov, lobes_fix, lobes_mov, affine_pre_reg=None,
                      n_keypoints=2048, generator=None):
    """:64-168 on tensors.  Every volume (1, 1, H, W, D) on the GPU, images in HU -> Registration:
    disp (1, 3, H, W, D) the field in grid_sample's normalised (x, y, z) units, defined on the fixed grid;
    keypts_fix (K, 3) random points inside the fixed mask (K <= n_keypoints, normalised (x, y, z)), keypts_moved = keypts_fix +
    the field read there (functional.sample_grid, 'torch' mode);
    warped: the moving image pulled onto the fixed grid (trilinear; outside the moving volume it reads -1000 HU);
    warped_labels: the combined lobe + fissure labels of the moving side pulled the same way (nearest), int64;
    fitted_grid and the loss history of adam_instance_optimisation."""
    dev = img_fix.device
    H, W, D = img_fix.shape[2:]
    with torch.no_grad():
        num = int(max(_combined_labels(lobes_fix, fissures_fix).max(), _combined_labels(lobes_mov, fissures_mov).max())) + 1
        feat_fix, C = registration_features(img_fix, mask_fix, lobes_fix, fissures_fix, num)
        feat_mov, _ = registration_features(img_mov, mask_mov, lobes_mov, fissures_mov, num)

        # random keypoints inside the fixed mask (:72-76)
        keypts_rand = 2 * torch.rand(int(n_keypoints) * 24, 3, device=dev, generator=generator) - 1
        val = F_hip.sample_grid(mask_fix.float(), keypts_rand.view(1, -1, 3), 'torch')
        idx = torch.nonzero(val.reshape(-1) == 1).reshape(-1)
        keypts_fix = keypts_rand[idx[:int(n_keypoints)]]

        fitted_grid, history = adam_instance_optimisation(feat_fix, feat_mov, affine_pre_reg, channels=C)
        disp = displacement_field(fitted_grid, (H, W, D))
        if keypts_fix.shape[0]:
            pred = F_hip.sample_grid(disp, keypts_fix.view(1, -1, 3), 'torch')[0].t()
        else:
            pred = keypts_fix.new_zeros(0, 3)
        grid = disp.permute(0, 2, 3, 4, 1) + F.affine_grid(torch.eye(3, 4, device=dev).unsqueeze(0), (1, 1, H, W, D),
                                                           align_corners=False)
        warped = F.grid_sample(img_mov.float() + 1000, grid, align_corners=False) - 1000
        labels_mov = _combined_labels(lobes_mov, fissures_mov).float()
        warped_labels = F.grid_sample(labels_mov, grid, mode='nearest', align_corners=False).long()
    return Registration(disp, keypts_fix, keypts_fix + pred, warped, warped_labels, fitted_grid, history)
