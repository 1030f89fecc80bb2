"""Drop-in for the reference's models/divroc.py: `DiVRoC`, differentiable voxel rasterisation of point clouds.

The reference obtains the splat by differentiating `F.grid_sample(x, coords, align_corners=False)` against a zero grid of the
full output size with `autograd.functional.jacobian` (:36-38), and its backward by a second jacobian over a (B C)-fold repeated
coordinate tensor (:52-57).  That splat is exactly the adjoint of trilinear sampling with zero padding, so here both directions
are the two kernels of csrc/grid_points.hip (functional.splat_to_grid, mode 'torch'): forward = splat, grad of the values =
sample of the grid gradient, grad of the coordinates = the sample kernel's coordinate gradient weighted by the values."""
import torch

from .. import functional as F_hip


class DiVRoC:
    """`DiVRoC.apply(feature_values (B, C, N, 1, 1), coords (B, N, 1, 1, 3), shape (B, C, D, H, W)) -> (B, C, D, H, W)`, the
    reference's call (seg_logits_to_mesh.py:95, dpsr_utils.py:96).  coords are grid_sample's: (x -> W, y -> H, z -> D) in
    [-1, 1]; points outside contribute only through their in-grid corners."""

    @staticmethod
    def apply(feature_values, coords, shape):
        if feature_values.dim() != 5 or tuple(feature_values.shape[3:]) != (1, 1):
            raise ValueError(f"expected feature_values (B, C, N, 1, 1), got {tuple(feature_values.shape)}")
        if coords.dim() != 5 or tuple(coords.shape[2:]) != (1, 1, 3):
            raise ValueError(f"expected coords (B, N, 1, 1, 3), got {tuple(coords.shape)}")
        shape = tuple(int(s) for s in shape)
        B, C, N = feature_values.shape[:3]
        if len(shape) != 5 or shape[:2] != (B, C):
            raise ValueError(f"shape must be (B, C, D, H, W) = ({B}, {C}, ...), got {shape}")
        return F_hip.splat_to_grid(feature_values.reshape(B, C, N), coords.reshape(coords.shape[0], coords.shape[1], 3),
                                   shape[2:], "torch")
