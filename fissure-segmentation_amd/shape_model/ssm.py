"""Statistical shape model of DG-SSM (reference: shape_model/ssm.py): PCA of corresponding-point shapes, projection and
decode.  Same constructor arguments, attribute names and state_dict keys (`num_modes`, `percent_of_variance`, `mean_shape`,
`eigenvalues`, `eigenvectors`, registered as None until `fit`) as the reference.  `decode` of a GPU tensor is one launch of
the fused decode kernel (fsg_ssm_decode_fwd_f32, no transform); fitting and projection are plumbing and run in torch
wherever their tensors live.  `LSSM.fit` (the vendored LPCA numpy library) and `save_shape` / `load_shape` stay out."""
import torch
from torch import nn

from .. import functional as F_hip
from ..models.modelio import LoadableModel, store_config_args


class SSM(LoadableModel):
    @store_config_args
    def __init__(self, alpha=2.5, target_variance=0.95, dimensionality=3):
        super().__init__()
        self.target_variance = target_variance
        self.alpha = alpha
        self.dim = dimensionality

        # set by SSM.fit; usable like plain attributes (ssm.py:23-30)
        self.register_parameter('num_modes', None)
        self.register_parameter('percent_of_variance', None)
        self.register_parameter('mean_shape', None)
        self.register_parameter('eigenvalues', None)
        self.register_parameter('eigenvectors', None)

        # the shape model is fixed during training (ssm.py:33)
        self.requires_grad_(False)

    def fit(self, train_shapes: torch.Tensor):
        """ssm.py:35-60.  train_shapes (N, F) data matrix, or (N, P, 3) shapes.  The eigenvectors are kept contiguous
        (same values as the reference's column slice), so that decode reads them without a copy."""
        if len(train_shapes.shape) == 3 and train_shapes.shape[-1] == self.dim:
            train_shapes = shape2vector(train_shapes)

        self.mean_shape = nn.Parameter(train_shapes.mean(0, keepdim=True), requires_grad=False)
        U, S, V = torch.pca_lowrank(train_shapes, q=min(train_shapes.shape), center=True)
        total_variance = S.sum()
        variance_at_sv = (S / total_variance).cumsum(0)

        # number of modes needed to account for the desired portion of the variance
        num_modes = (variance_at_sv <= self.target_variance).sum() + 1

        self.num_modes = nn.Parameter(num_modes, requires_grad=False)
        self.percent_of_variance = nn.Parameter(variance_at_sv[self.num_modes - 1], requires_grad=False)
        self.eigenvalues = nn.Parameter(S[None, :self.num_modes], requires_grad=False)
        self.eigenvectors = nn.Parameter(V[None, :, :self.num_modes].contiguous(), requires_grad=False)
        self.requires_grad_(False)

    def forward(self, shapes):
        """shapes (B, P, 3) -> mode weights (B, M): projection on the eigenvectors (ssm.py:62-72)"""
        self.assert_trained()
        shapes = shape2vector(shapes)
        projection = torch.matmul(self.eigenvectors.transpose(-1, -2), (shapes - self.mean_shape).unsqueeze(-1))
        return projection.squeeze(-1)

    def decode(self, weights):
        """weights (B, M) or (B, M, 1) -> shapes (B, P, 3) (ssm.py:74-83)"""
        self.assert_trained()
        if weights.is_cuda:
            if self.dim != 3:
                raise NotImplementedError("the HIP decode kernel serves three-dimensional shapes only")
            return F_hip.ssm_decode_affine(weights.reshape(*weights.shape[:2]), self.mean_shape, self.eigenvectors)
        weights = weights.view(*weights.shape[:2], 1)
        reconstruction = self.mean_shape + torch.matmul(self.eigenvectors, weights).squeeze(-1)
        return vector2shape(reconstruction, self.dim)

    def random_samples(self, n_samples: int):
        self.assert_trained()
        stddev = torch.sqrt(self.eigenvalues)
        ranges = self.alpha * stddev
        return torch.rand(n_samples, self.num_modes.data, device=stddev.device, dtype=self.eigenvectors.dtype) * 2 * ranges \
            - ranges

    def assert_trained(self):
        if self.eigenvectors is None:
            raise ValueError("SSM is not trained yet. You need to call fit before using it.")

    @classmethod
    def load(cls, path, device):
        checkpoint = torch.load(path, map_location=torch.device(device))
        model = cls(**checkpoint['config'])
        model.register_parameters_from_state_dict(checkpoint['model_state'])
        return model

    def register_parameters_from_state_dict(self, state_dict):
        for key, value in state_dict.items():
            self.register_parameter(key, nn.Parameter(value.contiguous(), requires_grad=False))


class LSSM(SSM):
    """The reference's kernelized localised shape model (ssm.py:112-157).  Fitting needs its vendored LPCA numpy library,
    which is not part of this package; a checkpoint fitted by the reference loads and decodes, since decode is SSM's."""

    def fit(self, train_shapes: torch.Tensor):
        raise NotImplementedError("LSSM.fit needs the reference's vendored LPCA library (shape_model/LPCA), which is outside "
                                  "this package: fit with the reference and load the checkpoint, or use SSM")


def shape2vector(shape: torch.Tensor):
    return shape.flatten(start_dim=-2)


def vector2shape(vector: torch.Tensor, dimensionality=3):
    assert vector.shape[-1] % dimensionality == 0, \
        f"Vector cannot be unflattened. Last dimension needs be multiple of dimensionality ({dimensionality})."
    return vector.unflatten(dim=-1, sizes=(int(vector.shape[-1] / dimensionality), dimensionality))
