"""DG-SSM (reference: models/dg_ssm.py): the upstream DGCNN with three regression heads on its global feature predicts the
mode weights of a statistical shape model and a similarity transform; the shape is decoded and moved by ONE fused HIP
stage (functional.ssm_decode_affine) that carries the gradient to the weights and to the rotation / translation / scaling
heads.  Same class names, constructor arguments and state_dict keys as the reference."""
from types import SimpleNamespace

import torch
from torch import nn

from .. import functional as F_hip
from ..norm import BatchNorm1d
from ..shape_model.ssm import LSSM, SSM
from ..utils.model_utils import init_weights
from .dgcnn_opensrc import DGCNN
from .modelio import LoadableModel, store_config_args


class RegressionHead(nn.Module):
    """dg_ssm.py:13-28: Linear (no bias) [-> BatchNorm -> Dropout -> LeakyReLU(0.2) -> Linear]*, the last Linear without bias"""

    def __init__(self, in_channels, out_channel_list, dropout=0.):
        super().__init__()
        out_channels = out_channel_list.pop(0)
        self.layers = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False)])
        for i, oc in enumerate(out_channel_list):
            self.layers.extend([BatchNorm1d(out_channels), nn.Dropout(p=dropout), nn.LeakyReLU(negative_slope=0.2),
                                nn.Linear(out_channels, oc, bias=not i == len(out_channel_list) - 1)])
            out_channels = oc

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


def create_in_feature_hook(feature_dict, name):
    def input_hook(model, input, output):
        feature_dict[name] = input
    return input_hook


class MultiHeadDGCNN(DGCNN):
    """dg_ssm.py:31-82: the heads read the input of linear1 (the pooled global feature) through a forward hook.  They run as
    module calls, so further hooks, `head_active` and a replaced linear3 keep working."""

    def __init__(self, dgcnn_args, input_channels, output_channels_main, other_heads_out):
        super().__init__(dgcnn_args, input_channels, output_channels_main)
        self.heads = nn.ModuleDict()
        self.head_active = {'main': True}
        for name, channels in other_heads_out.items():
            self.heads[name] = RegressionHead(dgcnn_args.emb_dims * 2, channels, dgcnn_args.dropout)
            self.head_active[name] = True

        self.feat = {}
        # create_in_feature_hook(self.feat, 'global_feature') as a bound method, so that a deepcopy of the net fills its own dict
        self.linear1.register_forward_hook(self._global_feature_hook)

    def _global_feature_hook(self, module, input, output):
        self.feat['global_feature'] = input

    def forward(self, x):
        main_head_out = super().forward(x)
        global_feature = self.feat['global_feature'][0]
        other_heads_out = {}
        with F_hip.deferred_bn_counters(), F_hip.no_autocast():
            for name, head in self.heads.items():
                if self.head_active[name]:
                    other_heads_out[name] = head(global_feature)
                else:   # an inactive head predicts the identity: zeros, ones for the scaling
                    fill = torch.ones if name == "scaling" else torch.zeros
                    other_heads_out[name] = fill(x.shape[0], head.layers[-1].out_features, device=x.device,
                                                 dtype=main_head_out.dtype)
        if not self.head_active['main']:
            main_head_out = torch.zeros_like(main_head_out)
        return main_head_out, other_heads_out

    def set_head_active(self, name, active=True):
        self.head_active[name] = active

    def predict_full_pointcloud(self, pc, sample_points=1024, n_runs_min=50):
        """dg_ssm.py:66-82.  Where nothing couples the samples of a batch (`ensemble_batchable`: eval mode, no grad) the runs --
        drawn by the same torch.randperm calls in the same order -- go through the net in chunks of `ensemble_max_clouds`
        and are summed in run order, for the main head and every other head; otherwise the sequential loop runs."""
        B = pc.shape[0]
        acc = torch.zeros(B, self.linear3.out_features, 1, device=pc.device)
        accs = {name: torch.zeros(B, head.layers[-1].out_features, device=pc.device) for name, head in self.heads.items()}
        if self._ensemble_batchable(pc):
            per = max(1, self.ensemble_max_clouds // max(B, 1))
            pts = torch.stack([torch.randperm(pc.shape[-1], device=pc.device)[:sample_points] for _ in range(n_runs_min)])
            for r0 in range(0, n_runs_min, per):
                chunk = pts[r0:r0 + per]
                runs = chunk.shape[0]
                x = pc[:, :, chunk].permute(2, 0, 1, 3).reshape(runs * B, pc.shape[1], chunk.shape[1])
                coeff, transforms = self(x)
                for o in coeff.view(runs, B, -1, 1):
                    acc += o
                for name in self.heads.keys():
                    for o in transforms[name].view(runs, B, -1):
                        accs[name] += o
        else:
            for _ in range(n_runs_min):
                perm = torch.randperm(pc.shape[-1], device=pc.device)[:sample_points]
                coeff, transforms = self(pc[..., perm])
                acc += coeff
                for name in self.heads.keys():
                    accs[name] += transforms[name]
        return acc / n_runs_min, {name: val / n_runs_min for name, val in accs.items()}


class DGSSM(LoadableModel):
    @store_config_args
    def __init__(self, k, in_features, spatial_transformer=False, dynamic=True, image_feat_module=False,
                 predict_affine_params=True, ssm_alpha=3., ssm_targ_var=0.95, ssm_modes=1, lssm=False, only_affine=False):
        super().__init__()
        if spatial_transformer:
            raise NotImplementedError()
        if image_feat_module:
            raise NotImplementedError()

        self.predict_affine_params = predict_affine_params or only_affine
        self.only_affine = only_affine
        self.ssm = (LSSM if lssm else SSM)(ssm_alpha, ssm_targ_var)
        dgcnn_args = SimpleNamespace(k=k, emb_dims=1024, dropout=0., static=not dynamic)
        self.dgcnn = MultiHeadDGCNN(dgcnn_args, input_channels=in_features, output_channels_main=ssm_modes,
                                    other_heads_out={'translation': [512, 50, 3], 'rotation': [512, 50, 3],
                                                     'scaling': [512, 50, 3]})

    def forward(self, x):
        """x (B, in_features, N) -> (reconstructions (B, P, 3), pred_weights (B, M), cat(rotation, translation, scaling)
        (B, 9)).  The coefficients multiply the eigenvalues (dg_ssm.py:128); only their trailing dimension is squeezed, so a
        batch or a shape model of ONE works (the reference's bare squeeze() drops that dimension too and then fails in decode).
        Without affine parameters the reference returns the decoded shapes transposed, (B, 3, P) (dg_ssm.py:138); kept."""
        self.ssm.assert_trained()

        x = self.dgcnn(x)
        coefficients, so3_rotation, translation, scaling = self.split_prediction(x)
        if not self.only_affine:
            pred_weights = coefficients.squeeze(-1) * self.ssm.eigenvalues
        else:
            pred_weights = torch.zeros_like(coefficients)
        weights = pred_weights.reshape(*pred_weights.shape[:2])
        if not self.predict_affine_params:   # the identity transform: decode alone
            reconstructions = F_hip.ssm_decode_affine(weights, self.ssm.mean_shape, self.ssm.eigenvectors).transpose(1, 2)
        else:
            reconstructions = F_hip.ssm_decode_affine(weights, self.ssm.mean_shape, self.ssm.eigenvectors,
                                                      so3_rotation, scaling, translation)
        return reconstructions, pred_weights, torch.cat((so3_rotation, translation, scaling), dim=1)

    def fit_ssm(self, shapes):
        self.ssm.fit(shapes)
        self.config['ssm_modes'] = self.ssm.num_modes.data.item()

        # the main head regresses one coefficient per mode of the fitted model
        self.dgcnn.linear3 = nn.Linear(256, self.config['ssm_modes'])
        self.dgcnn.apply(init_weights)

    def split_prediction(self, dgcnn_pred):
        main, others = dgcnn_pred
        if self.predict_affine_params:
            return main, others['rotation'], others['translation'], others['scaling']
        bs = main.shape[0]
        return main, main.new_zeros(bs, 3), main.new_zeros(bs, 3), main.new_ones(bs, 3)

    @classmethod
    def load(cls, path, device):
        checkpoint = torch.load(path, map_location=torch.device(device))
        model = cls(**checkpoint['config'])
        model.load_state_dict(checkpoint['model_state'], strict=False)
        ssm_state = {key.replace("ssm.", ""): value for key, value in checkpoint['model_state'].items() if "ssm." in key}
        model.ssm.register_parameters_from_state_dict(ssm_state)
        return model

    def set_head_active(self, name, active=True):
        self.dgcnn.set_head_active(name, active)
