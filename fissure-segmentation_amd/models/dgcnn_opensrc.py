"""The upstream DGCNN code path (reference: models/dgcnn_opensrc.py): graph feature, the four-block EdgeConv encoder shared
with the PC-AE encoder, the classification/regression net `DGCNN` (backbone of DG-SSM) and `PointNet`, on the HIP
kernels.  Same constructor arguments, attribute names and state_dict keys as the reference."""
import torch
import torch.nn.functional as F
from torch import nn

from .. import functional as F_hip
from ..norm import BatchNorm1d, BatchNorm2d


def knn(x, k):
    """(B,C,N) -> (B,N,k) int64: the k nearest points INCLUDING the point itself, no forced-zero
    diagonal -- dgcnn_opensrc.py:34-40 ranks by the negated distance with topk(largest)."""
    return F_hip.knn_graph(x, k, fix_diag=False).long()


def get_graph_feature(x, k=20, idx=None):
    """(B,C,N) -> (B,2C,N,k) = cat(x_j - x_i, x_i)   (dgcnn_opensrc.py:43-66)."""
    B, N = x.size(0), x.size(2)
    x = x.reshape(B, -1, N)
    if idx is None:
        idx = F_hip.knn_graph(x, k, fix_diag=False)
    return F_hip.edge_features(x, idx)


def edgeconv_encoder(blocks, x, k, static):
    """The four EdgeConv blocks of the upstream encoder (dgcnn_opensrc.py:137-158, folding_net.py:113-133): blocks are the
    (Conv2d, BatchNorm2d, LeakyReLU) Sequentials conv1..conv4, x (B,C,N) -> point-major concatenation (B*N, sum Co) of
    their outputs, the input of conv5.  static: one graph over the coordinates (channels 0:3) for all four blocks."""
    graph = F_hip.knn_graph(x, k, c_knn=3, fix_diag=False) if static else None
    B, _, N = x.shape
    feats, x_pm = [], None
    for block in blocks:
        conv, bn, act = block
        if F_hip.edgeconv1_supported(conv.out_channels, k):  # fused gather+conv+BN+LeakyReLU+max
            idx = graph if graph is not None else F_hip.knn_graph(x, k, fix_diag=False)
            # the point-major output has two consumers (next block, concatenation): hand the concatenation an alias so
            # that the two gradients reach the backward kernel separately (summed there, the slice taken by stride)
            x, x_pm, x_cat = F_hip.edgeconv1(x, idx, conv.weight, bn, act.negative_slope, x_pm=x_pm, both="twice")
        else:
            x = block(get_graph_feature(x, k=k, idx=graph)).max(dim=-1)[0]
            x_pm = x_cat = x.transpose(1, 2).contiguous()
        feats.append(x_cat)
    return torch.cat(feats, dim=2).view(B * N, -1)


class PointNet(nn.Module):
    """dgcnn_opensrc.py:69-98.  Point-wise Conv1d/BN stacks and a max-pool only: plumbing, it runs wherever its tensors live
    (like PointNetSeg)."""

    def __init__(self, args, output_channels=40):
        super().__init__()
        self.args = args
        self.conv1 = nn.Conv1d(3, 64, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(64, 64, kernel_size=1, bias=False)
        self.conv3 = nn.Conv1d(64, 64, kernel_size=1, bias=False)
        self.conv4 = nn.Conv1d(64, 128, kernel_size=1, bias=False)
        self.conv5 = nn.Conv1d(128, args.emb_dims, kernel_size=1, bias=False)
        self.bn1, self.bn2, self.bn3 = BatchNorm1d(64), BatchNorm1d(64), BatchNorm1d(64)
        self.bn4 = BatchNorm1d(128)
        self.bn5 = BatchNorm1d(args.emb_dims)
        self.linear1 = nn.Linear(args.emb_dims, 512, bias=False)
        self.bn6 = BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=args.dropout)
        self.linear2 = nn.Linear(512, output_channels)

    @F_hip.with_deferred_bn_counters
    def forward(self, x):
        for conv, bn in ((self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3), (self.conv4, self.bn4),
                         (self.conv5, self.bn5)):
            x = F.relu(bn(conv(x)))
        x = F.adaptive_max_pool1d(x, 1).squeeze()
        x = F.relu(self.bn6(self.linear1(x)))
        x = self.dp1(x)
        return self.linear2(x)


def _leaky(slope):
    return nn.LeakyReLU(negative_slope=slope)


class DGCNN(nn.Module):
    """dgcnn_opensrc.py:101-179: the upstream DGCNN classification/regression net, the backbone that DG-SSM's
    MultiHeadDGCNN subclasses (models/dg_ssm.py:31-45).  Encoder: the PC-AE encoder's fused EdgeConv blocks
    (`edgeconv_encoder`) over all `input_channels`; conv5 + BatchNorm + LeakyReLU + [max | mean] pooling in one HIP stage
    (fsg_bn_act_maxavg_*).  The head runs as MODULE calls (linear1, bn6, dp1, ...) that read the modules at call time: the
    subclass hooks linear1 to read the global feature and DGSSM.fit_ssm replaces linear3 after construction."""

    #: clouds per forward of the batched ensembling in `predict_full_pointcloud`
    ensemble_max_clouds = 64

    def __init__(self, args, input_channels, output_channels=40):
        super().__init__()
        self.args = args
        self.k = args.k
        self.bn1, self.bn2, self.bn3, self.bn4 = (BatchNorm2d(c) for c in (64, 64, 128, 256))
        self.bn5 = BatchNorm1d(args.emb_dims)
        self.conv1 = nn.Sequential(nn.Conv2d(input_channels * 2, 64, kernel_size=1, bias=False), self.bn1, _leaky(0.2))
        self.conv2 = nn.Sequential(nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False), self.bn2, _leaky(0.2))
        self.conv3 = nn.Sequential(nn.Conv2d(64 * 2, 128, kernel_size=1, bias=False), self.bn3, _leaky(0.2))
        self.conv4 = nn.Sequential(nn.Conv2d(128 * 2, 256, kernel_size=1, bias=False), self.bn4, _leaky(0.2))
        self.conv5 = nn.Sequential(nn.Conv1d(512, args.emb_dims, kernel_size=1, bias=False), self.bn5, _leaky(0.2))
        self.linear1 = nn.Linear(args.emb_dims * 2, 512, bias=False)
        self.bn6 = BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=args.dropout)
        self.linear2 = nn.Linear(512, 256)
        self.bn7 = BatchNorm1d(256)
        self.dp2 = nn.Dropout(p=args.dropout)
        self.linear3 = nn.Linear(256, output_channels)

    @F_hip.with_deferred_bn_counters
    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("DGCNN (HIP path) needs its input on the GPU")
        B, N = x.shape[0], x.shape[2]
        conv5, bn5, act5 = self.conv5
        y = F_hip.linear_pm(edgeconv_encoder((self.conv1, self.conv2, self.conv3, self.conv4), x, self.k, self.args.static),
                            conv5.weight.view(conv5.out_channels, -1))                       # (B*N, emb_dims)
        if conv5.out_channels % 64 == 0:   # BN + LeakyReLU + [max | mean] over the points, activation never materialised
            x = F_hip.bn_act_maxavg(y.view(B, N, -1), bn5, act5.negative_slope)
        else:
            a = act5(bn5(y)).view(B, N, -1)
            x = torch.cat((a.max(dim=1)[0], a.mean(dim=1)), 1)
        x = F.leaky_relu(self.bn6(self.linear1(x)), negative_slope=0.2)
        x = self.dp1(x)
        x = F.leaky_relu(self.bn7(self.linear2(x)), negative_slope=0.2)
        x = self.dp2(x)
        x = self.linear3(x)
        return x.unsqueeze(-1)

    def _ensemble_batchable(self, pc):
        from .point_seg_net import ensemble_batchable
        return ensemble_batchable(self, pc)

    def predict_full_pointcloud(self, pc, sample_points=1024, n_runs_min=50):
        """dgcnn_opensrc.py:173-179.  When nothing couples the samples of a batch (eval mode, BatchNorm on running statistics,
        dropout off, no grad) the runs -- drawn exactly like the reference's loop draws them -- go through the net as
        batches of runs and are summed in run order; otherwise the sequential loop runs."""
        acc = torch.zeros(pc.shape[0], self.linear3.out_features, 1, device=pc.device)
        if self._ensemble_batchable(pc):
            B, per = pc.shape[0], max(1, self.ensemble_max_clouds // max(pc.shape[0], 1))
            pts = torch.stack([torch.randperm(pc.shape[-1], device=pc.device)[:sample_points] for _ in range(n_runs_min)])
            for r0 in range(0, n_runs_min, per):
                chunk = pts[r0:r0 + per]
                x = pc[:, :, chunk].permute(2, 0, 1, 3).reshape(chunk.shape[0] * B, pc.shape[1], chunk.shape[1])
                for o in self(x).view(chunk.shape[0], B, -1, 1):
                    acc += o
            return acc / n_runs_min
        for _ in range(n_runs_min):
            perm = torch.randperm(pc.shape[-1], device=pc.device)[:sample_points]
            acc += self(pc[..., perm])
        return acc / n_runs_min
