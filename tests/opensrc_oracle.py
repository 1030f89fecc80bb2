"""CPU torch oracle of the upstream DGCNN (reference: models/dgcnn_opensrc.py:101-171), built from the blocks of
oracle.ref_cpu.ClsEncoder (the PC-AE encoder restatement, same four EdgeConv blocks and conv5), the graph builders
ref_cpu.knn_opensrc / ref_cpu.edge_features (looked up at call time, so GraphTape can replay the HIP graphs), max + mean
pooling and the head.  Module and state_dict names follow the reference.  Pinned by tests/test_dgcnn_opensrc_cpu.py
against the open_* fixtures of the real reference before the GPU tests use it at full size."""
import torch
from torch import nn

from oracle import ref_cpu


class OpenDGCNN(nn.Module):
    def __init__(self, args, input_channels, output_channels=40):
        super().__init__()
        self.args, self.k = args, args.k
        enc = ref_cpu.ClsEncoder(args.k, args.emb_dims)
        if input_channels != 3:
            enc.conv1[0] = nn.Conv2d(input_channels * 2, 64, 1, bias=False)
        for i in range(1, 6):          # registration order of the reference: bn1..bn5, then conv1..conv5 (which hold them again)
            setattr(self, f"bn{i}", getattr(enc, f"bn{i}"))
        for i in range(1, 6):
            setattr(self, f"conv{i}", getattr(enc, f"conv{i}"))
        self.linear1 = nn.Linear(args.emb_dims * 2, 512, bias=False)
        self.bn6 = nn.BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=args.dropout)
        self.linear2 = nn.Linear(512, 256)
        self.bn7 = nn.BatchNorm1d(256)
        self.dp2 = nn.Dropout(p=args.dropout)
        self.linear3 = nn.Linear(256, output_channels)
        self.act6, self.act7 = nn.LeakyReLU(0.2), nn.LeakyReLU(0.2)   # modules, so that FlipOracle sees the head's kinks

    def forward(self, x):
        graph = ref_cpu.knn_opensrc(x[:, :3], self.k) if self.args.static else None
        feats = []
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4):
            idx = graph if graph is not None else ref_cpu.knn_opensrc(x, self.k)
            x = conv(ref_cpu.edge_features(x, idx)).max(dim=-1)[0]
            feats.append(x)
        a = self.conv5(torch.cat(feats, dim=1))
        x = torch.cat((a.max(dim=-1)[0], a.mean(dim=-1)), 1)
        x = self.dp1(self.act6(self.bn6(self.linear1(x))))
        x = self.dp2(self.act7(self.bn7(self.linear2(x))))
        return self.linear3(x).unsqueeze(-1)
