"""Atrous spatial pyramid pooling in 3-D, the middle of the voxel CNN (reference: models/aspp_3d.py), written from the
architecture with the reference's state_dict keys: branch 0 a 1x1x1 convolution, one dilated 3x3x3 convolution per rate, a
global-average-pooling branch broadcast back over the volume; each followed by BatchNorm and ReLU; the concatenation is
projected by a 1x1x1 convolution, BatchNorm, ReLU and Dropout(0.5).  `forward` is the torch composition (training: batch
statistics, dropout); `forward_folded` is the eval form on torch's `conv3d` with every BatchNorm folded into its convolution."""
import torch
from torch import nn
from torch.nn import functional as F

from .mobilenet import fold_bn


def conv_bn_relu(cin, cout, kernel, dilation=1):
    return [nn.Conv3d(cin, cout, kernel, padding=dilation * (kernel // 2), dilation=dilation, bias=False), nn.BatchNorm3d(cout), nn.ReLU()]


def fold_conv_bn(conv, bn):
    """(weight, bias) of the convolution that equals conv followed by the eval-mode bn"""
    scale, shift = fold_bn(bn)
    w = conv.weight.detach().float() * scale.view(-1, 1, 1, 1, 1)
    if conv.bias is not None:
        shift = shift + conv.bias.detach().float() * scale
    return w.contiguous(), shift


class ASPPConv(nn.Sequential):
    def __init__(self, in_channels, out_channels, dilation):
        super().__init__(*conv_bn_relu(in_channels, out_channels, 3, dilation))


class ASPPPooling(nn.Sequential):
    def __init__(self, in_channels, out_channels):
        super().__init__(*conv_bn_relu(in_channels, out_channels, 1))

    def forward(self, x):
        y = x.mean(dim=(2, 3, 4), keepdim=True)
        for layer in self:
            y = layer(y)
        return y.expand(-1, -1, *x.shape[2:])


class ASPP(nn.Module):
    def __init__(self, in_channels, atrous_rates, out_channels=256):
        super().__init__()
        self.rates = tuple(atrous_rates)
        branches = [nn.Sequential(*conv_bn_relu(in_channels, out_channels, 1))]
        branches += [ASPPConv(in_channels, out_channels, r) for r in self.rates]
        branches.append(ASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(branches)
        self.project = nn.Sequential(*conv_bn_relu(len(branches) * out_channels, out_channels, 1), nn.Dropout(0.5))

    def forward(self, x):
        return self.project(torch.cat([branch(x) for branch in self.convs], dim=1))

    def fold(self):
        return [fold_conv_bn(b[0], b[1]) for b in self.convs] + [fold_conv_bn(self.project[0], self.project[1])]

    def forward_folded(self, x, folded):
        """eval mode (no dropout): x (B, C, D, H, W) on the device, `folded` from fold()"""
        res = [F.relu(F.conv3d(x, *folded[0]))]
        for rate, (w, b) in zip(self.rates, folded[1:-2]):
            res.append(F.relu(F.conv3d(x, w, b, padding=rate, dilation=rate)))
        pooled = F.relu(F.conv3d(x.mean(dim=(2, 3, 4), keepdim=True), *folded[-2]))
        res.append(pooled.expand(-1, -1, *x.shape[2:]))
        return F.relu(F.conv3d(torch.cat(res, dim=1), *folded[-1]))
