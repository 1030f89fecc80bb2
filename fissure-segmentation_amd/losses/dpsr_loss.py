"""DPSRLoss (reference: losses/dpsr_loss.py:9-44): the nnU-Net point segmentation loss plus the Chamfer distance between surface
samples of the predicted and the target meshes, on `NNULoss` (csrc/seg_loss.hip) and `RegularizedMeshLossHIP(w_chamfer=1, others
0)` (csrc/mesh.hip sampler + csrc/chamfer.hip).  Predictions are what `DPSRNet2.forward` returns: (seg_logits,
fissure_segmentation_amd.mesh.Meshes).  An opt-in class like RegularizedMeshLossHIP: the loss registry does not name it."""
import torch
from torch import nn

from .mesh_loss import RegularizedMeshLossHIP
from .nnu_loss import NNULoss


class DPSRLoss(nn.Module):
    """Same constructor and `(loss, {'Segmentation': ..., 'Chamfer': ...})` as the reference.  The mesh term joins once
    `current_epoch_fraction >= epoch_start_mesh_loss`, the numbers of predicted and target meshes agree and w_mesh > 0;
    before that the loss is the segmentation loss alone and 'Chamfer' is a zero tensor."""
    DEFAULT_W_SEG = 0.5
    DEFAULT_W_CHAMFER = 0.5
    DEFAULT_EPOCH_START_CHAMFER = 0.1

    def __init__(self, class_weights, w_seg=DEFAULT_W_SEG, w_mesh=DEFAULT_W_CHAMFER, epoch_start_mesh_loss=DEFAULT_EPOCH_START_CHAMFER):
        super().__init__()
        self.w_seg = w_seg
        self.w_mesh = w_mesh
        self.epoch_start_mesh = epoch_start_mesh_loss
        self.seg_loss = NNULoss(class_weights)
        self.chamfer_loss = RegularizedMeshLossHIP(w_chamfer=1, w_laplacian=0, w_edge_length=0, w_normal_consistency=0)

    def forward(self, prediction, target, current_epoch_fraction=None):
        pred_seg, pred_meshes = prediction
        targ_seg, targ_meshes = target
        seg_loss, _ = self.seg_loss(pred_seg, targ_seg)
        if (current_epoch_fraction >= self.epoch_start_mesh
                and len(pred_meshes) == len(targ_meshes)
                and self.w_mesh > 0):
            cham_loss, _ = self.chamfer_loss(pred_meshes, targ_meshes)
            loss = self.w_seg * seg_loss + self.w_mesh * cham_loss
        else:   # only the segmentation loss at first
            cham_loss = torch.tensor(0)
            loss = seg_loss
        return loss, {'Segmentation': seg_loss, 'Chamfer': cham_loss}
