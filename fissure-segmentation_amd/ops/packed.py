"""Packed clouds (pointops.py): kNN and farthest point sampling over the segments of one (n, 3) tensor."""
import torch

from .._launch import _f32c, _need_gpu, _p, launch


# ------------------------------------------------------------------ packed clouds (pointops.py)
def knn_segment(nsample, xyz, new_xyz, offset, new_offset):
    """-> idx (m,nsample) int32, dist2 (m,nsample) squared distances."""
    _need_gpu(xyz, new_xyz, offset, new_offset)
    xyz, new_xyz = _f32c(xyz), _f32c(new_xyz)
    offset, new_offset = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    m = new_xyz.shape[0]
    idx = torch.empty(m, nsample, dtype=torch.int32, device=xyz.device)
    d2 = torch.empty(m, nsample, dtype=torch.float32, device=xyz.device)
    launch(xyz.device, "fsg_knn_segment_f32", _p(xyz), _p(new_xyz), _p(offset), _p(new_offset), offset.shape[0],
           xyz.shape[0], m, nsample, _p(idx), _p(d2))
    return idx, d2


def fps(xyz, offset, new_offset, m):
    """m = total number of samples (new_offset[-1], known on the host) -> idx (m) int32."""
    _need_gpu(xyz, offset, new_offset)
    xyz = _f32c(xyz)
    offset, new_offset = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    n = xyz.shape[0]
    idx = torch.empty(m, dtype=torch.int32, device=xyz.device)     # every entry is written (empty segments: zeros, by the kernel)
    tmp = torch.empty(n, dtype=torch.float32, device=xyz.device)
    launch(xyz.device, "fsg_fps_f32", _p(xyz), _p(offset), _p(new_offset), offset.shape[0], n, _p(tmp), _p(idx))
    return idx
