"""DSEG-AE glue (csrc/dseg_ae.hip): label partition, jittered segment extension, FPS from a given start."""
import torch

from .. import _lib
from .._launch import _f32c, _need_gpu, _p, _stream, launch
from .packed import knn_segment
from .spatial import _LABEL_KINDS


# ------------------------------------------------------------------ DSEG-AE glue (csrc/dseg_ae.hip)
PARTITION_MAX_LABELS = _lib.PARTITION_MAX_LABELS


def label_partition(labels, x, num_labels, first_label=1):
    """labels (B, N) uint8 / int32 / int64, x (B, C, N) with the coordinates in its first three channels -> the points of the
    objects first_label .. first_label + num_labels - 1 as packed segments, one per (item, object) in that order:
    counts (B, num_labels) int32, offset (B * num_labels) int32 (the end of every segment), xyz (B * N, 3) fp32 and
    src (B * N) int32 (the point's index inside its item), of which the first offset[-1] rows are filled and the rest are
    zero.  Inside a segment the points keep their order.  Any other label is dropped.  Nothing is read on the host."""
    if labels.dim() != 2 or x.dim() != 3 or x.shape[0] != labels.shape[0] or x.shape[2] != labels.shape[1] or x.shape[1] < 3:
        raise ValueError(f"label_partition: labels (B, N) and x (B, C >= 3, N) expected, got {tuple(labels.shape)} and {tuple(x.shape)}")
    if labels.dtype not in _LABEL_KINDS:
        raise TypeError(f"label_partition: labels must be uint8, int32 or int64, got {labels.dtype}")
    L = int(num_labels)
    if not 1 <= L <= PARTITION_MAX_LABELS:
        raise ValueError(f"label_partition: num_labels must be in 1..{PARTITION_MAX_LABELS}, got {num_labels}")
    B, N = labels.shape
    if B == 0 or N == 0 or B * N >= 2 ** 31:
        raise ValueError(f"label_partition: {B} clouds of {N} points (1 <= B * N < 2^31)")
    _need_gpu(labels, x)
    labels, x = labels.contiguous(), _f32c(x)
    dev = x.device
    counts = torch.empty(B, L, dtype=torch.int32, device=dev)
    offset = torch.empty(B * L, dtype=torch.int32, device=dev)
    xyz = torch.zeros(B * N, 3, dtype=torch.float32, device=dev)
    src = torch.zeros(B * N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _lib.workspace("fsg_label_partition", B, N, L, device=dev)
        _lib.call("fsg_label_partition", _p(labels), _LABEL_KINDS[labels.dtype], _p(x), B, x.shape[1], N, int(first_label), L,
                  _p(counts), _p(offset), _p(xyz), _p(src), _p(ws), ws.numel(), _stream())
    return counts, offset, xyz, src


def segment_jitter_extend(xyz, offset, target, src_idx, direction, z, nn_d2=None):
    """`random_extend_points` of dseg_ae_regularization.py for G packed segments in one launch.  xyz (n, 3) with offset (G)
    HOST-known segment ends (a list, or a tensor that is read on the host); every segment grows to max(its length, target) --
    target a number or one per segment.  The caller's draws cover the P padded rows, packed in segment order: src_idx (P)
    the source row inside the segment, direction (P, 3), z (P).  nn_d2 (n): squared distance to the nearest OTHER point of
    the segment; by default column 1 of `knn_segment(2, xyz, xyz, offset, offset)`.
    -> out (n_new, 3), new_offset (G) int32 on the device, stats (G, 2) = mean and unbiased std of the nearest distances
    (0, 0 for fewer than two points).  A padded row is xyz[src] + direction / |direction| * (z * std + mean)."""
    _need_gpu(xyz, src_idx, direction, z, nn_d2)
    ends = [int(v) for v in (offset.tolist() if torch.is_tensor(offset) else offset)]
    G = len(ends)
    lens = [e - s for s, e in zip([0] + ends[:-1], ends)]
    tg = [int(v) for v in (target.tolist() if torch.is_tensor(target) else target)] if hasattr(target, "__len__") else [int(target)] * G
    if xyz.dim() != 2 or xyz.shape[1] != 3 or G == 0 or len(tg) != G or min(lens) < 0 or ends[-1] != xyz.shape[0] or xyz.shape[0] == 0:
        raise ValueError(f"segment_jitter_extend: xyz {tuple(xyz.shape)} with segment ends {ends} and {len(tg)} targets")
    new_lens = [max(n, t) for n, t in zip(lens, tg)]
    n, n_new = ends[-1], sum(new_lens)
    P = n_new - n
    if src_idx.numel() != P or tuple(direction.shape) != (P, 3) or z.numel() != P:
        raise ValueError(f"segment_jitter_extend: {P} padded rows, draws of {src_idx.numel()}, {tuple(direction.shape)}, {z.numel()}")
    dev = xyz.device
    xyz = _f32c(xyz)
    off = torch.tensor(ends, dtype=torch.int32).to(dev)
    new_off = torch.tensor(new_lens, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
    if nn_d2 is None:
        nn_d2 = knn_segment(2, xyz, xyz, off, off)[1][:, 1]
    if nn_d2.shape != (n,):
        raise ValueError(f"segment_jitter_extend: nn_d2 {tuple(nn_d2.shape)} for {n} points")
    nn_d2 = _f32c(nn_d2)
    src_idx, direction, z = src_idx.to(torch.int32).contiguous(), _f32c(direction), _f32c(z).reshape(-1)
    out = torch.empty(n_new, 3, dtype=torch.float32, device=dev)
    stats = torch.empty(G, 2, dtype=torch.float32, device=dev)
    launch(dev, "fsg_segment_jitter_extend_f32", _p(xyz), _p(off), _p(nn_d2), _p(new_off), _p(src_idx), _p(direction), _p(z), G, n,
           n_new, _p(out), _p(stats))
    return out, new_off, stats


def fps_start(xyz, offset, new_offset, m, start=None):
    """`fps` with a first sample per segment: start (b) = its index INSIDE the segment (None: 0, and then the result equals
    `fps`'s bit for bit).  One workgroup of 1024 threads per segment; segments of up to 16 384 points are sampled from
    registers.  m = total number of samples (new_offset[-1], known on the host) -> idx (m) int32 into xyz."""
    _need_gpu(xyz, offset, new_offset, start)
    xyz = _f32c(xyz)
    offset, new_offset = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    if start is not None:
        if start.shape != offset.shape:
            raise ValueError(f"fps_start: start {tuple(start.shape)} for {offset.shape[0]} segments")
        start = start.to(torch.int32).contiguous()
    n = xyz.shape[0]
    idx = torch.empty(m, dtype=torch.int32, device=xyz.device)     # every entry is written (empty segments: zeros, by the kernel)
    tmp = torch.empty(n, dtype=torch.float32, device=xyz.device)
    launch(xyz.device, "fsg_fps_start_f32", _p(xyz), _p(offset), _p(new_offset), _p(start), offset.shape[0], n, _p(tmp), _p(idx))
    return idx
