"""Voxel CNN inference (csrc/seg_cnn.hip)."""
import ctypes

import torch

from .. import _lib
from .._launch import _f32c, _need_gpu, _p, launch


# ------------------------------------------------------------------ voxel CNN inference (csrc/seg_cnn.hip)
MBCONV_MAX_CIN, MBCONV_MAX_CMID, MBCONV_MAX_COUT = _lib.MBCONV_MAX_CIN, _lib.MBCONV_MAX_CMID, _lib.MBCONV_MAX_COUT


def _ndhwc(x):
    """(B, C, D, H, W) -> the (B, D, H, W, C) buffer behind it, without a copy when x is in channels-last memory"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def mbconv3d(x, w1, s1, b1, wd, s2, b2, w3, s3, b3, stride=1, residual=False, first=False):
    """One eval-mode inverted-residual block of models/mobilenet.py in one launch (fsg_mbconv3d_fwd_f32); inference only, no
    autograd.  x (B, Cin, D, H, W) fp32 on the GPU, read in `torch.channels_last_3d` memory (any other layout is copied into it)
    -> (B, Cout, Do, Ho, Wo) in the same memory format.  w1 (Cmid, Cin[, 1, 1, 1]), or with `first` the dense 3x3x3 stride-2
    padding-1 kernel (Cmid, 1, 3, 3, 3); wd (Cmid, 1, 3, 3, 3) the depthwise kernel of `stride` 1 | 2; w3 (Cout, Cmid[, 1, 1, 1]);
    (s, b) the three folded BatchNorms, ReLU6 after the first two; `residual` adds x.  Cin, Cout <= 64, Cmid a multiple of 16,
    <= 384."""
    if x.dim() != 5:
        raise ValueError(f"mbconv3d: x must be (B, Cin, D, H, W), got {tuple(x.shape)}")
    B, Cin, D, H, W = x.shape
    Cmid, Cout = wd.shape[0], w3.shape[0]
    if not (1 <= Cin <= MBCONV_MAX_CIN and 1 <= Cout <= MBCONV_MAX_COUT and 16 <= Cmid <= MBCONV_MAX_CMID and Cmid % 16 == 0):
        raise ValueError(f"mbconv3d: channels {Cin} -> {Cmid} -> {Cout} outside the kernel's limits (Cin, Cout <= 64; Cmid a "
                         f"multiple of 16, <= 384)")
    if stride not in (1, 2):
        raise ValueError(f"mbconv3d: stride must be 1 or 2, got {stride}")
    if first and Cin != 1:
        raise ValueError(f"mbconv3d: the dense first layer takes one input channel, got {Cin}")
    if residual and (first or stride != 1 or Cin != Cout):
        raise ValueError("mbconv3d: the residual add needs stride 1, Cin == Cout and the 1x1x1 expand stage")
    k1 = 27 if first else Cin
    if w1.numel() != Cmid * k1 or wd.numel() != Cmid * 27 or w3.numel() != Cout * Cmid:
        raise ValueError(f"mbconv3d: weights {tuple(w1.shape)}, {tuple(wd.shape)}, {tuple(w3.shape)} do not fit "
                         f"{Cin} -> {Cmid} -> {Cout}")
    for t, n in ((s1, Cmid), (b1, Cmid), (s2, Cmid), (b2, Cmid), (s3, Cout), (b3, Cout)):
        if t.numel() != n:
            raise ValueError("mbconv3d: a scale / shift vector does not have one entry per channel")
    _need_gpu(x, w1, s1, b1, wd, s2, b2, w3, s3, b3)
    dm = [(n - 1) // 2 + 1 for n in (D, H, W)] if first else [D, H, W]
    do = [(n - 1) // stride + 1 for n in dm]
    xc = _ndhwc(x.detach().to(torch.float32))
    y = torch.empty((B, *do, Cout), dtype=torch.float32, device=x.device)
    w1, wd, w3, s1, b1, s2, b2, s3, b3 = (_f32c(t) for t in (w1, wd, w3, s1, b1, s2, b2, s3, b3))
    launch(x.device, "fsg_mbconv3d_fwd_f32", _p(xc), _p(w1), _p(s1), _p(b1), _p(wd), _p(s2), _p(b2), _p(w3), _p(s3), _p(b3), B, Cin,
           Cmid, Cout, D, H, W, int(stride), int(bool(first)), int(bool(residual)), _p(y))
    return y.permute(0, 4, 1, 2, 3)


def patch_accumulate(logits, starts, patch_size, out_sum, out_weight, weight_map=None):
    """The tail of the reference's patch loop (models/seg_cnn.py:48-59) for P patches (fsg_patch_accumulate_f32): logits
    (P, K, pd/2, ph/2, pw/2) the head's half-resolution output, starts a list of P (item, z, y, x), patch_size (pd, ph, pw),
    weight_map (pd, ph, pw) | None (weight 1).  x2 trilinear up-sampling, softmax over K, times the weight, cropped to the
    volume and added IN PLACE into out_sum (B, K, D, H, W) and out_weight (B, 1, D, H, W), patch after patch in the order given."""
    pd, ph, pw = (int(p) for p in patch_size)
    if logits.dim() != 5 or tuple(logits.shape[2:]) != (pd // 2, ph // 2, pw // 2) or pd % 2 or ph % 2 or pw % 2:
        raise ValueError(f"patch_accumulate: logits {tuple(logits.shape)} are not the half-resolution output of patches {patch_size}")
    P, K = logits.shape[:2]
    B, K2, D, H, W = out_sum.shape
    if K2 != K or tuple(out_weight.shape) != (B, 1, D, H, W) or len(starts) != P:
        raise ValueError("patch_accumulate: out_sum (B, K, D, H, W), out_weight (B, 1, D, H, W) and one start per patch expected")
    for t in (out_sum, out_weight):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("patch_accumulate: out_sum and out_weight must be contiguous fp32 (they are updated in place)")
    if weight_map is not None and tuple(weight_map.shape[-3:]) != (pd, ph, pw):
        raise ValueError(f"patch_accumulate: weight_map {tuple(weight_map.shape)} does not cover a patch {patch_size}")
    _need_gpu(logits, out_sum, out_weight, weight_map)
    host = (ctypes.c_int * (4 * P))(*[int(v) for s in starts for v in s])
    lg = _f32c(logits)
    wm = _f32c(weight_map) if weight_map is not None else None
    launch(logits.device, "fsg_patch_accumulate_f32", _p(lg), P, K, pd, ph, pw, host, _p(wm), _p(out_sum), _p(out_weight), B, D, H, W)


def patch_finalize(out_sum, out_weight):
    """softmax over K of out_sum / out_weight (models/seg_cnn.py:61-62; fsg_patch_finalize_f32) -> a new (B, K, D, H, W) tensor"""
    _need_gpu(out_sum, out_weight)
    B, K, D, H, W = out_sum.shape
    if tuple(out_weight.shape) != (B, 1, D, H, W):
        raise ValueError("patch_finalize: out_weight must be (B, 1, D, H, W)")
    s, w = _f32c(out_sum), _f32c(out_weight)
    out = torch.empty_like(s)
    launch(s.device, "fsg_patch_finalize_f32", _p(s), _p(w), B, K, D, H, W, _p(out))
    return out
