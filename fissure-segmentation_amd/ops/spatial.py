"""Voxel patch augmentation and resampling (csrc/spatial.hip)."""
import torch

from .. import _lib
from .._launch import _f32c, _need_gpu, _p, _stream, launch


# ------------------------------------------------------------------ voxel patch augmentation, resampling (csrc/spatial.hip)
BSPLINE_PAD = _lib.BSPLINE_PAD      # edge-replicated samples the prefilter adds on every side (scipy's own for mode='nearest')
ELASTIC_MAX_SIGMA = _lib.ELASTIC_MAX_SIGMA
_LABEL_KINDS = {torch.uint8: _lib.LABEL_U8, torch.int32: _lib.LABEL_I32, torch.int64: _lib.LABEL_I64}


def _volume5(t, what, floating=True):
    if t.dim() != 5 or t.numel() == 0 or (floating and not t.is_floating_point()):
        raise ValueError(f"{what}: expected a{' floating-point' if floating else 'n'} (B, C, D, H, W) tensor, got "
                         f"{tuple(t.shape)} {t.dtype}")
    if (t.shape[2] + 2 * BSPLINE_PAD) * (t.shape[3] + 2 * BSPLINE_PAD) * (t.shape[4] + 2 * BSPLINE_PAD) >= 2 ** 31:
        raise ValueError(f"{what}: volume {tuple(t.shape[2:])} holds 2^31 voxels or more with its padding")
    if t.shape[0] > 65535:
        raise ValueError(f"{what}: batch of {t.shape[0]} (at most 65535)")


def bspline_prefilter(vol):
    """vol (B, C, D, H, W) floating point -> the cubic B-spline coefficients (B, C, D + 24, H + 24, W + 24) fp32 of the volume
    extended by BSPLINE_PAD = 12 edge-replicated samples on every side: what scipy.ndimage.map_coordinates(order=3,
    mode='nearest') computes before it interpolates.  Three axis passes (csrc/spatial.hip).  Feed it to `spatial_transform(...,
    order_data=3, prefiltered=True)`; a data set keeps it across epochs."""
    _volume5(vol, "bspline_prefilter")
    _need_gpu(vol)
    x = _f32c(vol)
    B, C, D, H, W = x.shape
    p = 2 * BSPLINE_PAD
    dev = x.device
    with torch.no_grad(), torch.cuda.device(dev):
        a = torch.empty(B, C, D, H, W + p, dtype=torch.float32, device=dev)
        _lib.call("fsg_bspline_prefilter_axis_f32", _p(x), B * C * D * H, W, 1, _p(a), _stream())
        b = torch.empty(B, C, D, H + p, W + p, dtype=torch.float32, device=dev)
        _lib.call("fsg_bspline_prefilter_axis_f32", _p(a), B * C * D, H, W + p, _p(b), _stream())
        del a
        out = torch.empty(B, C, D + p, H + p, W + p, dtype=torch.float32, device=dev)
        _lib.call("fsg_bspline_prefilter_axis_f32", _p(b), B * C, D, (H + p) * (W + p), _p(out), _stream())
    return out


def _per_item(v, B, dev, what, lo=None, hi=None):
    """a number or a (B,) tensor -> (B,) fp32 on the device; a number is range-checked here, a tensor is not read"""
    if torch.is_tensor(v):
        if v.shape != (B,):
            raise ValueError(f"{what} must be a number or a tensor of shape ({B},), got {tuple(v.shape)}")
        _need_gpu(v)
        return _f32c(v)
    v = float(v)
    if (lo is not None and not v > lo) or (hi is not None and not v <= hi):
        raise ValueError(f"{what} = {v} must lie in ({lo}, {hi}]")
    return torch.full((B,), v, dtype=torch.float32, device=dev)


def elastic_field(noise, sigma, alpha):
    """noise (B, 3, pd, ph, pw) -> alpha * scipy.ndimage.gaussian_filter(noise, sigma, mode='constant', cval=0, truncate=4)
    per item and component, fp32: batchgenerators' elastic displacement field (`elastic_deform_coordinates`).  sigma, alpha: a
    number or a (B,) device tensor (never read on the host).  scipy's taps, radius int(4 sigma + 0.5), which may exceed an
    axis; one launch per axis for all items and components.  sigma must lie in (0, 255]; an item of a sigma TENSOR that does
    not gives NaN."""
    if noise.dim() != 5 or noise.shape[1] != 3 or noise.numel() == 0 or not noise.is_floating_point():
        raise ValueError(f"elastic_field: expected floating-point noise (B, 3, pd, ph, pw), got {tuple(noise.shape)} {noise.dtype}")
    B, _, pd, ph, pw = noise.shape
    if 3 * pd * ph * pw >= 2 ** 31 or B > 65535:
        raise ValueError(f"elastic_field: field {tuple(noise.shape)}: 2^31 values or more per item, or more than 65535 items")
    dev = noise.device
    sg = _per_item(sigma, B, dev, "elastic_field: sigma", 0.0, ELASTIC_MAX_SIGMA)
    al = _per_item(alpha, B, dev, "elastic_field: alpha")
    _need_gpu(noise)
    x = _f32c(noise)
    with torch.no_grad(), torch.cuda.device(dev):
        out, tmp = torch.empty_like(x), torch.empty_like(x)
        _lib.call("fsg_gauss_axis_f32", _p(x), B, 3 * pd * ph, pw, 1, _p(sg), None, _p(out), _stream())
        _lib.call("fsg_gauss_axis_f32", _p(out), B, 3 * pd, ph, pw, _p(sg), None, _p(tmp), _stream())
        _lib.call("fsg_gauss_axis_f32", _p(tmp), B, 3, pd, ph * pw, _p(sg), _p(al), _p(out), _stream())
    return out


def _patch3(patch_size, what):
    try:
        p = tuple(int(v) for v in patch_size)
    except TypeError:
        p = ()
    if len(p) != 3 or min(p) < 1 or p[0] * p[1] * p[2] >= 2 ** 31:
        raise ValueError(f"{what}: patch_size must be three positive integers (pd, ph, pw) with fewer than 2^31 voxels, got "
                         f"{patch_size!r}")
    return p


def spatial_transform(img, seg, patch_size, matrix, centre, elastic=None, mirror=None, order_data=3, order_seg=0,
                      prefiltered=False, intensity=None):
    """One fused launch (csrc/spatial.hip) that cuts a transformed patch out of an image and its label map: for output voxel o
    of item b the source coordinate is  matrix_b @ ((o - (patch_size - 1) / 2) + elastic_b(o)) + centre_b,  in voxel units, axes
    (D, H, W) -> (img_patch (B, C, *patch_size) fp32, seg_patch (B, Cs, *patch_size) int64); either input may be None (its
    output is then None).

    img (B, C, D, H, W) floating point, read at order_data 3 (cubic B-spline; the coefficients come from `bspline_prefilter`,
      or are `img` itself, (B, C, D + 24, H + 24, W + 24), with prefiltered=True), 1 (trilinear) or 0 (nearest).  Borders:
      edge replication -- orders 0 and 1 clamp the coordinate to [0, n - 1]; order 3 evaluates the spline in the 12 padded
      samples and runs into the edge coefficient beyond them, as scipy's map_coordinates(mode='nearest') does.
    seg (B, Cs, D, H, W) integer (values must fit an int32): order_seg 0 = nearest (floor(x + 0.5)), 1 = batchgenerators'
      per-label rule (the largest label whose summed trilinear weight is >= 0.5, else 0).  A coordinate outside [0, n - 1] on
      any axis gives 0 (scipy's mode='constant', cval=0).
    matrix (B, 3, 3), centre (B, 3), elastic (B, 3, *patch_size) or None, mirror (B, 3) bool or None (a set flag reverses the
      item's OUTPUT along that axis, after everything else), intensity (a, b) or None: img_patch = a * value + b.
    No host read, no atomics: bit-reproducible, batch-independent, capturable in a graph."""
    what = "spatial_transform"
    pd, ph, pw = _patch3(patch_size, what)
    if img is None and seg is None:
        raise ValueError(f"{what}: neither an image nor a label map")
    if order_data not in (0, 1, 3) or order_seg not in (0, 1):
        raise ValueError(f"{what}: order_data must be 0, 1 or 3 and order_seg 0 or 1, got {order_data!r}, {order_seg!r}")
    if prefiltered and (order_data != 3 or img is None):
        raise ValueError(f"{what}: prefiltered=True goes with an image and order_data=3")
    pad = BSPLINE_PAD if prefiltered else 0
    shape = None
    if img is not None:
        _volume5(img, f"{what}: img")
        if min(img.shape[2:]) <= 2 * pad:
            raise ValueError(f"{what}: prefiltered coefficients {tuple(img.shape)} are smaller than their padding")
        shape = (img.shape[0],) + tuple(s - 2 * pad for s in img.shape[2:])
    if seg is not None:
        _volume5(seg, f"{what}: seg", floating=False)
        if seg.is_floating_point() or seg.is_complex() or seg.dtype == torch.bool:
            raise ValueError(f"{what}: seg must be an integer tensor, got {seg.dtype}")
        sshape = (seg.shape[0],) + tuple(seg.shape[2:])
        if shape is not None and sshape != shape:
            raise ValueError(f"{what}: img {tuple(img.shape)} (padding {pad}) and seg {tuple(seg.shape)} do not match")
        shape = sshape
    B, D, H, W = shape
    if not torch.is_tensor(matrix) or not torch.is_tensor(centre) or matrix.shape != (B, 3, 3) or centre.shape != (B, 3):
        raise ValueError(f"{what}: matrix must be a ({B}, 3, 3) tensor and centre ({B}, 3)")
    if elastic is not None and elastic.shape != (B, 3, pd, ph, pw):
        raise ValueError(f"{what}: elastic must be ({B}, 3, {pd}, {ph}, {pw}), got {tuple(elastic.shape)}")
    if mirror is not None and (mirror.shape != (B, 3) or mirror.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"{what}: mirror must be a bool or uint8 tensor of shape ({B}, 3)")
    ia, ib = (1.0, 0.0) if intensity is None else (float(intensity[0]), float(intensity[1]))
    _need_gpu(img, seg, matrix, centre, elastic, mirror)
    dev = matrix.device
    with torch.no_grad():
        src, C, out_img = None, 0, None
        if img is not None:
            src = bspline_prefilter(img) if order_data == 3 and not prefiltered else _f32c(img)
            C = src.shape[1]
            out_img = torch.empty(B, C, pd, ph, pw, dtype=torch.float32, device=dev)
        lab, Cs, kind, out_seg = None, 0, 0, None
        if seg is not None:
            lab = seg.contiguous() if seg.dtype in _LABEL_KINDS else seg.to(torch.int32).contiguous()
            Cs, kind = lab.shape[1], _LABEL_KINDS[lab.dtype]
            out_seg = torch.empty(B, Cs, pd, ph, pw, dtype=torch.int64, device=dev)
        m, c = _f32c(matrix), _f32c(centre)
        e = None if elastic is None else _f32c(elastic)
        f = None if mirror is None else mirror.contiguous().view(torch.uint8)
        launch(dev, "fsg_spatial_resample_f32", _p(src), C, order_data, _p(lab), kind, Cs, order_seg, B, D, H, W, pd, ph, pw,
               _p(m), _p(c), _p(e), _p(f), ia, ib, _p(out_img), _p(out_seg))
    return out_img, out_seg
