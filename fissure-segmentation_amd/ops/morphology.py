"""Bit-plane volumes: ball morphology, thinning, connected components (csrc/morphology.hip, csrc/thinning.hip); the Euclidean
distance transform and what sits on it (csrc/edt.hip)."""
import torch

from .. import _lib
from .._launch import _need_gpu, _p, _stream, launch


# ------------------------------------------------------------------ ball morphology, connected components (csrc/morphology.hip)
def _radius3(radius):
    """an int or three ints (rz, ry, rx), each 0..8"""
    if isinstance(radius, int) and not isinstance(radius, bool):
        r = (radius,) * 3
    else:
        r = tuple(radius) if isinstance(radius, (tuple, list)) else ()
    if len(r) != 3 or any(not isinstance(x, int) or isinstance(x, bool) for x in r):
        raise ValueError(f"radius must be an int or three ints (rz, ry, rx), got {radius!r}")
    if any(x < 0 or x > _lib.MORPH_MAX_RADIUS for x in r):
        raise ValueError(f"radius {r} outside 0..{_lib.MORPH_MAX_RADIUS}")
    return r


def ball_offsets(radius):
    """the offsets (n, 3) int64 (dz, dy, dx), in raster order, of the ball structuring element of per-axis radius
    (rz, ry, rx): sum_i (o_i / (r_i + 0.5))^2 <= 1 (an axis of radius 0 contributes only 0) -- the definition used here in
    place of sitk.sitkBall (parity with SimpleITK is unpinned).  Decided in integers: with m = 2 r + 1 the
    test is 4 sum_i o_i^2 prod_{j != i} m_j^2 <= prod_j m_j^2, whose sides have different parity."""
    rz, ry, rx = _radius3(radius)
    mz, my, mx = (2 * rz + 1) ** 2, (2 * ry + 1) ** 2, (2 * rx + 1) ** 2
    offs = [(dz, dy, dx) for dz in range(-rz, rz + 1) for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)
            if 4 * (dz * dz * my * mx + dy * dy * mz * mx + dx * dx * mz * my) <= mz * my * mx]
    return torch.tensor(offs, dtype=torch.int64)


def _binary_volume(vol, what):
    """(D, H, W) or (B, D, H, W), bool or integer -> the tensor as (B, D, H, W) and whether it came without a batch axis"""
    if vol.dim() not in (3, 4) or vol.is_floating_point() or vol.is_complex():
        raise ValueError(f"{what}: expected a bool or integer volume (D, H, W) or (B, D, H, W), got {tuple(vol.shape)} {vol.dtype}")
    if vol.numel() == 0:
        raise ValueError(f"{what}: empty volume {tuple(vol.shape)}")
    _need_gpu(vol)
    return (vol[None] if vol.dim() == 3 else vol), vol.dim() == 3


def _pack_bits(v4, value=None):
    """(B, D, H, W) bool / integer on the device -> bit plane (B, D, H, ceil(W / 64)) int64: voxel != 0, or == value (0..255
    on a uint8 volume)"""
    if v4.dtype == torch.bool:
        src = v4.contiguous().view(torch.uint8)
    elif v4.dtype == torch.uint8:
        src = v4.contiguous()
    elif value is None:
        src = (v4 != 0).contiguous().view(torch.uint8)       # (a comparison keeps the strides of a permuted input)
    else:
        src, value = (v4 == value).contiguous().view(torch.uint8), None
    B, D, H, W = src.shape
    bits = torch.empty(B, D, H, (W + 63) // 64, dtype=torch.int64, device=src.device)
    launch(src.device, "fsg_bits_pack_u8", _p(src), B, D, H, W, -1 if value is None else int(value), _p(bits))
    return bits


def _unpack_bits(bits, W):
    B, D, H, _ = bits.shape
    out = torch.empty(B, D, H, W, dtype=torch.uint8, device=bits.device)
    launch(bits.device, "fsg_bits_unpack_u8", _p(bits), B, D, H, W, _p(out))
    return out.view(torch.bool)   # the kernel writes 0 or 1: a view, not a pass


def _bits_dilate(bits, W, r, border=0, inv_in=False, inv_out=False):
    """one launch on a bit plane: [not] dilate([not] bits) with the ball of radius r = (rz, ry, rx) and the border value"""
    B, D, H, _ = bits.shape
    out = torch.empty_like(bits)
    launch(bits.device, "fsg_ball_dilate_bits", _p(bits), B, D, H, W, r[0], r[1], r[2], int(border), int(inv_in), int(inv_out), _p(out))
    return out


def _bits_erode(bits, W, r, border=1):
    """erosion = the complement of the dilation of the complement with the complementary border (the ball is symmetric)"""
    return _bits_dilate(bits, W, r, border=1 - int(border), inv_in=True, inv_out=True)


def _bits_window(bits, W, offset, out_dhw):
    """the box of size out_dhw whose corner sits at `offset` of the volume (negative: padding with 0), in bit-plane space"""
    B, D, H, _ = bits.shape
    Do, Ho, Wo = out_dhw
    out = torch.empty(B, Do, Ho, (Wo + 63) // 64, dtype=torch.int64, device=bits.device)
    launch(bits.device, "fsg_bits_window", _p(bits), B, D, H, W, offset[0], offset[1], offset[2], Do, Ho, Wo, _p(out))
    return out


def _bits_closing(bits, W, r):
    """closing on the zero-extended infinite grid, cropped: the dilation is also formed r voxels outside the volume (the
    plane is padded in bit space, never as bytes), so the erosion sees what it would on the infinite grid"""
    B, D, H, _ = bits.shape
    Wp = W + 2 * r[2]
    padded = _bits_window(bits, W, (-r[0], -r[1], -r[2]), (D + 2 * r[0], H + 2 * r[1], Wp))
    closed = _bits_erode(_bits_dilate(padded, Wp, r, border=0), Wp, r, border=0)
    return _bits_window(closed, Wp, r, (D, H, W))


def _bits_opening(bits, W, r):
    """dilate(erode(x, border 0), border 0): what the zero-extended infinite grid gives, cropped"""
    return _bits_dilate(_bits_erode(bits, W, r, border=0), W, r, border=0)


def _morph_public(vol, radius, what, op):
    r = _radius3(radius)
    v4, squeeze = _binary_volume(vol, what)
    with torch.no_grad():
        out = _unpack_bits(op(_pack_bits(v4), v4.shape[-1], r), v4.shape[-1])
    return out[0] if squeeze else out


def _border01(border):
    if border not in (0, 1, False, True):
        raise ValueError(f"border must be 0 or 1, got {border!r}")
    return int(border)


def binary_dilate(vol, radius, border=0):
    """sitk.BinaryDilate with a ball (find_lobes.py:123): vol (D, H, W) or (B, D, H, W), bool or integer (nonzero = set) ->
    bool.  radius an int or (rz, ry, rx), each 0..8, the ball of `ball_offsets`; `border` is the value outside the volume."""
    b = _border01(border)
    return _morph_public(vol, radius, "binary_dilate", lambda bits, W, r: _bits_dilate(bits, W, r, border=b))


def binary_erode(vol, radius, border=1):
    """sitk.BinaryErode with a ball (find_lobes.py:118; its boundary counts as foreground, hence border = 1)"""
    b = _border01(border)
    return _morph_public(vol, radius, "binary_erode", lambda bits, W, r: _bits_erode(bits, W, r, border=b))


def binary_closing(vol, radius):
    """sitk.BinaryMorphologicalClosing with a ball (find_lobes.py:122) on the zero-extended infinite grid, cropped"""
    return _morph_public(vol, radius, "binary_closing", _bits_closing)


def binary_opening(vol, radius):
    """sitk.BinaryMorphologicalOpening with a ball (find_lobes.py:128) on the zero-extended infinite grid, cropped"""
    return _morph_public(vol, radius, "binary_opening", _bits_opening)


def _thin_slice_fits(H, W):
    words = H * ((W + 63) // 64)
    if words > _lib.THIN_MAX_WORDS:
        raise ValueError(f"binary_thinning: a slice of {H} x {W} voxels is {words} words of 64 voxels, at most "
                         f"{_lib.THIN_MAX_WORDS} (H * ceil(W / 64)) fit in LDS")


def _bits_thin(bits, W, want_iterations=False):
    """one launch on a bit plane (csrc/thinning.hip): every slice thinned in its (y, x) plane until a pair of steps clears
    nothing -> (thinned plane, (B, D) int32 pair counts or None).  No host read."""
    B, D, H, _ = bits.shape
    _thin_slice_fits(H, W)
    out = torch.empty_like(bits)
    iters = torch.empty(B, D, dtype=torch.int32, device=bits.device) if want_iterations else None
    launch(bits.device, "fsg_thin_bits", _p(bits), B, D, H, W, _p(out), _p(iters))
    return out, iters


def binary_thinning(vol, return_iterations=False):
    """sitk.BinaryThinning as poisson_reconstruction uses it (data_processing/surface_fitting.py:109): vol (D, H, W) or
    (B, D, H, W), bool or integer (nonzero = set), any strides -> bool of the same shape; the input is not modified.  The
    two-sub-iteration thinning of Gonzalez & Woods in the (y, x) plane of every slice, clamped borders: slices never
    interact, so a sheet that crosses the slices becomes a one-voxel-wide sheet, not a curve.  The rule of csrc/thinning.hip
    and tests/thinning_oracle.py is the authority, parity with SimpleITK is unpinned.  A slice may hold at most
    `_lib.THIN_MAX_WORDS` words, H * ceil(W / 64) (ValueError beyond).  return_iterations: also the int32 (D) or (B, D)
    numbers of step pairs that cleared something, on the device.  One launch between the pack and the unpack, no host read."""
    v4, squeeze = _binary_volume(vol, "binary_thinning")
    W = v4.shape[-1]
    _thin_slice_fits(v4.shape[-2], W)        # before any work
    with torch.no_grad():
        bits, iters = _bits_thin(_pack_bits(v4), W, return_iterations)
        out = _unpack_bits(bits, W)
    if squeeze:
        out, iters = out[0], (iters[0] if return_iterations else None)
    return (out, iters) if return_iterations else out


def _cc_bits(bits, W, connectivity):
    """bit plane -> (labels (B, D, H, W) int32, n (B) int32 on the device): no host read"""
    B, D, H, _ = bits.shape
    dev = bits.device
    ws = _lib.workspace("fsg_cc", B, D, H, W, device=dev)
    labels = torch.empty(B, D, H, W, dtype=torch.int32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    launch(dev, "fsg_cc_label_bits", _p(bits), B, D, H, W, int(connectivity), _p(labels), _p(n), _p(ws), ws.numel())
    return labels, n


def _stats_device(labels4, cap):
    """(B, D, H, W) int32 labels -> (B, cap, 4) int64 on the device: count, sum z, sum y, sum x of the labels 1..cap"""
    B, D, H, W = labels4.shape
    stats = torch.empty(B, cap, 4, dtype=torch.int64, device=labels4.device)
    launch(labels4.device, "fsg_component_stats_i32", _p(labels4), B, D, H, W, int(cap), _p(stats))
    return stats


def _labels_volume(labels, what):
    if labels.dim() not in (3, 4) or labels.dtype != torch.int32:
        raise ValueError(f"{what}: expected int32 labels (D, H, W) or (B, D, H, W), got {tuple(labels.shape)} {labels.dtype}")
    _need_gpu(labels)
    return (labels[None] if labels.dim() == 3 else labels).contiguous(), labels.dim() == 3


def _count(n, B, what):
    """n as given to component_stats / relabel_by_size: an int, or one int per item -> the capacity max(n, 1)"""
    ns = [n] if isinstance(n, int) else list(n)
    if any(not isinstance(x, int) or x < 0 for x in ns) or len(ns) not in (1, B):
        raise ValueError(f"{what}: n must be a non-negative int (or one per item), got {n!r}")
    return max(max(ns), 1)


def connected_components(mask, connectivity=6):
    """sitk.ConnectedComponentImageFilter (find_lobes.py:130-132; 6 is its default, fullyConnected is 26): mask (D, H, W) or
    (B, D, H, W), bool or integer (nonzero = object) -> (labels int32, n).  Components are numbered 1..n in raster order of
    their first voxel, as scipy.ndimage.label numbers them; n is an int, or a list of B ints for a batch (one host read)."""
    if connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    v4, squeeze = _binary_volume(mask, "connected_components")
    with torch.no_grad():
        labels, n = _cc_bits(_pack_bits(v4), v4.shape[-1], connectivity)
        n = n.tolist()
    return (labels[0], n[0]) if squeeze else (labels, n)


def component_stats(labels, n):
    """sizes and index sums of the labels 1..n (RelabelComponentImageFilter's sizes, LabelShapeStatisticsImageFilter's
    centroids before the division; find_lobes.py:141-158): labels int32 (D, H, W) -> (sizes (n) int64, index_sums (n, 3)
    int64 in (z, y, x) order), on the device, exact; a batch (B, D, H, W) with n = max over the items -> (B, n), (B, n, 3).
    No host read."""
    l4, squeeze = _labels_volume(labels, "component_stats")
    cap = _count(n, l4.shape[0], "component_stats")
    n_max = max([n] if isinstance(n, int) else list(n))
    with torch.no_grad():
        stats = _stats_device(l4, cap)[:, :n_max]
    sizes, sums = stats[..., 0], stats[..., 1:]
    return (sizes[0], sums[0]) if squeeze else (sizes, sums)


def _size_order_lut(sizes):
    """(B, n) int64 sizes -> lut (B, n + 1) int32: old label -> rank by size, largest first, ties by the smaller label (a
    stable sort)"""
    B, n = sizes.shape
    order = torch.sort(sizes, dim=1, descending=True, stable=True).indices           # order[b, new - 1] = old - 1
    lut = torch.zeros(B, n + 1, dtype=torch.int32, device=sizes.device)
    lut.scatter_(1, order + 1, torch.arange(1, n + 1, dtype=torch.int32, device=sizes.device).expand(B, n).contiguous())
    return lut


def _apply_lut(l4, lut, out_dtype=torch.int32):
    B = l4.shape[0]
    out = torch.empty(l4.shape, dtype=out_dtype, device=l4.device)
    lut = lut.contiguous()
    launch(l4.device, "fsg_relabel_lut_i32", _p(l4), B, l4[0].numel(), _p(lut), lut.shape[1], _p(out), int(out_dtype == torch.int64))
    return out


def relabel_by_size(labels, n):
    """sitk.RelabelComponentImageFilter with SortByObjectSize (find_lobes.py:141-143): label 1 becomes the largest component;
    equal sizes keep the order of their labels (this rule is ours, ITK's is unpinned).  labels int32 with values 0..n -> int32.
    Items of a batch whose count is below n have empty trailing labels, which sort last.  No host read."""
    l4, squeeze = _labels_volume(labels, "relabel_by_size")
    cap = _count(n, l4.shape[0], "relabel_by_size")
    with torch.no_grad():
        lut = _size_order_lut(_stats_device(l4, cap)[..., 0])
        out = _apply_lut(l4, lut)
    return out[0] if squeeze else out


# ------------------------------------------------------------------ Euclidean distance transform (csrc/edt.hip)
EDT_MAX_DIM = _lib.EDT_MAX_DIM
EDT_MAX_LABELS = _lib.EDT_MAX_LABELS
EDT_INT_INF = 2 ** 31 - 1    # the int32 mode's +inf


def _edt_shape(shape, what):
    D, H, W = (int(v) for v in shape[-3:])
    if max(D, H, W) > EDT_MAX_DIM or D * H * W >= 2 ** 31:
        raise ValueError(f"{what}: volume {(D, H, W)}: a dimension above {EDT_MAX_DIM} or 2^31 voxels or more")


def _edt_sampling(sampling, what):
    """None -> None (unit spacing: the int32 mode); a number or three (s0, s1, s2) for (D, H, W) -> three floats rounded to
    fp32, what the kernel computes with"""
    if sampling is None:
        return None
    s = (sampling,) * 3 if isinstance(sampling, (int, float)) and not isinstance(sampling, bool) else tuple(sampling)
    if len(s) != 3:
        raise ValueError(f"{what}: sampling must be None, a number or three numbers for (D, H, W), got {sampling!r}")
    s = tuple(float(torch.tensor(float(v), dtype=torch.float32)) for v in s)
    if any(not (0.0 < v <= 1e6) for v in s):
        raise ValueError(f"{what}: sampling {sampling!r} must be positive and at most 1e6")
    return s


def _edt_bits(bits, W, sampling, want_idx):
    """bit plane (B, D, H, WW) -> (d2 (B, D, H, W) int32 for unit spacing / fp32, site index (B, D, H, W) int32 or None).  Three
    launches on the current stream, no host read."""
    B, D, H, _ = bits.shape
    dev = bits.device
    d2 = torch.empty(B, D, H, W, dtype=torch.int32 if sampling is None else torch.float32, device=dev)
    idx = torch.empty(B, D, H, W, dtype=torch.int32, device=dev) if want_idx else None
    ws = _lib.workspace("fsg_edt", B, D, H, W, int(want_idx), device=dev)
    with torch.cuda.device(dev):
        if sampling is None:
            _lib.call("fsg_edt_sq_i32", _p(bits), B, D, H, W, _p(d2), _p(idx), _p(ws), ws.numel(), _stream())
        else:
            _lib.call("fsg_edt_sq_f32", _p(bits), B, D, H, W, sampling[0], sampling[1], sampling[2], _p(d2), _p(idx), _p(ws),
                      ws.numel(), _stream())
    return d2, idx


def distance_transform_edt(vol, sampling=None, return_distances=True, return_indices=False, squared=False):
    """scipy.ndimage.distance_transform_edt on the device (process_lung_mask.py:85): vol (D, H, W) or (B, D, H, W), bool or
    integer, nonzero = set; every voxel gets the Euclidean distance to the nearest zero voxel (a SITE) of its item, under
    `sampling` = None (unit), a number, or (s0, s1, s2) for (D, H, W).  Exact and separable (csrc/edt.hip).

    Distances are float32 square roots of the squared values; `squared=True` returns the squared values themselves: int32,
    exact, for sampling=None, else float32 (each term fl(fl(s * delta)^2), sums rounded once, no fused multiply-add; the
    spacings are rounded to fp32 first).  Indices are (3, D, H, W) int32 -- (B, 3, D, H, W) for a batch -- the (z, y, x) of the
    site that won.  Returns the distances, the indices, or (distances, indices), as scipy does.

    Where this is NOT scipy: an item without a zero voxel gives +inf distances (2^31 - 1 as squared int32) and -1 indices
    (scipy returns garbage there); among equidistant sites the winner is, per pass (W, then H, then D), the one with the
    smaller offset and then the lower index, which is not scipy's choice."""
    if not (return_distances or return_indices):
        raise ValueError("distance_transform_edt: at least one of return_distances / return_indices must be set")
    if vol.dim() in (3, 4):
        _edt_shape(vol.shape, "distance_transform_edt")
    s = _edt_sampling(sampling, "distance_transform_edt")
    v4, squeeze = _binary_volume(vol, "distance_transform_edt")
    B, D, H, W = v4.shape
    with torch.no_grad():
        d2, idx = _edt_bits(_pack_bits(v4), W, s, return_indices)
        out = []
        if return_distances:
            if squared:
                dist = d2
            else:
                dist = d2.to(torch.float32).sqrt_()
                if s is None:
                    dist.masked_fill_(d2 == EDT_INT_INF, float("inf"))
            out.append(dist[0] if squeeze else dist)
        if return_indices:
            x = idx % W
            y = torch.div(idx, W, rounding_mode="floor") % H
            z = torch.div(idx, H * W, rounding_mode="floor")
            zyx = torch.stack((z, y, x), 1)
            zyx.masked_fill_((idx < 0)[:, None], -1)
            out.append(zyx[0] if squeeze else zyx)
    return out[0] if len(out) == 1 else tuple(out)


def nearest_label(labels, candidates, sampling=None, keep=None):
    """For every voxel of `labels` (D, H, W), integer, the member of `candidates` whose nearest voxel is closest (Euclidean,
    under `sampling` as in `distance_transform_edt`) -> int32 (D, H, W).  On an exact tie the lowest label wins, as np.argmin
    over the distance maps in label order does (process_lung_mask.py:83-87; the feature transform has another tie rule and
    cannot stand in).  One batched distance transform over len(candidates) bit planes and one compare launch; with unit
    spacing the compare is exact in integers.  A candidate without voxels is infinitely far; if none has any, the lowest is
    returned.  `keep` (D, H, W), bool or uint8: voxels where it is 0 get 0 (process_lung_mask.py:88).  No host read."""
    cands = sorted({int(c) for c in candidates})
    if not cands or len(cands) > EDT_MAX_LABELS or len(cands) != len(list(candidates)):
        raise ValueError(f"nearest_label: candidates must be 1..{EDT_MAX_LABELS} distinct integers, got {candidates!r}")
    if labels.dim() != 3 or labels.is_floating_point() or labels.is_complex() or labels.numel() == 0:
        raise ValueError(f"nearest_label: expected an integer label map (D, H, W), got {tuple(labels.shape)} {labels.dtype}")
    _edt_shape(labels.shape, "nearest_label")
    s = _edt_sampling(sampling, "nearest_label")
    _need_gpu(labels, keep)
    if keep is not None and (keep.shape != labels.shape or keep.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"nearest_label: keep must be bool or uint8 of shape {tuple(labels.shape)}")
    D, H, W = labels.shape
    dev = labels.device
    with torch.no_grad():
        cand_t = torch.tensor(cands, dtype=torch.int32, device=dev)
        planes = labels[None] != cand_t[:, None, None, None]       # (K, D, H, W) bool; the comparison promotes, never wraps
        d2, _ = _edt_bits(_pack_bits(planes), W, s, False)          # a candidate's voxels are the sites of its plane
        out = torch.empty(D, H, W, dtype=torch.int32, device=dev)
        k8 = None if keep is None else keep.contiguous().view(torch.uint8)
        launch(dev, "fsg_edt_nearest_label", _p(d2), int(s is not None), len(cands), D * H * W, _p(cand_t), _p(k8), _p(out))
    return out


def _quantile_linear(d, q):
    """torch.quantile(d, q) (linear interpolation) of a 1-D tensor of any length: torch.quantile itself up to its limit of
    metrics.QUANTILE_MAX_ELEMENTS, above it the same formula on a sort"""
    from .. import metrics
    n = d.numel()
    if n <= metrics.QUANTILE_MAX_ELEMENTS:
        return torch.quantile(d, q)
    srt = torch.sort(d).values
    pos = q * (n - 1)
    lo = int(pos)
    hi = min(lo + 1, n - 1)
    return srt[lo] + (srt[hi] - srt[lo]) * (pos - lo)


def labelmap_distances(a, b, spacing=(1., 1., 1.)):
    """The symmetric surface-distance statistics between the voxel clouds of two label maps -- what the reference's
    `label_label_assd` (metrics.py:79-93) measures with open3d point-cloud distances -> (mean, std, hd, hd95), fp64 tensors on
    the device, each the average of the two directions (`metrics._symmetric_point_distances`).  a, b (D, H, W), bool or integer,
    nonzero = set; `spacing` in (x, y, z), as `mask_to_points` takes it.  The distance from a set voxel of `a` to the nearest
    set voxel of `b` is the distance transform of b == 0 read at that voxel (squared distances in fp32 as in
    `distance_transform_edt`, square roots and statistics in fp64).  An empty mask gives four NaNs (`metrics._nan4`).  Parity
    with open3d is unpinned; scipy's transform is the checker."""
    from .. import metrics
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"labelmap_distances: expected two volumes (D, H, W) of one shape, got {tuple(a.shape)}, {tuple(b.shape)}")
    _need_gpu(a, b)
    sx, sy, sz = (float(v) for v in spacing)
    with torch.no_grad():
        am, bm = a != 0, b != 0
        if not bool(am.any()) or not bool(bm.any()):
            return metrics._nan4()
        d2 = distance_transform_edt(torch.stack((~bm, ~am)), sampling=(sz, sy, sx), squared=True)
        d_ab, d_ba = d2[0][am].double().sqrt_(), d2[1][bm].double().sqrt_()
        if max(d_ab.numel(), d_ba.numel()) <= metrics.QUANTILE_MAX_ELEMENTS:
            return metrics._symmetric_point_distances(d_ab, d_ba)
        both = (d_ab, d_ba)
        return (sum(d.mean() for d in both) / 2, sum(d.std() for d in both) / 2, sum(d.max() for d in both) / 2,
                sum(_quantile_linear(d, 0.95) for d in both) / 2)
