"""utils/image_ops.py of the reference for tensors: the label-map morphology that keypoints and data sets use
(keypoint_extraction.py:175, data.py:311).  No SimpleITK: convert with `torch.from_numpy(sitk.GetArrayFromImage(img))` on
the way in."""
import torch

from .. import functional as F_hip


def multiple_objects_morphology(labelmap: torch.Tensor, radius, mode: str = 'dilate') -> torch.Tensor:
    """image_ops.py:31-47 (sitk.DilateObjectMorphology / ErodeObjectMorphology with the ball, object by object): for each
    nonzero label i ascending, 'dilate' paints i over every voxel its dilation reaches -- a later label overwrites an earlier
    one where they collide, and sees the map as the earlier ones left it --, 'erode' sets the voxels of i outside its erosion
    (border 1) to 0.  labelmap (D, H, W) integer with labels 0..255 on the device -> uint8, like the reference's cast.  One
    host read (the labels present)."""
    if mode not in ('dilate', 'erode'):
        raise ValueError(f'No morphology operation named "{mode}". Use "dilate" or "erode".')
    r = F_hip._radius3(radius)
    if labelmap.dim() != 3 or labelmap.is_floating_point() or labelmap.dtype == torch.bool:
        raise ValueError(f"expected an integer label map (D, H, W), got {tuple(labelmap.shape)} {labelmap.dtype}")
    F_hip._need_gpu(labelmap)
    with torch.no_grad():
        objects = torch.unique(labelmap).tolist()
        if objects and (objects[0] < 0 or objects[-1] > 255):
            raise ValueError(f"labels span {objects[0]}..{objects[-1]}, outside 0..255")
        out = labelmap.to(torch.uint8).contiguous()[None].clone()
        W = out.shape[-1]
        for i in objects:
            if i == 0:
                continue
            obj = F_hip._pack_bits(out, value=i)     # the object of label i in the map as it stands: no one-hot volume
            if mode == 'dilate':
                out.masked_fill_(F_hip._unpack_bits(F_hip._bits_dilate(obj, W, r, border=0), W), i)
            else:
                gone = obj & ~F_hip._bits_erode(obj, W, r, border=1)
                out.masked_fill_(F_hip._unpack_bits(gone, W), 0)
    return out[0]


def get_resample_factors(current_spacing, target_spacing: float = 1.):
    """image_ops.py:8-9"""
    return [spacing / target_spacing for spacing in current_spacing]


def resample_equal_spacing(img: torch.Tensor, spacing, target_spacing: float = 1., use_nearest_neighbor: bool = False):
    """image_ops.py:12-28 for a tensor: img (D, H, W) on the device with voxel `spacing` (one number per axis, in the tensor's
    axis order) -> (resampled, new_spacing).  The output size is round(size * spacing / target) with Python's round; when no
    size changes the SAME tensor comes back with its spacing.  Output and input share their origin: output index i reads
    input index i * target / spacing -- the fused resample kernel (csrc/spatial.hip) with a diagonal matrix, trilinear, or
    nearest (floor(x + 0.5)) with use_nearest_neighbor.  Border rule (ours; parity with sitk.Resample is unpinned, SimpleITK
    is not installed): a coordinate past the last sample reads the last sample (edge replication).  The result has the dtype
    of `img`; integer volumes go through fp32, which holds labels up to 2^24 exactly."""
    if img.dim() != 3 or img.numel() == 0 or img.is_complex() or img.dtype == torch.bool:
        raise ValueError(f"resample_equal_spacing: expected a numeric volume (D, H, W), got {tuple(img.shape)} {img.dtype}")
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3 or not all(s > 0 for s in spacing) or not float(target_spacing) > 0:
        raise ValueError(f"resample_equal_spacing: spacing {spacing!r} / target {target_spacing!r} must be positive, three axes")
    F_hip._need_gpu(img)
    factors = get_resample_factors(spacing, target_spacing)
    output_size = [round(size * factor) for size, factor in zip(img.shape, factors)]
    if all(i == o for i, o in zip(img.shape, output_size)):
        return img, spacing
    if min(output_size) < 1:
        raise ValueError(f"resample_equal_spacing: output size {output_size} has an empty axis")
    dev = img.device
    step = torch.tensor([1.0 / f for f in factors], dtype=torch.float64)
    matrix = torch.diag(step).to(torch.float32)[None].to(dev)
    half = torch.tensor([(o - 1) / 2 for o in output_size], dtype=torch.float64)
    centre = (matrix[0].cpu().double() @ half).to(torch.float32)[None].to(dev)
    out, _ = F_hip.spatial_transform(img[None, None].to(torch.float32), None, output_size, matrix, centre,
                                     order_data=0 if use_nearest_neighbor else 1)
    out = out[0, 0]
    if not img.is_floating_point():
        out = out.round().to(img.dtype)
    elif out.dtype != img.dtype:
        out = out.to(img.dtype)
    return out, (float(target_spacing),) * 3
