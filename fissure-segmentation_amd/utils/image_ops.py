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
