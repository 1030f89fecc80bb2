"""Point-to-mesh distance (csrc/point_mesh.hip) and meshes -> voxel label maps (csrc/voxelize.hip)."""
import torch

from .._launch import _f32c, _need_gpu, _p, launch


# ------------------------------------------------------------------ point-to-mesh distance (metrics.py:11-25)
_faces_checked = {}   # (storage, data_ptr, version, shape, strides, dtype) -> (weak storage reference, lowest, highest index)


def _faces_range(faces):
    """(lowest, highest) index of a faces tensor: one reduction and one synchronisation per tensor, remembered by storage,
    address and version counter (an in-place write bumps the version, so a modified list is looked at again).  The entry
    holds a weak reference to the storage: an address alone says nothing once the tensor is gone and the allocator has handed
    its memory to another one."""
    from torch.multiprocessing.reductions import StorageWeakRef
    storage = faces.untyped_storage()
    key = (storage._cdata, faces.data_ptr(), faces._version, tuple(faces.shape), faces.stride(), faces.dtype)
    got = _faces_checked.get(key)
    if got is None or got[0].expired():
        for k in [k for k, v in _faces_checked.items() if v[0].expired()]:
            del _faces_checked[k]
        if len(_faces_checked) >= 64:
            _faces_checked.clear()
        lo, hi = torch.aminmax(faces)
        got = _faces_checked[key] = (StorageWeakRef(storage), int(lo), int(hi))
    return got[1], got[2]


def point_mesh_distance(points, verts, faces, return_face=False, return_closest=False, validate=True):
    """Unsigned Euclidean distance from every point to a triangle mesh (fsg_point_mesh_dist_f32; the square root is torch's).

    points (B,P,3), verts (B,V,3), faces (F,3) shared by all meshes or (B,F,3) -> dist (B,P) fp32
    [, face (B,P) int32: a face that attains it, the lowest index on ties][, closest (B,P,3): the closest point on it].
    Faces without area are legal (distance to their longest edge, or to the point).  `validate` checks the face indices
    against V once per faces tensor; the kernel itself does not.  P == 0 gives empty results, F == 0 (or V == 0) NaN
    distances, face -1 and NaN closest points; no kernel is launched then.

    An evaluation primitive, NOT differentiable: it runs under torch.no_grad and its outputs never require grad.  A
    point-to-surface loss (the gradient with respect to points and vertices) is not part of this package yet."""
    _need_gpu(points, verts, faces)
    if (points.dim() != 3 or verts.dim() != 3 or points.shape[2] != 3 or verts.shape[2] != 3 or points.shape[0] != verts.shape[0]
            or faces.dim() not in (2, 3) or faces.shape[-1] != 3 or (faces.dim() == 3 and faces.shape[0] != verts.shape[0])):
        raise ValueError(f"expected points (B,P,3), verts (B,V,3) and faces (F,3) or (B,F,3), got {tuple(points.shape)}, "
                         f"{tuple(verts.shape)} and {tuple(faces.shape)}")
    if faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError(f"faces must hold integer vertex indices, got {faces.dtype}")
    with torch.no_grad():
        pc, vc = _f32c(points), _f32c(verts)
        B, P, _ = pc.shape
        V, F = vc.shape[1], faces.shape[-2]
        dev = pc.device
        if P == 0 or F == 0 or V == 0 or B == 0:
            out = [torch.full((B, P), float("nan"), dtype=torch.float32, device=dev)]
            if return_face:
                out.append(torch.full((B, P), -1, dtype=torch.int32, device=dev))
            if return_closest:
                out.append(torch.full((B, P, 3), float("nan"), dtype=torch.float32, device=dev))
            return out[0] if len(out) == 1 else tuple(out)
        if validate:
            lo, hi = _faces_range(faces)
            if lo < 0 or hi >= V:
                raise ValueError(f"face indices span [{lo}, {hi}] but the mesh has {V} vertices")
        fc = faces.detach().to(torch.int32).contiguous()
        d2 = torch.empty(B, P, dtype=torch.float32, device=dev)
        face = torch.empty(B, P, dtype=torch.int32, device=dev) if return_face else None
        closest = torch.empty(B, P, 3, dtype=torch.float32, device=dev) if return_closest else None
        launch(dev, "fsg_point_mesh_dist_f32", _p(pc), _p(vc), _p(fc), B, P, V, F, B if fc.dim() == 3 else 1, _p(d2), _p(face),
               _p(closest))
        out = [d2.sqrt_()] + [t for t in (face, closest) if t is not None]
    return out[0] if len(out) == 1 else tuple(out)


# ------------------------------------------------------------------ meshes -> voxel label maps (csrc/voxelize.hip)
def _pack_meshes(who, verts, faces, shape, spacing, validate):
    """the meshes of one call as one vertex list, one face list (indices shifted) and the mesh number of every face; meshes
    without vertices or faces are left out but keep their number.  -> (verts, faces, labels) or None if nothing is left,
    shape and spacing as tuples, the device"""
    verts, faces = ([x] if torch.is_tensor(x) else list(x) for x in (verts, faces))
    if len(verts) != len(faces) or not verts:
        raise ValueError(f"{who}: expected as many vertex tensors as face tensors and at least one, got {len(verts)} and {len(faces)}")
    _need_gpu(*verts, *faces)
    shape, spacing = tuple(int(n) for n in shape), tuple(float(s) for s in spacing)
    if len(shape) != 3 or len(spacing) != 3:
        raise ValueError(f"{who}: expected a 3-D shape and one spacing per axis, got {shape} and {spacing}")
    dev = verts[0].device
    vs, fs, ls, base = [], [], [], 0
    for m, (v, f) in enumerate(zip(verts, faces)):
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"{who}: mesh {m}: expected verts (V,3) and faces (F,3), got {tuple(v.shape)} and {tuple(f.shape)}")
        if f.is_floating_point() or f.dtype == torch.bool:
            raise ValueError(f"{who}: mesh {m}: faces must hold integer vertex indices, got {f.dtype}")
        if v.shape[0] == 0 or f.shape[0] == 0:
            continue
        if validate:
            lo, hi = _faces_range(f)
            if lo < 0 or hi >= v.shape[0]:
                raise ValueError(f"{who}: mesh {m}: face indices span [{lo}, {hi}] but the mesh has {v.shape[0]} vertices")
            if not bool(torch.isfinite(v).all()):
                raise ValueError(f"{who}: mesh {m} has a non-finite vertex")
        vs.append(_f32c(v))
        fs.append(f.detach().to(torch.int32) + base)
        ls.append(torch.full((f.shape[0],), m, dtype=torch.int32, device=dev))
        base += v.shape[0]
    packed = (torch.cat(vs), torch.cat(fs).contiguous(), torch.cat(ls)) if vs else None
    return packed, shape, spacing, dev


def mesh_labelmap_dist(verts, faces, shape, spacing, dist_threshold=1.0, mask=None, validate=True):
    """Label map of the voxels within `dist_threshold` of a set of triangle meshes (fsg_mesh_labelmap_dist_f32).

    verts: list of (V_m,3), faces: list of (F_m,3) integer tensors on the GPU (one tensor each for a single mesh); vertex
    coordinates in the axis order of the volume, in the units of `spacing` (s0, s1, s2); voxel (i0,i1,i2) has the centre
    (i0 s0, i1 s1, i2 s2).  -> int64 tensor of `shape`: 1 + m for the mesh m of smallest distance if that distance is
    <= dist_threshold and `mask` (bool, `shape`; None = everywhere) is set, else 0; the lowest m on an exact tie.  A mesh
    without vertices or faces takes part in nothing, the others keep their numbers.  Distances are those of
    `point_mesh_distance`; faces without area are legal.  Bitwise reproducible.

    `validate` checks the face indices against V (once per faces tensor) and that the vertices are finite, and raises
    ValueError before anything is launched; the kernel clips in float and never forms an index from a coordinate outside
    the volume, but does not check face indices.  Not differentiable."""
    packed, shape, spacing, dev = _pack_meshes("mesh_labelmap_dist", verts, faces, shape, spacing, validate)
    if mask is not None:
        _need_gpu(mask)
        if tuple(mask.shape) != shape:
            raise ValueError(f"mesh_labelmap_dist: mask of shape {tuple(mask.shape)} for a volume of {shape}")
        mask = (mask.detach() != 0).contiguous()
    if packed is None:
        return torch.zeros(shape, dtype=torch.int64, device=dev)
    v, f, lab = packed
    out = torch.empty(shape, dtype=torch.int64, device=dev)
    keys = torch.empty(shape, dtype=torch.int64, device=dev)
    launch(dev, "fsg_mesh_labelmap_dist_f32", _p(v), _p(f), _p(lab), v.shape[0], f.shape[0], *shape, *spacing,
           float(dist_threshold), _p(mask), _p(keys), _p(out))
    return out


def mesh_labelmap_cover(verts, faces, shape, spacing, validate=True):
    """Label map of the cells that the surface of a set of triangle meshes passes through (fsg_mesh_labelmap_cover_f32): what
    scattering floor(sample / spacing) of surface samples tends to as their number grows.

    Arguments as for `mesh_labelmap_dist`.  Cell (i0,i1,i2) is the box [i s, (i + 1) s) per axis.  -> int64 tensor of `shape`:
    the highest 1 + m among the meshes with a triangle that intersects the cell, 0 if none; parts of a mesh outside the
    volume are dropped.  A face without area counts as its longest edge (or its point).  Bitwise reproducible."""
    packed, shape, spacing, dev = _pack_meshes("mesh_labelmap_cover", verts, faces, shape, spacing, validate)
    if packed is None:
        return torch.zeros(shape, dtype=torch.int64, device=dev)
    v, f, lab = packed
    out = torch.empty(shape, dtype=torch.int64, device=dev)
    launch(dev, "fsg_mesh_labelmap_cover_f32", _p(v), _p(f), _p(lab), v.shape[0], f.shape[0], *shape, *spacing, _p(out))
    return out
