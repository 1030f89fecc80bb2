"""Corresponding-point shapes from registered clouds: `data_set_correspondences` of the reference's
shape_model/generate_corresponding_points.py (:28-178), the step between the CPD registrations (point_cloud_registration.py) and
`SSM.fit`.

For every object (a fissure or a lobe) a set of sampling locations is chosen -- the fixed cloud ('simple', the reference's
command-line default), the centres of a k-means over the pooled moved clouds of all instances ('kmeans') or the means of the
OPTICS clusters of that pool ('cluster', the function's own default) --, each instance's
displacement field is interpolated there from its MOVED cloud and subtracted, the affine pre-registration is undone, and the
result is scored against the instance's mesh and moving cloud.

The reference runs this as a Python double loop (objects x instances: one kNN interpolation, one open3d point-to-mesh query and
one pytorch3d Chamfer call per pair) and clusters with sklearn on the CPU.  Here every object is ONE call of each of
`interpolate_displacements_weighted_knn` (or, with interpolation_mode='tps', `interpolate_displacements_tps`: one batched spline
fit and one fused sampling kernel, csrc/tps.hip), `inverse_affine_transform_batch`, `functional.point_mesh_distance` and
`functional.chamfer_nn` over all its instances, 'kmeans' is one `functional.kmeans` over all objects (csrc/kmeans.hip) and
'cluster' one `functional.optics` over all objects with a radius per object (csrc/optics.hip), followed by the xi extraction and
the cluster means on the host (shape_model/optics.py).

Kept from the reference: the displacements are interpolated from the moved cloud; the evaluation always uses the cloud with the
affine pre-registration undone, whatever `undo_affine_reg` says; `std` is torch's unbiased one; labels are object index + 1;
every transform dict gets ['is_applied'] = not undo_affine_reg; 'parzen' raises NotImplementedError, an unknown mode ValueError.
Different: 'kmeans' is seeded by farthest point sampling instead of k-means++ on numpy's random stream and an emptied cluster
keeps its centre (see functional.kmeans) -- deterministic, but not sklearn's centres; `plot_dir` and `show` are accepted and
ignored (no matplotlib); 'cluster' follows the rule of functional.optics (sklearn's OPTICS without its rounding of the
distances to 15 decimals, compared on squares; labels equal sklearn's on the tested inputs), gives as many centroids as there are
clusters (the reference allocates `len(np.unique(labels)) - 1` rows and so fails when OPTICS leaves no outlier), raises
ValueError for an object without any cluster and for min_samples = instances // optics_minsamples_divisor outside 2 .. n, and
NotImplementedError for optics_minsamples_divisor < 1 (the default -1 hands sklearn a negative min_samples, which it rejects:
pass a positive divisor, the reference's driver passes 16); in that mode the objects differ in their point counts; 'tps' needs
`fixed_img_shape` = (D, H, W) and raises NotImplementedError without it (the reference fails there as well; a grid-free spline is
out of scope); the file-reading `__main__` driver is not mirrored.

numpy arrays in give numpy arrays out, with the evaluation as CPU tensors, as in the reference (the work still runs on the current
GPU); GPU tensors in give GPU tensors out."""
import numpy as np
import torch

from .. import functional as F_hip
from ..metrics import _device, _mesh_arrays
from .optics import cluster_means, optics_xi_labels
from .point_cloud_registration import (INTERPOLATION_MODES, TPS_NEEDS_SHAPE, interpolate_displacements_tps,
                                       interpolate_displacements_weighted_knn)

CORRESPONDENCE_MODES = ["kmeans", "cluster", "simple"]


def _det3(m):
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1])
            - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def inverse_affine_transform_batch(point_clouds, scaling, rotation_mats, affine_translations):
    """`utils.general_utils.inverse_affine_transform` for a batch: undo p = scaling_i * rotation_i @ x + translation_i for the
    rows of point_clouds (I,N,3), with scaling (I,), rotation_mats (I,3,3), affine_translations (I,3), torch tensors on one
    device -> (I,N,3).  The 3 x 3 systems are solved in closed form (adjugate over determinant, Cramer's rule) with element-wise
    operations only: an instance's result has the same bits alone and inside a batch, which a batched library solve does not
    promise.  Meant for the well-conditioned matrices of a rigid pre-registration."""
    centred = (point_clouds - affine_translations[:, None, :]) / scaling[:, None, None]
    R = rotation_mats
    det = _det3(R)[:, None]
    r = [centred[..., k] for k in range(3)]
    cols = []
    for j in range(3):   # x_j = sum_k cofactor(k, j) r_k / det
        j1, j2 = (j + 1) % 3, (j + 2) % 3
        cof = [(R[:, (k + 1) % 3, j1] * R[:, (k + 2) % 3, j2] - R[:, (k + 1) % 3, j2] * R[:, (k + 2) % 3, j1])[:, None]
               for k in range(3)]
        cols.append(((cof[0] * r[0] + cof[1] * r[1]) + cof[2] * r[2]) / det)
    return torch.stack(cols, -1)


def _clouds(a, name, ndim, as_numpy, dev):
    """an array (.., P, 3) with `ndim` axes -> tensor on the device in its own floating dtype"""
    if as_numpy:
        a = np.asarray(a)
        if a.dtype == object:
            raise ValueError(f"{name}: every instance and object must hold the same number of points (got a ragged array)")
        a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    elif not torch.is_tensor(a):
        raise TypeError(f"{name} must be a torch tensor like the other inputs, got {type(a).__name__}")
    else:
        F_hip._need_gpu(a)
    if a.dim() != ndim or a.shape[-1] != 3 or not a.is_floating_point():
        raise ValueError(f"{name} must be a floating-point array with {ndim} axes ending in 3, got {tuple(a.shape)} {a.dtype}")
    return a


def _transforms(all_prereg_transforms, instances, dev):
    """the dicts of the rigid pre-registration -> scale (I,), rotation (I,3,3), translation (I,3) in fp64 on the device"""
    if len(all_prereg_transforms) != instances:
        raise ValueError(f"{len(all_prereg_transforms)} pre-registration transforms for {instances} instances")
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)   # noqa: E731
    s = np.array([float(host(t['scale'])) for t in all_prereg_transforms], np.float64)
    R = np.stack([host(t['rotation']).astype(np.float64).reshape(3, 3) for t in all_prereg_transforms])
    tr = np.stack([host(t['translation']).astype(np.float64).reshape(3) for t in all_prereg_transforms])
    return tuple(torch.from_numpy(a).to(dev) for a in (s, R, tr))


def _mesh_distances(points, meshes):
    """points (I,Q,3) and one mesh per instance -> distances (I,Q) fp32.  One launch when the meshes have equal vertex and
    face counts; otherwise one launch per mesh (the sizes differ, the points do not)."""
    arrays = [_mesh_arrays(m) for m in meshes]
    dev = points.device
    arrays = [(v.to(dev), f.to(dev)) for v, f in arrays]
    if len({(v.shape[0], f.shape[0]) for v, f in arrays}) == 1:
        return F_hip.point_mesh_distance(points, torch.stack([v for v, _ in arrays]), torch.stack([f for _, f in arrays]))
    return torch.cat([F_hip.point_mesh_distance(points[i:i + 1], v[None], f) for i, (v, f) in enumerate(arrays)])


def object_correspondences(centroids, moved, displacements, moving, meshes, scale, rotation, translation, undo_affine_reg=True,
                           interpolation_mode='knn', img_shape=None, tps_solver='lu'):
    """One object, all instances at once: centroids (Q,3) the sampling locations, moved / displacements (I,P,3) the registered
    clouds and their displacements, moving (I,Pm,3) the original clouds, one mesh per instance, the pre-registration as
    scale (I,), rotation (I,3,3), translation (I,3) -> (corresponding points (I,Q,3) in the dtype of the centroids, mean, std,
    hd, cf (I,) fp32).  GPU tensors.  interpolation_mode 'tps' needs img_shape = (D, H, W); tps_solver is the solve of its fit
    (point_cloud_registration.TPS_SOLVERS)."""
    I = moved.shape[0]
    sample = centroids[None].expand(I, -1, -1).contiguous()
    if interpolation_mode == 'tps':
        if img_shape is None:
            raise NotImplementedError(TPS_NEEDS_SHAPE.format("object_correspondences", "img_shape"))
        interpolated = interpolate_displacements_tps(moved.float(), displacements.float(), sample.float(), img_shape,
                                                     solver=tps_solver)
    elif interpolation_mode == 'knn':
        interpolated = interpolate_displacements_weighted_knn(moved.float(), displacements.float(), sample.float())
    else:
        raise ValueError(f"interpolation_mode must be one of {INTERPOLATION_MODES}, got {interpolation_mode!r}")
    sampled = sample - interpolated.to(sample.dtype)
    not_affine = inverse_affine_transform_batch(sampled.double(), scale, rotation, translation).to(sample.dtype)
    dist = _mesh_distances(not_affine.float(), meshes).double()
    d_xy, _ = F_hip.chamfer_nn(not_affine.float(), moving.float())
    d_yx, _ = F_hip.chamfer_nn(moving.float(), not_affine.float())
    cf = d_xy.double().mean(1) + d_yx.double().mean(1)       # pytorch3d's chamfer_distance of one pair, for every pair
    std = dist.std(1) if dist.shape[1] > 1 else torch.full_like(dist[:, 0], float("nan"))
    pcs = not_affine if undo_affine_reg else sampled
    return pcs, dist.mean(1).float(), std.float(), dist.max(1).values.float(), cf.float()


def _optics_centroids(moved, min_samples):
    """'cluster' (:50-62): moved (I,O,P,3) -> one (C_obj,3) tensor per object in the dtype of `moved`: the cluster means of an
    OPTICS run over the object's pooled clouds with max_eps = 5 % of the range of all its coordinates.  ONE ordering launch
    for all objects; the xi labels and the means are taken per object on the host (shape_model/optics.py)."""
    I, O, P, _ = moved.shape
    n = I * P
    if not 2 <= min_samples <= n:
        raise ValueError(f"data_set_correspondences(mode='cluster'): min_samples = instances // optics_minsamples_divisor = "
                         f"{min_samples} must be in 2 .. {n} (instances * points), as sklearn's OPTICS demands")
    pool = moved.transpose(0, 1).reshape(O, n, 3)
    flat = pool.reshape(O, -1).double()
    eps = (flat.max(1).values - flat.min(1).values) * 0.05
    ordering, _, reach2, pred = F_hip.optics(pool, min_samples, eps, return_squared=True)
    ordering, reach, pred, host = ordering.cpu().numpy(), np.sqrt(reach2.cpu().numpy()), pred.cpu().numpy(), pool.float().cpu().numpy()
    centroids = []
    for obj in range(O):
        labels = optics_xi_labels(reach[obj], pred[obj], ordering[obj], min_samples)
        if labels.max() < 0:
            raise ValueError(f"data_set_correspondences(mode='cluster'): OPTICS found no cluster in object {obj + 1} "
                             f"(min_samples={min_samples}, max_eps={float(eps[obj]):.6g})")
        centroids.append(torch.from_numpy(cluster_means(host[obj], labels)).to(device=moved.device, dtype=moved.dtype))
    return centroids


def data_set_correspondences(fixed_pcs, all_moving_meshes, all_moving_pcs, all_prereg_transforms, all_moved_pcs,
                             all_displacements, fixed_img_shape=None, plot_dir=None,
                             mode='cluster', undo_affine_reg=True, show=True, optics_minsamples_divisor=-1,
                             interpolation_mode='knn', tps_solver='lu'):
    """generate_corresponding_points.py:28-178.  fixed_pcs (objects, P, 3); all_moving_meshes[instance][object] a mesh in any
    form `metrics._mesh_arrays` takes; all_moving_pcs, all_moved_pcs, all_displacements (instances, objects, P, 3);
    all_prereg_transforms one dict per instance with 'scale', 'rotation', 'translation' ->
    (corresponding_pcs (instances, sum of points, 3), all_prereg_transforms, corresponding_fixed_pc (sum of points, 3),
    labels (sum of points,), {'mean', 'std', 'hd', 'cf'} each (instances, objects) fp32).  fixed_img_shape = (D, H, W) is read by
    interpolation_mode='tps' only, and so is tps_solver, the solve of the spline's fit (point_cloud_registration.TPS_SOLVERS)."""
    if mode == 'parzen':
        raise NotImplementedError('Parzen mode is unfinished')
    if mode == 'cluster' and (isinstance(optics_minsamples_divisor, bool) or not isinstance(optics_minsamples_divisor, int)
                              or optics_minsamples_divisor < 1):
        raise NotImplementedError(f"data_set_correspondences(mode='cluster'): OPTICS needs min_samples = instances // "
                                  f"optics_minsamples_divisor >= 2, and optics_minsamples_divisor={optics_minsamples_divisor!r} "
                                  f"gives none (the reference hands sklearn a negative min_samples here, which it rejects); "
                                  f"pass a positive divisor (the reference's driver passes 16)")
    if mode not in CORRESPONDENCE_MODES:
        raise ValueError(f'No mode named {mode}.')
    if interpolation_mode not in INTERPOLATION_MODES:
        raise ValueError(f"interpolation_mode must be one of {INTERPOLATION_MODES}, got {interpolation_mode!r}")
    if interpolation_mode == 'tps' and fixed_img_shape is None:
        raise NotImplementedError(TPS_NEEDS_SHAPE.format("data_set_correspondences", "fixed_img_shape"))
    as_numpy = not torch.is_tensor(all_moved_pcs)
    dev = _device() if as_numpy else all_moved_pcs.device
    moved = _clouds(all_moved_pcs, "all_moved_pcs", 4, as_numpy, dev)
    disp = _clouds(all_displacements, "all_displacements", 4, as_numpy, dev)
    moving = _clouds(all_moving_pcs, "all_moving_pcs", 4, as_numpy, dev)
    fixed = _clouds(fixed_pcs, "fixed_pcs", 3, as_numpy, dev)
    I, O, P, _ = moved.shape
    if disp.shape != moved.shape or moving.shape[:2] != (I, O) or fixed.shape[0] != O:
        raise ValueError(f"all_moved_pcs {tuple(moved.shape)}, all_displacements {tuple(disp.shape)}, all_moving_pcs "
                         f"{tuple(moving.shape)} and fixed_pcs {tuple(fixed.shape)} do not describe the same instances and objects")
    if len(all_moving_meshes) != I or any(len(m) != O for m in all_moving_meshes):
        raise ValueError(f"all_moving_meshes must hold {O} meshes for each of the {I} instances")
    with torch.no_grad():
        scale, rotation, translation = _transforms(all_prereg_transforms, I, dev)
        if mode == 'kmeans':
            # the moved clouds of all instances pooled per object, n_clusters = P: one batched run for all objects
            pool = moved.transpose(0, 1).reshape(O, I * P, 3)
            centroids = F_hip.kmeans(pool, n_clusters=P, init='fps')[0].to(moved.dtype)
        elif mode == 'cluster':
            centroids = _optics_centroids(moved, I // optics_minsamples_divisor)
        else:
            centroids = fixed
        pcs, evaluation = [], []
        for obj in range(O):
            out = object_correspondences(centroids[obj], moved[:, obj], disp[:, obj], moving[:, obj],
                                         [all_moving_meshes[i][obj] for i in range(I)], scale, rotation, translation,
                                         undo_affine_reg, interpolation_mode, fixed_img_shape, tps_solver)
            pcs.append(out[0])
            evaluation.append(out[1:])
        for t in all_prereg_transforms:
            t['is_applied'] = not undo_affine_reg
        corresponding_pcs = torch.cat(pcs, 1)
        corresponding_fixed_pc = torch.cat(list(centroids))   # a list in 'cluster' mode: the objects differ in their counts
        labels = torch.cat([torch.full((len(centroids[obj]),), obj + 1, dtype=torch.int64, device=dev) for obj in range(O)])
        evaluation = {k: torch.stack([e[j] for e in evaluation], 1) for j, k in enumerate(('mean', 'std', 'hd', 'cf'))}
    if as_numpy:
        return corresponding_pcs.cpu().numpy(), all_prereg_transforms, corresponding_fixed_pc.cpu().numpy(), \
            labels.cpu().numpy(), {k: v.cpu() for k, v in evaluation.items()}
    return corresponding_pcs, all_prereg_transforms, corresponding_fixed_pc, labels, evaluation
