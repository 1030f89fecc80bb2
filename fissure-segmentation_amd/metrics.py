"""Evaluation metrics with the reference's names, argument order and return conventions (metrics.py:11-153): surface
distances (ASSD, its standard deviation, Hausdorff, 95 % Hausdorff) between meshes and between a point cloud and a mesh, and
Dice / recall / precision of label maps.

Everything that measures a distance to a mesh rests on `functional.point_mesh_distance` (fsg_point_mesh_dist_f32), which
stands where the reference builds an open3d ray-casting scene on the CPU; distances between point clouds use
`functional.chamfer_nn`.  Those paths need a GPU (a CPU tensor is a RuntimeError, there is no fallback); the label-map
scores and `_symmetric_point_distances` are plain torch on whatever device their inputs are on.  Nothing here is
differentiable.

`label_mesh_assd` (metrics.py:45-55) starts from `utils.general_utils.mask_to_points`; the way back from meshes to label
maps, for `batch_dice`, is data_processing/surface_fitting.py and surface_fitting_optimization.py.

Not included under its name: `label_label_assd` (metrics.py:79-93), the distance between the point clouds of two label maps;
`functional.labelmap_distances` computes the same four numbers from a distance transform.
"""
import numpy as np
import torch

from . import functional as F_hip

QUANTILE_MAX_ELEMENTS = 16_000_000   # torch.quantile refuses larger inputs


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("fissure_segmentation_amd.metrics: surface distances run on the GPU only (no device found)")
    return torch.device("cuda", torch.cuda.current_device())


def _as_tensor(a, dtype, device=None):
    """tensors stay where they are (a CPU tensor is refused further down, like at every HIP entry point); array-likes --
    lists, numpy arrays, open3d's Vector3dVector -- are host data by nature and go to the current device"""
    if torch.is_tensor(a):
        return a.detach().to(dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype={torch.float32: np.float32, torch.int32: np.int32}[dtype])
                            ).to(device or _device())


def _mesh_raw(mesh):
    """(verts, faces) of a `(verts, faces)` pair or of an object with `.vertices` / `.triangles` (open3d's TriangleMesh, read
    through np.asarray), not yet moved anywhere"""
    if isinstance(mesh, (tuple, list)):
        return mesh
    return np.asarray(mesh.vertices), np.asarray(mesh.triangles)


def _mesh_arrays(mesh):
    """-> verts (V,3) fp32, faces (T,3) int32 on the device"""
    verts, faces = _mesh_raw(mesh)
    dev = next((t.device for t in (verts, faces) if torch.is_tensor(t)), None)
    return _as_tensor(verts, torch.float32, dev).reshape(-1, 3), _as_tensor(faces, torch.int32, dev).reshape(-1, 3)


def _is_empty(mesh):
    return any(len(part) == 0 for part in _mesh_raw(mesh))


def _quantile95(d):
    assert d.shape[-1] <= QUANTILE_MAX_ELEMENTS, \
        f"torch.quantile takes at most {QUANTILE_MAX_ELEMENTS} elements, got {d.shape[-1]} distances: use fewer points / samples"
    return torch.quantile(d, 0.95, dim=-1)


def _nan4():
    return (torch.tensor(float("nan")),) * 4


def point_surface_distance(query_points, trg_points, trg_tris):
    """Unsigned distance from N query points to a triangle mesh: (N,3), (V,3), (T,3) array-likes or tensors -> (N,) tensor
    on the device.  One kernel launch."""
    trg_points = trg_points if torch.is_tensor(trg_points) else _as_tensor(trg_points, torch.float32)
    dev = trg_points.device
    q, f = _as_tensor(query_points, torch.float32, dev), _as_tensor(trg_tris, torch.int32, dev)
    return F_hip.point_mesh_distance(q.reshape(1, -1, 3), trg_points.reshape(1, -1, 3), f.reshape(-1, 3))[0]


def _symmetric_point_distances(dist_points1, dist_points2):
    """the two directed distance sets -> (mean, std, Hausdorff, 95 % Hausdorff), each the average of the two directions;
    std is torch's default (unbiased)"""
    both = (dist_points1, dist_points2)
    return (sum(d.mean() for d in both) / 2, sum(d.std() for d in both) / 2, sum(d.max() for d in both) / 2,
            sum(_quantile95(d) for d in both) / 2)


def assd(mesh_x, mesh_y):
    """Symmetric surface distance between two meshes, measured from the vertices of each to the surface of the other.
    -> mean, standard deviation, Hausdorff, 95 % Hausdorff; four NaN tensors if a mesh has no vertices (or no faces)."""
    if _is_empty(mesh_x) or _is_empty(mesh_y):
        return _nan4()
    (vx, fx), (vy, fy) = _mesh_arrays(mesh_x), _mesh_arrays(mesh_y)
    return _symmetric_point_distances(point_surface_distance(vx, vy, fy), point_surface_distance(vy, vx, fx))


def batch_assd(verts_x, faces_x, verts_y, faces_y):
    """`assd` per mesh pair of a batch, then the batch mean of each of the four numbers.  verts (B,V,3), faces (B,T,3) or (T,3)
    shared by the batch.  Two launches for the whole batch; the per-mesh statistics are reduced on the device."""
    if 0 in (verts_x.shape[1], verts_y.shape[1], faces_x.shape[-2], faces_y.shape[-2]):
        return _nan4()
    dxy = F_hip.point_mesh_distance(verts_x, verts_y, faces_y)
    dyx = F_hip.point_mesh_distance(verts_y, verts_x, faces_x)
    stats = [(dxy.mean(1) + dyx.mean(1)) / 2, (dxy.std(1) + dyx.std(1)) / 2, (dxy.amax(1) + dyx.amax(1)) / 2,
             (_quantile95(dxy) + _quantile95(dyx)) / 2]
    return tuple(s.mean() for s in stats)


def sample_mesh_surface(verts, faces, n_samples, generator=None):
    """n_samples points uniform on the surface of a mesh: faces drawn in proportion to their area (with replacement), then
    uniform barycentric coordinates.  verts (V,3), faces (T,3) on the device -> (points (n,3), face index (n,))."""
    tri = verts[faces.long()]                                            # (T,3,3)
    area = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1)
    if not bool(area.sum() > 0):
        area = torch.ones_like(area)                                     # a mesh without any area: every face alike
    pick = torch.multinomial(area, n_samples, replacement=True, generator=generator)
    u = torch.rand(n_samples, 2, device=verts.device, generator=generator)
    r = u[:, 0].sqrt()
    w = torch.stack([1 - r, r * (1 - u[:, 1]), r * u[:, 1]], 1)          # uniform on the triangle
    return (tri[pick] * w[:, :, None]).sum(1), pick


def pseudo_symmetric_point_to_mesh_distance(points, mesh, n_samples=10 ** 6, generator=None):
    """Points -> mesh surface exactly (the point-to-mesh kernel); mesh -> points through `n_samples` surface samples and their
    nearest point (`functional.chamfer_nn`).  -> mean, standard deviation, Hausdorff, 95 % Hausdorff.  `generator`: a
    torch.Generator on the device of the mesh, for reproducible samples."""
    if _is_empty(mesh) or len(points) == 0:
        return _nan4()
    verts, faces = _mesh_arrays(mesh)
    pts = _as_tensor(points, torch.float32, verts.device).reshape(-1, 3)
    assert max(n_samples, len(pts)) <= QUANTILE_MAX_ELEMENTS, \
        f"torch.quantile takes at most {QUANTILE_MAX_ELEMENTS} elements: n_samples={n_samples}, {len(pts)} points"
    dist_pts_to_mesh = point_surface_distance(pts, verts, faces)
    samples, _ = sample_mesh_surface(verts.to(torch.float32), faces, n_samples, generator)
    with torch.no_grad():
        dist_mesh_to_points = F_hip.chamfer_nn(samples[None], pts[None].contiguous())[0][0].sqrt()
    return _symmetric_point_distances(dist_pts_to_mesh, dist_mesh_to_points)


def label_mesh_assd(labelmap, mesh, spacing=(1., 1., 1.), n_samples=10 ** 6, generator=None):
    """Surface distance between the foreground of a label map (D, H, W; every non-zero voxel, as the world point
    index[::-1] * spacing with `spacing` in (x, y, z)) and a mesh with vertices in (x, y, z).
    -> mean, standard deviation, Hausdorff, 95 % Hausdorff, and the (N, 3) points.  `n_samples` and `generator` go to
    `pseudo_symmetric_point_to_mesh_distance`.  The label map is a tensor on the GPU, like every tensor handed to a distance."""
    from .utils.general_utils import mask_to_points
    points = mask_to_points(labelmap, spacing)
    return (*pseudo_symmetric_point_to_mesh_distance(points, mesh, n_samples, generator), points)


def batch_dice(prediction, target, n_labels):
    """Dice per label, averaged over the batch: (B, ...) label maps -> (n_labels,) on the CPU"""
    pred, targ = prediction.flatten(start_dim=1), target.flatten(start_dim=1)
    labels = torch.arange(n_labels, device=pred.device).view(1, -1, 1)
    p, t = pred[:, None, :] == labels, targ[:, None, :] == labels       # (B, n_labels, N)
    dice = 2 * (p & t).sum(-1) / (p.sum(-1) + t.sum(-1) + 1e-8)
    return dice.to(torch.float32).mean(0).cpu()


def _foreground_overlap(prediction, target):
    p, t = (prediction != 0).flatten(start_dim=1), (target != 0).flatten(start_dim=1)
    return (p & t).sum(-1), p.sum(-1), t.sum(-1)


def binary_recall(prediction, target):
    """per item: foreground of the target that the prediction also marks"""
    hit, _, n_targ = _foreground_overlap(prediction, target)
    return (hit + 1e-8) / (n_targ + 1e-8)


def binary_precision(prediction, target):
    """per item: foreground of the prediction that the target also marks"""
    hit, n_pred, _ = _foreground_overlap(prediction, target)
    return (hit + 1e-8) / (n_pred + 1e-8)
