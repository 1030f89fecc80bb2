"""Drop-in for the kNN part of the reference's utils/general_utils.py (:43-53, :315-327), its label map <-> point cloud helpers
and its mesh clean-up (:157-209: `mask_out_verts_from_mesh`, `remove_all_but_biggest_component`)."""
import numpy as np
import torch

from .. import functional as F_hip


def knn(x, k, self_loop=False, return_dist=False):
    """Same contract as utils/general_utils.py:315 -- x: (B,C,N) -> idx (B,N,k) int64, neighbours in
    ascending distance; `self_loop=False` selects k+1 and drops the first column (:317,:320-322).
    The (B,N,N) matrix of `pairwise_dist` is never materialised (fused in fsg_knn_dense_f32)."""
    out = F_hip.knn_graph(x, k, fix_diag=True, drop_first=not self_loop, return_dist=return_dist)
    if return_dist:
        return out[0].long(), out[1]
    return out.long()


def pairwise_dist(x):
    """utils/general_utils.py:43-53 for callers that really want the dense (B,N,N) matrix (none on the
    hot path).  Plain device-side torch ops; kept only for API completeness."""
    if not x.is_cuda:
        raise RuntimeError("GPU tensors only")
    sq = x.pow(2).sum(2, keepdim=True)
    d = sq - 2.0 * torch.bmm(x, x.transpose(1, 2)) + sq.transpose(1, 2)
    ar = torch.arange(x.shape[1], device=x.device)
    d[:, ar, ar] = 0
    return d


def farthest_point_sampling(kpts, num_points, start=None):
    """Drop-in for the pure-torch loop of dseg_ae_regularization.py:30-43 (used at :85 to pick the auto-encoder's input
    points of one object): `kpts (1,N,3)` -> `(kpts[:, ind, :], ind)` with `ind (num_points,) int64`.  The reference's
    `torch.argmax(dist)` runs over the flattened (B,N) distances, so it is only meaningful -- and only ever called -- with
    one cloud; B > 1 raises here.

    One `fsg_fps_f32` launch instead of `num_points` arg-max round trips.  The reference starts at a random point
    (`torch.randint(N, (1,))`); the kernel starts a segment at its first row, so the cloud is rotated to put the start
    there (`start` fixes it for tests).  Distances are the direct form (x-y)^2 as in the reference; ties (measure zero on
    real data) go to the first point after the start instead of the lowest index."""
    B, N, _ = kpts.size()
    if N <= num_points:
        if N < num_points:
            print(f'Tried to sample {num_points} from a point cloud with only {N}')
        return kpts, torch.arange(N)
    if B != 1:
        raise ValueError("farthest_point_sampling: one cloud at a time (the reference shares one index list and is "
                         "called with B = 1)")
    if not kpts.is_cuda:
        raise RuntimeError("farthest_point_sampling (HIP path) needs its input on the GPU")
    if start is None:
        start = int(torch.randint(N, (1,)))
    pts = torch.roll(kpts[0].to(torch.float32), -start, 0).contiguous()
    offset = torch.tensor([N], dtype=torch.int32, device=kpts.device)
    new_offset = torch.tensor([num_points], dtype=torch.int32, device=kpts.device)
    ind = (F_hip.fps(pts, offset, new_offset, num_points).long() + start) % N
    return kpts[:, ind, :], ind


def inverse_affine_transform(point_cloud, scaling, rotation_mat, affine_translation):
    """Same contract as utils/general_utils.py:299-312: undo p = scaling * rotation_mat @ x + affine_translation for every row
    of point_cloud (N, 3), numpy or torch (any device) -> (N, 3).  With the parameters the reference stores for a rigid
    pre-registration -- scale, rotation.T and translation of RigidRegistration (point_cloud_registration.py:236-237) -- this
    takes registered points back to the moving cloud's space."""
    centred = (point_cloud - affine_translation) / scaling          # rows: rotation_mat @ x
    linalg = torch.linalg if isinstance(centred, torch.Tensor) else np.linalg
    return linalg.solve(rotation_mat, centred.T).T                  # one 3 x 3 solve for all rows, no explicit inverse


# ------------------------------------------------------------------ label maps <-> point clouds (plain torch, any device)
def mask_to_points(mask, spacing=(1., 1., 1.)):
    """Same contract as utils/general_utils.py:151-154: the non-zero voxels of `mask` (D, H, W) as world points (N, 3) in
    (x, y, z): index, flipped, times `spacing` (given x, y, z).  On the device of the mask."""
    xyz = torch.nonzero(mask).flip(-1)
    return xyz * torch.tensor(spacing, device=mask.device)       # int64 x fp32 -> fp32, like the reference


def points_to_label_map(pts, labels, out_shape, spacing):
    """Same contract as utils/general_utils.py:212-233: world points (N, 3) in (x, y, z) with one label each -> (label map of
    `out_shape` (D, H, W) in the dtype of the labels, voxel index (N, 3) in (z, y, x) of every point): divide by `spacing`
    (x, y, z), flip, round, clamp into the volume, scatter (where points share a voxel, one of their labels stays).  On the
    device of the points."""
    zyx = (pts / torch.tensor(spacing, device=pts.device)).flip(-1).round().long()
    last = torch.tensor(tuple(out_shape), device=zyx.device) - 1
    zyx = torch.minimum(zyx.clamp_min(0), last)
    label_map = torch.zeros(tuple(out_shape), dtype=labels.dtype, device=labels.device)
    label_map[tuple(zyx.unbind(1))] = labels.reshape(-1)
    return label_map, zyx


# ------------------------------------------------------------------ voxel <-> grid coordinates, patches (plain torch, any device)
ALIGN_CORNERS = False


def _extent_xyz(shape, device):
    depth, height, width = shape
    return torch.tensor([width, height, depth], device=device)


def kpts_to_grid(kpts_world, shape, align_corners=None, return_transform=False):
    """Same contract as the reference's utils/general_utils.py: kpts_to_grid -- points (N, 3) in (x, y, z) voxel units of a
    volume with `shape` (D, H, W) -> torch grid coordinates: index 0 maps to -1 and index size - 1 to +1, and without
    `align_corners` the result is shrunk by (size - 1) / size so that voxel CENTRES sit where `grid_sample` expects them.
    `return_transform` would need pytorch3d's Transform3d, which this package does not depend on."""
    if return_transform:
        raise NotImplementedError("kpts_to_grid(return_transform=True) needs pytorch3d, which this package does not use")
    size = _extent_xyz(shape, kpts_world.device)
    grid = (kpts_world * (1 / (size - 1))) * 2 - 1
    if not align_corners:
        grid = grid * ((size - 1) / size)
    return grid


def kpts_to_world(kpts_pt, shape, align_corners=None):
    """the inverse of `kpts_to_grid`: grid coordinates (N, 3) in (x, y, z) -> voxel units of a volume with `shape` (D, H, W)"""
    size = _extent_xyz(shape, kpts_pt.device)
    if not align_corners:
        kpts_pt = kpts_pt / ((size - 1) / size)
    return ((kpts_pt + 1) / 2) * (size - 1)


def sample_patches_at_kpts(img: torch.Tensor, kpts_grid: torch.Tensor, patch_size: int):
    """Same contract as the reference's sample_patches_at_kpts: img (1, 1, D, H, W), kpts_grid (N, 3) grid coordinates
    (x, y, z) -> (1, N, p, p, p) with p = patch_size: a p^3 lattice of voxel-spaced samples centred on every keypoint, read by
    one `grid_sample` call (nearest for odd p, where the lattice falls on voxel centres; trilinear for even p; border
    padding)."""
    if bool(kpts_grid.min() < -1) or bool(kpts_grid.max() > 1):
        raise ValueError('sample_patches_at_kpts: keypoints outside [-1, 1] (expected torch grid coordinates, see kpts_to_grid)')
    if tuple(img.shape[:2]) != (1, 1):
        raise NotImplementedError(f'sample_patches_at_kpts: one single-channel volume at a time, got {tuple(img.shape)}')
    n, p = kpts_grid.shape[0], patch_size
    nn_f = torch.nn.functional
    # the identity lattice over [-1, 1]^3 with p samples per axis, scaled to p voxels of this volume
    lattice = nn_f.affine_grid(torch.eye(3, 4)[None], [1, 1, p, p, p], align_corners=ALIGN_CORNERS).to(img.device)
    lattice = lattice * (p / torch.tensor(tuple(img.shape[:1:-1]), device=img.device))
    grid = (lattice + kpts_grid.view(n, 1, 1, 1, 3)).reshape(1, n, p ** 3, 1, 3)
    out = nn_f.grid_sample(img, grid, mode='nearest' if p % 2 else 'bilinear', padding_mode='border', align_corners=ALIGN_CORNERS)
    return out.view(1, n, p, p, p)


# ------------------------------------------------------------------ mesh clean-up (csrc/mesh_cleanup.hip through functional)
def _as_meshes(mesh, who):
    """`mesh.Meshes`, a (verts, faces) pair or an object with .vertices / .triangles (open3d's TriangleMesh) -> Meshes; host
    arrays go to the current GPU"""
    from ..mesh import Meshes
    from ..metrics import _as_tensor, _mesh_raw
    if isinstance(mesh, Meshes):
        return mesh
    verts, faces = _mesh_raw(mesh)
    verts = _as_tensor(verts, torch.float32)
    return Meshes([verts], [_as_tensor(faces, torch.int32, verts.device)])


def mask_out_verts_from_mesh(mesh, mask, spacing):
    """utils/general_utils.py:157-168: drop the vertices of `mesh` (and the faces that name one) whose voxel
    floor(v / spacing), clamped from above into the volume, is not set in `mask` (D, H, W) bool; vertices in (x, y, z), spacing
    (sx, sy, sz), the mask indexed [z, y, x].

    The reference edits an open3d mesh IN PLACE and returns nothing; this takes a `fissure_segmentation_amd.mesh.Meshes` (a batch
    shares the mask) or one (verts, faces) pair and RETURNS the new `Meshes`.  A vertex with a negative coordinate is dropped,
    where the reference's negative index would wrap around to the far side of the volume."""
    if not torch.is_tensor(mask):
        mask = torch.as_tensor(np.asarray(mask))
    meshes = _as_meshes(mesh, "mask_out_verts_from_mesh")
    return F_hip.mesh_remove_vertices(meshes, mask=(mask != 0).to(meshes.device), spacing=spacing)


def remove_all_but_biggest_component(mesh, right=None, center_x=None):
    """utils/general_utils.py:171-209: keep only the edge-connected cluster of triangles with the largest area and drop the
    vertices nothing refers to any more.  With `right` and `center_x` both given, a cluster whose distinct-vertex mean lies on the
    wrong side of x = center_x (x > center_x when right, x < center_x when not right) takes part with the value -1 / area instead
    of its area, so the biggest of them still wins when no cluster is on the wanted side; the first maximum wins.

    Takes a `Meshes` or one (verts, faces) pair and RETURNS the new `Meshes` (the reference edits in place).  A batch applies the
    rule per mesh; `right` may be a sequence with one entry per mesh.  A mesh without vertices or faces comes back unchanged."""
    meshes = _as_meshes(mesh, "remove_all_but_biggest_component")
    B = len(meshes)
    nv, nf = meshes._nv, meshes._nf
    if not any(v and f for v, f in zip(nv, nf)):
        return meshes
    with torch.no_grad():
        clusters, _ = F_hip.mesh_face_components(meshes)
        area, num, vsum, counts = F_hip.mesh_component_stats(meshes, clusters)
        dev = area.device
        C = sum(counts)
        cluster_mesh = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts).to(dev), output_size=C)
        value = area
        if center_x is not None and right is not None:
            r = torch.as_tensor(right, dtype=torch.bool).to(dev).reshape(-1)
            if r.numel() not in (1, B):
                raise ValueError(f"right must be one bool or one per mesh ({B}), got {r.numel()}")
            r = r.expand(B)[cluster_mesh]
            cx = vsum[:, 0] / num
            wrong = torch.where(r, cx > float(center_x), cx < float(center_x))
            value = torch.where(wrong, -1 / area, area)
        first = torch.tensor([sum(counts[:m]) for m in range(B)]).to(dev)
        table = torch.full((B, max(counts)), float("-inf"), dtype=torch.float64, device=dev)
        table[cluster_mesh, torch.arange(C, device=dev) - first[cluster_mesh]] = value
        chosen = table.argmax(1)                                    # the first maximal value, like numpy's
        face_mesh = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(nf).to(dev), output_size=sum(nf))
        out = F_hip.mesh_remove_vertices(meshes, face_keep=clusters.long() == chosen[face_mesh], drop_unreferenced=True)
    if all(v and f for v, f in zip(nv, nf)):
        return out
    from ..mesh import Meshes
    keep_old = [not (v and f) for v, f in zip(nv, nf)]              # the reference returns early on these
    pick = lambda new, old: [o if k else n for n, o, k in zip(new, old, keep_old)]     # noqa: E731
    normals = None if meshes._normals is None else pick(out.verts_normals_list(), meshes.verts_normals_list())
    return Meshes(pick(out.verts_list(), meshes.verts_list()), pick(out.faces_list(), meshes.faces_list()), normals)
