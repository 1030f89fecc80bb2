"""Point-cloud normals and frames (csrc/pcl_normals.hip); surface fitting: orientation, mesh clean-up (csrc/mesh_cleanup.hip)."""
import torch

from .. import _lib
from .._launch import _f32c, _need_gpu, _p, _stream, launch
from .packed import knn_segment


# ------------------------------------------------------------------ point-cloud normals (csrc/pcl_normals.hip)
def _neighborhood_size(neighborhood_size):
    K = int(neighborhood_size)
    if not 2 <= K <= _lib.PCL_NORMALS_MAX_K:
        raise ValueError(f"neighborhood_size must be in 2..{_lib.PCL_NORMALS_MAX_K}, got {neighborhood_size}")
    return K


def _check_neighbours(idx, off, n, K):
    """the host-side look at a caller's neighbour lists (one synchronisation): the offsets end at n and do not decrease, and
    every column the kernel reads (the first k_s of a row) names a point of the row's own segment"""
    rows = torch.arange(n, device=idx.device)
    seg = torch.searchsorted(off, rows.to(torch.int32), right=True).clamp_(max=off.shape[0] - 1)
    en = off[seg].long()
    st = torch.where(seg > 0, off[(seg - 1).clamp_(min=0)].long(), torch.zeros_like(en))
    ks = (en - st - 1).clamp_(min=1, max=K)
    read = torch.arange(K, device=idx.device)[None] < ks[:, None]
    i = idx.long()
    bad_idx = (read & ((i < st[:, None]) | (i >= en[:, None]))).any()
    bad_off = (off[-1] != n) | (off[0] < 0) | (off[1:] < off[:-1]).any()
    bad_idx, bad_off = torch.stack([bad_idx, bad_off]).tolist()
    if bad_off:
        raise ValueError(f"offset must be non-decreasing cumulative segment ends finishing at n = {n}")
    if bad_idx:
        raise ValueError("idx holds an index outside its row's segment (or outside the cloud) in a column that is read")


def _pcl_normals_raw(xyz, off, K, disambiguate, idx, want_frames):
    """xyz (n, 3) fp32 contiguous, off (b) int32, idx (n, K) int32 -> normals (n, 3), curvatures (n, 3), frames (n, 3, 3) | None"""
    n = xyz.shape[0]
    normals = torch.empty(n, 3, dtype=torch.float32, device=xyz.device)
    curv = torch.empty(n, 3, dtype=torch.float32, device=xyz.device)
    frames = torch.empty(n, 3, 3, dtype=torch.float32, device=xyz.device) if want_frames else None
    launch(xyz.device, "fsg_pcl_normals_f32", _p(xyz), _p(idx), _p(off), off.shape[0], n, K, int(bool(disambiguate)), _p(normals),
           _p(curv), _p(frames))
    return normals, curv, frames


def _pcl_packed(xyz, offset, neighborhood_size, disambiguate_directions, idx, validate, want_frames):
    K = _neighborhood_size(neighborhood_size)
    if not torch.is_tensor(xyz) or not xyz.is_floating_point() or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"expected packed points xyz (n, 3), got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    if not torch.is_tensor(offset) or offset.is_floating_point() or offset.dim() != 1 or offset.shape[0] < 1:
        raise ValueError("offset must be a 1-D integer tensor of cumulative segment ends")
    _need_gpu(xyz, offset, idx)
    with torch.no_grad():
        x, off = _f32c(xyz), offset.to(torch.int32).contiguous()
        n = x.shape[0]
        if idx is None:
            idx = knn_segment(K, x, x, off, off)[0] if n else torch.empty(0, K, dtype=torch.int32, device=x.device)
        else:
            if not torch.is_tensor(idx) or idx.is_floating_point() or idx.dtype == torch.bool or tuple(idx.shape) != (n, K):
                raise ValueError(f"idx must be an integer tensor of shape ({n}, {K}): the first neighborhood_size columns of "
                                 f"knn_segment's lists")
            idx = idx.to(torch.int32).contiguous()
            if validate and n:
                _check_neighbours(idx, off, n, K)
        return _pcl_normals_raw(x, off, K, disambiguate_directions, idx, want_frames)


def pointcloud_frames_packed(xyz, offset, neighborhood_size, disambiguate_directions=True, idx=None, validate=True):
    """The local PCA frame of every point of a packed cloud (fsg_pcl_normals_f32): xyz (n, 3), offset (b,) cumulative segment
    ends -> curvatures (n, 3), the eigenvalues of the neighbourhood covariance in ascending order, and frames (n, 3, 3) whose
    COLUMNS are (normal, y, z): the eigenvector of the smallest eigenvalue, z x normal, the eigenvector of the largest.

    Per point: the k nearest points of its own segment, itself included; C = mean of (x_j - mean)(x_j - mean)^T over them.  A
    segment of n_s points uses k_s = min(neighborhood_size, n_s - 1) (at least 1): a short segment gets a smaller neighbourhood
    instead of an error.  With disambiguate_directions a vector v is negated when fewer than half of the k neighbours have
    v . (x_j - p) > 0 (applied to the normal and to z); on a convex surface this points the normals INWARDS, as pytorch3d's
    rule does.  Parity with pytorch3d is unpinned (restated, not compared).

    idx (n, neighborhood_size): neighbour lists in knn_segment's layout (ascending distance, self first, indices into xyz);
    without it knn_segment runs (queries = the points).  Only the first k_s columns of a row are read.  validate=True checks a
    given idx (and the offsets) on the host, one synchronisation: an index outside the row's segment raises ValueError; with
    validate=False a bad index is clamped into the cloud by the kernel and gives a wrong frame, not a fault.
    neighborhood_size outside 2..64 raises ValueError.  No autograd: the outputs are constants (detached), as the reference
    uses them.  Deterministic: the same input gives the same bits."""
    _, curv, frames = _pcl_packed(xyz, offset, neighborhood_size, disambiguate_directions, idx, validate, True)
    return curv, frames


def _dense_cloud(pointclouds, neighborhood_size):
    K = _neighborhood_size(neighborhood_size)
    if not torch.is_tensor(pointclouds) or pointclouds.dim() != 3 or pointclouds.shape[2] != 3:
        raise ValueError(f"expected pointclouds (B, N, 3), got "
                         f"{tuple(pointclouds.shape) if torch.is_tensor(pointclouds) else type(pointclouds).__name__}")
    B, N, _ = pointclouds.shape
    if K >= N:
        raise ValueError(f"neighborhood_size ({K}) must be smaller than the number of points per cloud ({N})")
    _need_gpu(pointclouds)
    offset = torch.arange(1, B + 1, dtype=torch.int32, device=pointclouds.device) * N
    return K, B, N, offset


def estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=50, disambiguate_directions=True):
    """pytorch3d.ops.estimate_pointcloud_local_coord_frames for a (B, N, 3) tensor -> curvatures (B, N, 3), local_coord_frames
    (B, N, 3, 3); see pointcloud_frames_packed (every cloud is one segment).  2 <= neighborhood_size <= 64 and < N."""
    K, B, N, offset = _dense_cloud(pointclouds, neighborhood_size)
    _, curv, frames = _pcl_packed(pointclouds.reshape(B * N, 3), offset, K, disambiguate_directions, None, False, True)
    return curv.view(B, N, 3), frames.view(B, N, 3, 3)


def estimate_pointcloud_normals(pointclouds, neighborhood_size=50, disambiguate_directions=True):
    """pytorch3d.ops.estimate_pointcloud_normals for a (B, N, 3) tensor -> normals (B, N, 3), the first column of the frames of
    estimate_pointcloud_local_coord_frames (the same bits).  Constants: no gradient reaches the points."""
    K, B, N, offset = _dense_cloud(pointclouds, neighborhood_size)
    normals, _, _ = _pcl_packed(pointclouds.reshape(B * N, 3), offset, K, disambiguate_directions, None, False, False)
    return normals.view(B, N, 3)


# ------------------------------------------------------------------ surface fitting: orientation, mesh clean-up (csrc/mesh_cleanup.hip)
def orient_normals_consistent(xyz, normals, offset, k, idx=None):
    """Globally consistent signs for the normals of a packed cloud (fsg_orient_normals_f32), what open3d's
    orient_normals_consistent_tangent_plane does for data_processing/surface_fitting.py:64.

    xyz, normals (n, 3), offset (b,) cumulative segment ends, 2 <= k <= 64; idx (n, k): neighbour lists in knn_segment's layout
    (self first), built here when None.  Per segment the graph {u, idx[u, j]}, 1 <= j < min(k, n_s - 1), weighted by
    1 - |n_u . n_v|, gets its minimum spanning forest (Boruvka rounds on the device) and the signs are carried along it.  Per
    connected component the member of largest z (lowest index on ties) ends with n_z >= 0.  The graph is NOT connected by extra
    Euclidean edges as open3d does: every component is oriented on its own.
    -> oriented (n, 3) fp32 = normals with the sign flipped or not, signs (n,) int8 (+1 / -1), component (n,) int32: the smallest
    member of the point's component.  No host read; bitwise reproducible; a segment gives the same bits alone and in a batch.
    At most 2^20 points per call.  Not differentiable."""
    k = _neighborhood_size(k)
    if not torch.is_tensor(xyz) or not xyz.is_floating_point() or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"expected packed points xyz (n, 3), got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    if not torch.is_tensor(normals) or not normals.is_floating_point() or normals.shape != xyz.shape:
        raise ValueError(f"normals must be a floating-point tensor of the shape of xyz {tuple(xyz.shape)}")
    if not torch.is_tensor(offset) or offset.is_floating_point() or offset.dim() != 1 or offset.shape[0] < 1:
        raise ValueError("offset must be a 1-D integer tensor of cumulative segment ends")
    n = xyz.shape[0]
    if n > _lib.ORIENT_MAX_POINTS:
        raise ValueError(f"orient_normals_consistent: {n} points, at most {_lib.ORIENT_MAX_POINTS} per call (20 bits per endpoint "
                         f"in the edge key)")
    _need_gpu(xyz, normals, offset, idx)
    with torch.no_grad():
        x, nr, off = _f32c(xyz), _f32c(normals), offset.to(torch.int32).contiguous()
        dev = x.device
        out = torch.empty(n, 3, dtype=torch.float32, device=dev)
        signs = torch.empty(n, dtype=torch.int8, device=dev)
        comp = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return out, signs, comp
        if idx is None:
            idx = knn_segment(k, x, x, off, off)[0]
        else:
            if not torch.is_tensor(idx) or idx.is_floating_point() or idx.dtype == torch.bool or tuple(idx.shape) != (n, k):
                raise ValueError(f"idx must be an integer tensor of shape ({n}, {k}): knn_segment's lists")
            idx = idx.to(torch.int32).contiguous()
        with torch.cuda.device(dev):
            ws = _lib.workspace("fsg_orient_normals", n, k, device=dev)
            _lib.call("fsg_orient_normals_f32", _p(x), _p(nr), _p(idx), _p(off), off.shape[0], n, k, _p(ws), ws.numel(), _p(out),
                      _p(signs), _p(comp), _stream())
    return out, signs, comp


class _PackedMeshes:
    """the meshes of one call packed for csrc/mesh_cleanup.hip: verts (V, 3) fp32, faces (F, 3) int32 into verts, normals or None,
    the first vertex / face of every mesh as host lists and as int32 / int64 device tensors (B + 1), the mesh of every face"""

    def __init__(self, who, meshes):
        if hasattr(meshes, "verts_list") and hasattr(meshes, "faces_list"):
            vl, fl = meshes.verts_list(), meshes.faces_list()
            nl = meshes.verts_normals_list() if getattr(meshes, "_normals", None) is not None else None
        elif isinstance(meshes, (tuple, list)) and len(meshes) == 2 and torch.is_tensor(meshes[0]) and torch.is_tensor(meshes[1]):
            vl, fl, nl = [meshes[0]], [meshes[1]], None
        else:
            raise TypeError(f"{who}: expected fissure_segmentation_amd.mesh.Meshes or one (verts, faces) pair, got "
                            f"{type(meshes).__name__}")
        if not vl:
            raise ValueError(f"{who}: empty batch of meshes")
        for m, (v, f) in enumerate(zip(vl, fl)):
            if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or not v.is_floating_point():
                raise ValueError(f"{who}: mesh {m}: expected verts (V,3) and faces (F,3), got {tuple(v.shape)} and {tuple(f.shape)}")
            if f.is_floating_point() or f.dtype == torch.bool:
                raise ValueError(f"{who}: mesh {m}: faces must hold integer vertex indices, got {f.dtype}")
        _need_gpu(*vl, *fl)
        self.B, self.dev = len(vl), vl[0].device
        self.nv, self.nf = [v.shape[0] for v in vl], [f.shape[0] for f in fl]
        self.voff, self.foff = [0], [0]
        for a, b in zip(self.nv, self.nf):
            self.voff.append(self.voff[-1] + a)
            self.foff.append(self.foff[-1] + b)
        self.V, self.F = self.voff[-1], self.foff[-1]
        if max(self.V, 3 * self.F) >= 2 ** 31:
            raise ValueError(f"{who}: the batch has 2^31 or more vertices or half-edges")
        self.verts = torch.cat([_f32c(v) for v in vl])
        self.faces = torch.cat([f.detach().to(torch.int32) + b for f, b in zip(fl, self.voff)]).contiguous()
        self.normals = None if nl is None else torch.cat([_f32c(x) for x in nl])
        self.voff_t = torch.tensor(self.voff, dtype=torch.int32).to(self.dev)
        self.foff_t = torch.tensor(self.foff, dtype=torch.int64).to(self.dev)
        self.face_mesh = torch.repeat_interleave(torch.arange(self.B, device=self.dev), torch.tensor(self.nf).to(self.dev),
                                                 output_size=self.F)


def _face_components(pk):
    """-> clusters (F,) int32 local to the mesh, counts (B,) int64, both on the device; no host read"""
    dev, F = pk.dev, pk.F
    if F == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(pk.B, dtype=torch.int64, device=dev)
    f = pk.faces.long()
    a, b = f, f.roll(-1, 1)                                                  # half-edge 3 f + e = (f[e], f[e + 1])
    keys, half_edge = torch.sort((torch.minimum(a, b) * pk.V + torch.maximum(a, b)).reshape(-1))
    parent = torch.empty(F, dtype=torch.int32, device=dev)
    root = torch.empty(F, dtype=torch.int32, device=dev)
    launch(dev, "fsg_face_union_i32", _p(keys), _p(half_edge), F, _p(parent), _p(root))
    is_root = (root == torch.arange(F, dtype=torch.int32, device=dev)).long()
    before = torch.cumsum(is_root, 0)                                        # roots up to and including f
    before = torch.cat([before.new_zeros(1), before])                        # [f]: roots before face f
    start = before[pk.foff_t]                                                # roots before the first face of every mesh
    clusters = (before[root.long()] - start[pk.face_mesh]).to(torch.int32)
    return clusters, start[1:] - start[:-1]


def mesh_face_components(meshes):
    """Edge-connected components of the triangles of a batch of meshes (fsg_face_union_i32), open3d's cluster_connected_triangles
    as utils/general_utils.py:177 calls it: two faces are adjacent iff they share an edge (the same unordered vertex pair);
    sharing only a vertex does not connect them, and an edge with more than two faces links all of them.

    meshes: `mesh.Meshes` or one (verts, faces) pair -> clusters (sum F,) int32, the cluster of every face within ITS mesh, the
    clusters of a mesh numbered 0 .. c - 1 in ascending order of their smallest face; counts (B,) int64 on the device.  The 3F
    edge keys are paired by torch.sort, the union is the kernel, the numbering a prefix sum.  No host read."""
    with torch.no_grad():
        return _face_components(_PackedMeshes("mesh_face_components", meshes))


def _check_clusters(who, pk, clusters):
    if not torch.is_tensor(clusters) or clusters.is_floating_point() or clusters.dtype == torch.bool or tuple(clusters.shape) != (pk.F,):
        raise ValueError(f"{who}: clusters must be an integer tensor of shape ({pk.F},), one entry per face of the batch")
    _need_gpu(clusters)
    return clusters.to(torch.int32)


def mesh_component_stats(meshes, clusters):
    """Area, number of distinct vertices and their coordinate sum for every face cluster of a batch (fsg_cluster_stats_f64), what
    utils/general_utils.py:177-195 takes from open3d's cluster_area and np.unique / np.mean.

    clusters (sum F,): `mesh_face_components`' numbers.  -> area (C,) fp64, num_verts (C,) int64, vert_sum (C, 3) fp64 with the
    clusters of mesh 0 first, then mesh 1's, ..., and counts: a list of B ints (C = their sum; one host read).  A vertex that two
    clusters touch counts in both.  Sums are fp64 in a fixed order: bitwise reproducible."""
    with torch.no_grad():
        pk = _PackedMeshes("mesh_component_stats", meshes)
        cl = _check_clusters("mesh_component_stats", pk, clusters)
        dev = pk.dev
        if pk.F == 0:
            return (torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                    torch.zeros(0, 3, dtype=torch.float64, device=dev), [0] * pk.B)
        # clusters per mesh = 1 + the largest number: a padded (B, max F) table and a row maximum (a scatter-max would send every
        # face's atomic to one of B addresses)
        table = torch.full((pk.B, max(pk.nf)), -1, dtype=torch.int64, device=dev)
        table[pk.face_mesh, torch.arange(pk.F, device=dev) - pk.foff_t[pk.face_mesh]] = cl.long()
        per_mesh = table.amax(1) + 1
        first = torch.cumsum(per_mesh, 0) - per_mesh
        host = torch.cat([per_mesh, cl.min().long().view(1)]).tolist()      # the readback: C sizes the outputs
        counts, C = host[:pk.B], sum(host[:pk.B])
        if host[pk.B] < 0:
            raise ValueError("mesh_component_stats: negative cluster number")
        glob = (cl.long() + first[pk.face_mesh]).to(torch.int32)
        sorted_cl, order = torch.sort(glob, stable=True)
        vkeys = torch.sort((glob.long()[:, None] * pk.V + pk.faces.long()).reshape(-1))[0]
        area = torch.empty(C, dtype=torch.float64, device=dev)
        nvert = torch.empty(C, dtype=torch.int64, device=dev)
        vsum = torch.empty(C, 3, dtype=torch.float64, device=dev)
        launch(dev, "fsg_cluster_stats_f64", _p(pk.verts), _p(pk.faces), _p(sorted_cl), _p(order), _p(vkeys), pk.V, pk.F, C, _p(area),
               _p(nvert), _p(vsum))
    return area, nvert, vsum, counts


def mesh_remove_vertices(meshes, keep=None, box=None, mask=None, spacing=None, face_keep=None, drop_unreferenced=False):
    """Remove vertices (and the faces that lose one) from a batch of meshes and compact it (fsg_mesh_keep_flags_u8,
    fsg_mesh_face_flags_u8, fsg_mesh_compact_f32): open3d's remove_vertices_by_mask / crop / remove_triangles_by_mask /
    remove_unreferenced_vertices as utils/general_utils.py:157-209 and data_processing/surface_fitting.py:71-82 use them.

    A vertex is kept iff all the given tests pass: keep (sum V,) bool; box (2, 3) for all meshes or (B, 2, 3), rows (lo, hi) in
    (x, y, z), inclusive; mask (D, H, W) bool with spacing (sx, sy, sz): mask[iz, iy, ix] at i = floor(v / spacing), indices
    clamped from above like the reference's, a NEGATIVE index counts as outside (the reference's indexing wraps it around).
    A face survives iff its three vertices do and face_keep (sum F,) bool, if given, is set.  drop_unreferenced also removes the
    vertices that no surviving face names.  Survivors keep their order, faces are re-indexed.
    -> `mesh.Meshes` of as many meshes (vertex normals carried along when the input has them).  One host read (the sizes)."""
    from ..mesh import Meshes
    with torch.no_grad():
        pk = _PackedMeshes("mesh_remove_vertices", meshes)
        dev, V, F, B = pk.dev, pk.V, pk.F, pk.B

        def flags(t, n, what):
            if t is None:
                return None
            if not torch.is_tensor(t) or tuple(t.shape) != (n,) or t.is_floating_point():
                raise ValueError(f"mesh_remove_vertices: {what} must be a bool or integer tensor of shape ({n},)")
            _need_gpu(t)
            return (t != 0).to(torch.uint8).contiguous()
        keep, face_keep = flags(keep, V, "keep"), flags(face_keep, F, "face_keep")
        boxes = None
        if box is not None:
            boxes = torch.as_tensor(box, dtype=torch.float32).to(dev)
            if tuple(boxes.shape) == (2, 3):
                boxes = boxes.expand(B, 2, 3)
            if tuple(boxes.shape) != (B, 2, 3):
                raise ValueError(f"mesh_remove_vertices: box must be (2, 3) or ({B}, 2, 3): rows (lo, hi), got {tuple(boxes.shape)}")
            boxes = boxes.reshape(B, 6).contiguous()
        D = H = W = 0
        sp = (1., 1., 1.)
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dim() != 3 or mask.is_floating_point():
                raise ValueError("mesh_remove_vertices: mask must be a bool or integer tensor (D, H, W)")
            if spacing is None:
                raise ValueError("mesh_remove_vertices: a mask needs its spacing (sx, sy, sz)")
            sp = tuple(float(s) for s in (spacing.tolist() if torch.is_tensor(spacing) else spacing))
            if len(sp) != 3 or not all(0 < s < float("inf") for s in sp):
                raise ValueError(f"mesh_remove_vertices: spacing must be three positive numbers (sx, sy, sz), got {sp}")
            _need_gpu(mask)
            D, H, W = mask.shape
            if min(D, H, W) < 1 or D * H * W >= 2 ** 31:
                raise ValueError(f"mesh_remove_vertices: mask volume {tuple(mask.shape)} is empty or has 2^31 voxels or more")
            mask = (mask != 0).to(torch.uint8).contiguous()
        if V == 0:
            return meshes if isinstance(meshes, Meshes) else Meshes([meshes[0]], [meshes[1]])
        vkeep = torch.empty(V, dtype=torch.uint8, device=dev)
        fkeep = torch.empty(F, dtype=torch.uint8, device=dev)
        used = torch.zeros(V, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_mesh_keep_flags_u8", _p(pk.verts), V, _p(pk.voff_t), B, _p(keep), _p(boxes), _p(mask), D, H, W, *sp, _p(vkeep),
                      _stream())
            if F:                                                            # (an empty tensor has no address to hand over)
                _lib.call("fsg_mesh_face_flags_u8", _p(pk.faces), V, F, _p(vkeep), _p(face_keep), _p(fkeep), _p(used), _stream())
            vflag = used if drop_unreferenced else vkeep
            vnew = torch.cumsum(vflag, 0, dtype=torch.int64)
            vnew = torch.cat([vnew.new_zeros(1), vnew])                      # exclusive, with the total behind
            fnew = torch.cumsum(fkeep, 0, dtype=torch.int64)
            fnew = torch.cat([fnew.new_zeros(1), fnew])
            host = torch.cat([vnew[pk.voff_t.long()], fnew[pk.foff_t]]).tolist()   # the readback: the sizes depend on the data
            vo, fo = host[:B + 1], host[B + 1:]
            verts = torch.empty(vo[-1], 3, dtype=torch.float32, device=dev)
            normals = None if pk.normals is None else torch.empty(vo[-1], 3, dtype=torch.float32, device=dev)
            faces = torch.empty(fo[-1], 3, dtype=torch.int64, device=dev)
            if vo[-1] > 0:
                pad = torch.zeros(3, dtype=torch.int64, device=dev)         # stands in for the face arrays of a batch without faces
                _lib.call("fsg_mesh_compact_f32", _p(pk.verts), _p(pk.normals), _p(pk.faces if F else pad.int()), V, F, _p(pk.voff_t),
                          B, _p(vflag), _p(vnew), _p(fkeep if F else pad.to(torch.uint8)), _p(fnew), _p(verts), _p(normals),
                          _p(faces if fo[-1] else pad), _stream())
        cut = lambda t, o: [t[o[m]:o[m + 1]] for m in range(B)]             # noqa: E731
        return Meshes(cut(verts, vo), cut(faces, fo), None if normals is None else cut(normals, vo))
