"""Triangle-mesh batches, their regularisers and surface sampling on the HIP kernels of csrc/mesh.hip -- what the reference
takes from pytorch3d for `train_pc_ae.py --loss mesh` (losses/mesh_loss.py:28-57, models/folding_net.py:76-77, 225-226,
285-286): `Meshes`, `join_meshes_as_batch`, `sample_points_from_meshes`, `mesh_edge_loss`, `mesh_normal_consistency`,
`mesh_laplacian_smoothing(method="uniform")`.  `mesh_regularizers` is the one-launch form of the three terms.
`Meshes.sample_points_poisson_disk` / `sample_points_poisson_disk` stand in for open3d's TriangleMesh method of that name
(shape_model/point_cloud_registration.py:224, :338): the uniform sampler followed by weighted sample elimination on the GPU
(csrc/poisson_disk.hip), for the whole batch at once.

`Meshes` carries only what the reference's callers use.  It is a container on any device; everything that computes refuses
CPU tensors like the rest of the package.  Connectivity (unique edges, neighbour lists, the face pairs across an edge and the
per-vertex incidence lists the gradient needs) is built ONCE per face list on the host and cached by the identity of the
faces tensor(s): a decoder's faces never change, so a training run builds it on its first step.  DESIGN.md has the
definitions, the layout and the determinism rule.

Vertex normals are CARRIED, not computed: `Meshes(verts, faces, verts_normals=...)` keeps what marching cubes produced
(functional.marching_cubes), and asking a mesh that was given none raises NotImplementedError.

Not here: the cotangent / cotcurv Laplacian, a non-zero target edge length, textures, vertex normals of arbitrary meshes, and the
random stream of pytorch3d's sampler (the picks come from `torch.rand` through a fixed rule; which points are drawn for a given seed
differs from pytorch3d's multinomial)."""
import math

import torch
from torch.multiprocessing.reductions import StorageWeakRef

from . import _lib
from . import functional as F_hip
from ._launch import _amp_bwd, _amp_fwd, _f32c, _need_gpu, _p, launch


# ---------------------------------------------------------------------------------------------------------- topology
def build_topology(faces, V):
    """Connectivity of ONE mesh on the host: faces (F, 3) integer, V vertices -> dict of CPU int64 tensors

    edges (E, 2)    the unique undirected edges (lo, hi), ascending
    deg (V,), nbr_off (V + 1,), nbr (2E,)   neighbour lists over those edges, ascending per vertex
    pairs (P, 4)    (v0, v1, a, b): edge (v0, v1) and the opposite vertices of two faces that share it; an edge with c faces
                    gives all c (c - 1) / 2 unordered pairs, a boundary edge none; ordered by edge, then by face order
    inc_off (V + 1,), inc (4P,)   per vertex the pairs it is part of, as 4 * pair + role (0..3 = v0, v1, a, b), ascending

    A face that names a vertex twice has no edge structure and is refused, as are indices outside 0..V-1."""
    f = torch.as_tensor(faces).detach().cpu()
    if f.is_floating_point() or f.dtype == torch.bool or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be (F, 3) integer vertex indices, got {tuple(f.shape)} {f.dtype}")
    f = f.to(torch.int64)
    V = int(V)
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= V):
        raise ValueError(f"face indices span [{int(f.min())}, {int(f.max())}] but the mesh has {V} vertices")
    if bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()):
        raise ValueError("a face names the same vertex twice: such a face has no edges or normal")
    he = torch.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1).reshape(-1, 2)      # half-edges in face order
    opp = torch.stack([f[:, 2], f[:, 0], f[:, 1]], 1).reshape(-1)
    key = he.min(1).values * V + he.max(1).values
    order = torch.argsort(key, stable=True)
    uk, counts = torch.unique_consecutive(key[order], return_counts=True)
    opp = opp[order]
    edges = torch.stack([uk // V, uk % V], 1)
    E = edges.shape[0]
    starts = torch.cumsum(counts, 0) - counts
    rows, tags = [], []
    for c in torch.unique(counts).tolist():
        if c < 2:
            continue
        grp = torch.nonzero(counts == c).reshape(-1)                                     # edges shared by c faces
        comb = torch.combinations(torch.arange(c), 2)                                    # (K, 2), lexicographic
        at = starts[grp][:, None] + torch.arange(c)[None, :]                             # (G, c) half-edges of each edge
        a, b = opp[at[:, comb[:, 0]]], opp[at[:, comb[:, 1]]]                            # (G, K)
        e = edges[grp][:, None, :].expand(-1, comb.shape[0], -1)
        rows.append(torch.stack([e[..., 0], e[..., 1], a, b], -1).reshape(-1, 4))
        tags.append(grp[:, None].expand(-1, comb.shape[0]).reshape(-1))
    if rows:
        rows, tags = torch.cat(rows), torch.cat(tags)
        pairs = rows[torch.argsort(tags, stable=True)]
    else:
        pairs = torch.zeros(0, 4, dtype=torch.int64)
    src, dst = torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]])
    nbr = dst[torch.argsort(src * V + dst)]
    deg = torch.bincount(src, minlength=V)
    P = pairs.shape[0]
    pv = pairs.reshape(-1)
    inc = torch.argsort(pv * max(4 * P, 1) + torch.arange(4 * P))                        # position = 4 * pair + role
    zero = torch.zeros(1, dtype=torch.int64)
    return {"edges": edges, "deg": deg, "nbr_off": torch.cat([zero, torch.cumsum(deg, 0)]), "nbr": nbr, "pairs": pairs,
            "inc_off": torch.cat([zero, torch.cumsum(torch.bincount(pv, minlength=V), 0)]), "inc": inc, "V": V, "E": E, "P": P}


_cache = {}    # (kind, per-tensor keys, extra) -> ([weak storage references], value)


def _tensor_key(t):
    return (t.untyped_storage()._cdata, t.data_ptr(), t._version, tuple(t.shape), t.stride(), t.dtype, str(t.device))


def _cached(kind, tensors, extra, build):
    """`build()` once per (the identity of `tensors`, extra): storage, address and version counter, with a weak reference to
    the storage -- an in-place write or a freed and reused address is seen as another tensor (cf. functional._faces_range)"""
    key = (kind, tuple(_tensor_key(t) for t in tensors), extra)
    got = _cache.get(key)
    if got is None or any(r.expired() for r in got[0]):
        for k in [k for k, v in _cache.items() if any(r.expired() for r in v[0])]:
            del _cache[k]
        if len(_cache) >= 64:
            _cache.clear()
        got = _cache[key] = ([StorageWeakRef(t.untyped_storage()) for t in tensors], build())
    return got[1]


class _RegStruct:
    """device copy of a batch's connectivity in the layout of fsg_mesh_reg_f32"""

    def __init__(self, topos, which, num_verts, device):
        # topos: the distinct topologies; which[m]: the one mesh m uses
        i32 = lambda t: t.to(torch.int32).to(device)                   # noqa: E731
        obase, pbase, nbase, ibase, o, p, nb, ib = [], [], [], [], 0, 0, 0, 0
        for t in topos:
            obase.append(o), pbase.append(p), nbase.append(nb), ibase.append(ib)
            o, p, nb, ib = o + t["V"] + 1, p + t["P"], nb + t["nbr"].numel(), ib + t["inc"].numel()
        if max(o, 4 * p, nb, ib) >= 2 ** 31:
            raise ValueError("mesh batch too large for 32-bit connectivity tables")
        self.nbr_off = i32(torch.cat([t["nbr_off"] + b for t, b in zip(topos, nbase)]))
        self.inc_off = i32(torch.cat([t["inc_off"] + b for t, b in zip(topos, ibase)]))
        pad = torch.zeros(1, dtype=torch.int64)                         # never read; keeps the pointers non-NULL
        self.nbr = i32(torch.cat([t["nbr"] for t in topos] + [pad]))
        self.inc = i32(torch.cat([t["inc"] for t in topos] + [pad]))
        self.pairs = i32(torch.cat([t["pairs"] for t in topos] + [pad.expand(1, 4)]))
        desc, vb = [], 0
        for m, V in enumerate(num_verts):
            t = topos[which[m]]
            desc.append([vb, V, obase[which[m]], pbase[which[m]], t["E"], t["P"], 0, 0])
            vb += V
        self.desc = torch.tensor(desc, dtype=torch.int32).to(device)
        self.N, self.total_verts, self.max_V = len(num_verts), vb, max(num_verts)
        self.num_edges = [topos[w]["E"] for w in which]
        self.num_pairs = [topos[w]["P"] for w in which]


class _SampleStruct:
    """device copy of a batch's faces (local indices, int32) and the descriptors of fsg_mesh_sample_f32"""

    def __init__(self, faces, fbase, num_verts, num_faces, device):
        self.faces = faces
        desc, vb = [], 0
        for V, F, fb in zip(num_verts, num_faces, fbase):
            desc.append([vb, V, fb, F])
            vb += V
        self.sdesc = torch.tensor(desc, dtype=torch.int32).to(device)
        self.N, self.total_verts, self.max_V, self.max_F = len(num_verts), vb, max(num_verts), max(num_faces)


# ------------------------------------------------------------------------------------------------------------- Meshes
class Meshes:
    """A batch of triangle meshes: `Meshes(verts, faces)` with verts (B, V, 3) and faces (F, 3) (one face list for all) or
    (B, F, 3), or with lists of per-mesh (V_i, 3) / (F_i, 3) tensors.  Faces hold vertex indices local to their mesh.
    verts_normals, optional, has the form of verts."""

    def __init__(self, verts, faces, verts_normals=None):
        if torch.is_tensor(verts):
            if verts.dim() != 3 or verts.shape[2] != 3:
                raise ValueError(f"verts must be (B, V, 3) or a list of (V_i, 3), got {tuple(verts.shape)}")
            if not torch.is_tensor(faces) or faces.dim() not in (2, 3) or faces.shape[-1] != 3 or \
                    (faces.dim() == 3 and faces.shape[0] != verts.shape[0]):
                raise ValueError(f"faces must be (F, 3) or (B, F, 3) for verts {tuple(verts.shape)}, got "
                                 f"{tuple(faces.shape) if torch.is_tensor(faces) else type(faces).__name__}")
            if verts_normals is not None and (not torch.is_tensor(verts_normals) or verts_normals.shape != verts.shape):
                raise ValueError(f"verts_normals must have the shape of verts {tuple(verts.shape)}")
            self._padded, self._verts = verts, None
            self._faces_t, self._faces = faces, None
            self._normals = verts_normals
            self._nv, self._nf = [verts.shape[1]] * verts.shape[0], [faces.shape[-2]] * verts.shape[0]
            tensors = (verts, faces) + (() if verts_normals is None else (verts_normals,))
        else:
            verts, faces = list(verts), list(faces)
            if len(verts) != len(faces):
                raise ValueError(f"{len(verts)} vertex tensors for {len(faces)} face tensors")
            for v, f in zip(verts, faces):
                if not (torch.is_tensor(v) and v.dim() == 2 and v.shape[1] == 3 and torch.is_tensor(f) and f.dim() == 2
                        and f.shape[1] == 3):
                    raise ValueError("list form: verts (V_i, 3) and faces (F_i, 3) per mesh")
            if verts_normals is not None:
                verts_normals = list(verts_normals)
                if len(verts_normals) != len(verts) or any(not torch.is_tensor(n) or n.shape != v.shape
                                                           for n, v in zip(verts_normals, verts)):
                    raise ValueError("list form: verts_normals (V_i, 3) per mesh, matching verts")
            self._padded, self._verts = None, verts
            self._faces_t, self._faces = None, faces
            self._normals = verts_normals
            self._nv, self._nf = [v.shape[0] for v in verts], [f.shape[0] for f in faces]
            tensors = tuple(verts) + tuple(faces) + tuple(verts_normals or ())
        for f in ((self._faces_t,) if self._faces is None else self._faces):
            if f.is_floating_point() or f.dtype == torch.bool:
                raise ValueError(f"faces must hold integer vertex indices, got {f.dtype}")
        if len({t.device for t in tensors}) > 1:
            raise ValueError("all tensors of a Meshes must be on one device")
        self._device = tensors[0].device if tensors else torch.device("cpu")
        self._reg = None      # (edge, normal, laplacian) once evaluated: a Meshes is immutable

    # ---- the container
    def __len__(self):
        return len(self._nv)

    @property
    def device(self):
        return self._device

    def verts_list(self):
        return list(self._padded.unbind(0)) if self._verts is None else list(self._verts)

    def faces_list(self):
        if self._faces is not None:
            return list(self._faces)
        return [self._faces_t] * len(self) if self._faces_t.dim() == 2 else list(self._faces_t.unbind(0))

    def num_verts_per_mesh(self):
        return torch.tensor(self._nv, dtype=torch.int64, device=self._device)

    def num_faces_per_mesh(self):
        return torch.tensor(self._nf, dtype=torch.int64, device=self._device)

    def verts_packed(self):
        if self._verts is None:
            return self._padded.reshape(-1, 3)
        return torch.cat(self._verts) if self._verts else torch.zeros(0, 3, device=self._device)

    def faces_packed(self):
        """(sum F_i, 3) int64 indices into verts_packed()"""
        out, vb = [], 0
        for f, V in zip(self.faces_list(), self._nv):
            out.append(f.to(torch.int64) + vb)
            vb += V
        return torch.cat(out) if out else torch.zeros(0, 3, dtype=torch.int64, device=self._device)

    def verts_padded(self):
        """(B, max V, 3), zero rows behind the shorter meshes"""
        if self._verts is None:
            return self._padded
        if len(set(self._nv)) <= 1:
            return torch.stack(self._verts) if self._verts else torch.zeros(0, 0, 3, device=self._device)
        return torch.nn.utils.rnn.pad_sequence(self._verts, batch_first=True)

    def faces_padded(self):
        """(B, max F, 3) int64, rows of -1 behind the shorter meshes (pytorch3d's padding)"""
        fl = [f.to(torch.int64) for f in self.faces_list()]
        if not fl:
            return torch.zeros(0, 0, 3, dtype=torch.int64, device=self._device)
        return torch.stack(fl) if len(set(self._nf)) <= 1 else torch.nn.utils.rnn.pad_sequence(fl, batch_first=True, padding_value=-1)

    def _need_normals(self):
        if self._normals is None:
            raise NotImplementedError("this Meshes was given no verts_normals: vertex normals are only carried (marching cubes "
                                      "produces them), computing them for an arbitrary mesh is not built")

    def verts_normals_list(self):
        self._need_normals()
        return list(self._normals.unbind(0)) if self._verts is None else list(self._normals)

    def verts_normals_packed(self):
        self._need_normals()
        if self._verts is None:
            return self._normals.reshape(-1, 3)
        return torch.cat(self._normals) if self._normals else torch.zeros(0, 3, device=self._device)

    def verts_normals_padded(self):
        """(B, max V, 3), zero rows behind the shorter meshes"""
        self._need_normals()
        if self._verts is None:
            return self._normals
        if len(set(self._nv)) <= 1:
            return torch.stack(self._normals) if self._normals else torch.zeros(0, 0, 3, device=self._device)
        return torch.nn.utils.rnn.pad_sequence(self._normals, batch_first=True)

    def __getitem__(self, index):
        if isinstance(index, int):
            index = [index]
        elif isinstance(index, slice):
            index = list(range(len(self)))[index]
        elif torch.is_tensor(index):
            index = (torch.nonzero(index).reshape(-1) if index.dtype == torch.bool else index).tolist()
        v, f = self.verts_list(), self.faces_list()
        n = None if self._normals is None else self.verts_normals_list()
        return Meshes([v[i] for i in index], [f[i] for i in index], None if n is None else [n[i] for i in index])

    def to(self, device):
        device = torch.device(device)
        if device == self._device:
            return self
        if self._verts is None:
            return Meshes(self._padded.to(device), self._faces_t.to(device), None if self._normals is None else self._normals.to(device))
        return Meshes([v.to(device) for v in self._verts], [f.to(device) for f in self._faces],
                      None if self._normals is None else [n.to(device) for n in self._normals])

    # ---- what the kernels take
    def _face_tensors(self):
        return (self._faces_t,) if self._faces is None else tuple(self._faces)

    def _reg_struct(self):
        def build():
            if self._faces is None:
                fc = self._faces_t.detach().cpu()
                if fc.dim() == 3 and len(self) > 0 and bool((fc == fc[:1]).all()):
                    fc = fc[0]                                           # one face list repeated over the batch
                if fc.dim() == 2:
                    return _RegStruct([build_topology(fc, self._nv[0])], [0] * len(self), self._nv, self._device)
                faces = list(fc.unbind(0))
            else:
                faces = self._faces
            return _RegStruct([build_topology(f, V) for f, V in zip(faces, self._nv)], list(range(len(self))), self._nv,
                              self._device)
        return _cached("reg", self._face_tensors(), tuple(self._nv), build)

    def _sample_struct(self):
        def build():
            for f, V in ([(self._faces_t, self._nv[0])] if self._faces is None else zip(self._faces, self._nv)):
                lo, hi = F_hip._faces_range(f)
                if lo < 0 or hi >= V:
                    raise ValueError(f"face indices span [{lo}, {hi}] but the mesh has {V} vertices")
            if self._faces is None:
                fc = self._faces_t.detach().to(torch.int32).contiguous().reshape(-1, 3)
                step = self._nf[0] if self._faces_t.dim() == 3 else 0
                fbase = [step * m for m in range(len(self))]
            else:
                fc = torch.cat([f.detach().to(torch.int32) for f in self._faces]).contiguous()
                fbase = [0]
                for F in self._nf[:-1]:
                    fbase.append(fbase[-1] + F)
            return _SampleStruct(fc, fbase, self._nv, self._nf, self._device)
        return _cached("sample", self._face_tensors(), tuple(self._nv), build)

    def _check_computable(self, what, need_faces):
        if len(self) == 0:
            raise ValueError(f"{what}: empty batch of meshes")
        if min(self._nv) == 0 or (need_faces and min(self._nf) == 0):
            raise ValueError(f"{what}: a mesh without vertices" + (" or faces" if need_faces else ""))
        _need_gpu(*((self._padded,) if self._verts is None else self._verts), *self._face_tensors())

    def sample_points(self, n, generator=None, return_faces=False):
        """n points per mesh, uniform on the surface -> (B, n, 3), differentiable in the vertices [, face (B, n) int32,
        barycentric weights (B, n, 3)].  The uniforms are torch.rand(B, n, 3, generator=generator) on the meshes' device."""
        self._check_computable("sample_points", True)
        u = torch.rand(len(self), int(n), 3, device=self._device, dtype=torch.float32, generator=generator)
        return sample_points_from_uniforms(self, u, return_faces)

    def sample_points_poisson_disk(self, number_of_points, init_factor=5, generator=None, return_indices=False):
        """open3d's TriangleMesh.sample_points_poisson_disk for the whole batch: N = number_of_points blue-noise points per
        mesh -> (B, N, 3) fp32 [, the kept rows (B, N) int64 of the M initial samples, ascending].

        M = init_factor * N uniform surface samples are drawn from torch.rand(B, M, 3, generator=generator) through
        sample_points_from_uniforms and thinned by weighted sample elimination (functional.sample_elimination) with the
        constants open3d takes from Yuksel's paper: with A the mesh's surface area (the fp64 sum of face areas the sampler
        forms), R = 2 sqrt((A / N) / (2 sqrt 3)) and r_min = R / 2 (1 - (N / M)^1.5), evaluated in fp64 on the device and
        rounded to fp32.  Survivors keep their sample order.  Runs under no_grad and returns constants: no gradient reaches
        the vertices.  No host synchronisation.  Parity with open3d's own random stream and loop is unpinned."""
        N = number_of_points
        if isinstance(N, bool) or not isinstance(N, int) or N < 1:
            raise ValueError(f"sample_points_poisson_disk: number_of_points must be a positive integer, got {N!r}")
        if isinstance(init_factor, bool) or not isinstance(init_factor, (int, float)) or not init_factor >= 1:
            raise ValueError(f"sample_points_poisson_disk: init_factor must be a number >= 1, got {init_factor!r}")
        M = int(init_factor * N)
        if M > _lib.SAMPLE_ELIMINATION_MAX_POINTS:
            raise ValueError(f"sample_points_poisson_disk: init_factor * number_of_points = {M} initial samples, the elimination "
                             f"kernel serves at most {_lib.SAMPLE_ELIMINATION_MAX_POINTS}")
        self._check_computable("sample_points_poisson_disk", True)
        B = len(self)
        with torch.no_grad():
            u = torch.rand(B, M, 3, device=self._device, dtype=torch.float32, generator=generator)
            st = self._sample_struct()
            pts, _, _, cdf = _mesh_sample_raw(self.verts_packed(), u, st)
            last = (torch.tensor(self._nf, dtype=torch.int64) - 1).to(self._device)
            R, r_min = poisson_disk_radii(cdf.gather(1, last[:, None])[:, 0], N, M)
            keep = F_hip.sample_elimination(pts, N, R, r_min)
            out = torch.gather(pts, 1, keep[:, :, None].expand(B, N, 3))
        return (out, keep) if return_indices else out


def poisson_disk_radii(area, n, m):
    """open3d's constants of the weighted sample elimination for n points from m samples of a surface of area `area` ((B,)
    tensor): R = 2 sqrt((A / n) / (2 sqrt 3)), r_min = R / 2 (1 - (n / m)^1.5), in fp64, rounded to fp32 -> (R, r_min)"""
    a = area.to(torch.float64)
    # (tensor divisors: torch divides by a Python number through its reciprocal, which is not the quotient to the last bit)
    R = 2.0 * torch.sqrt((a / torch.full_like(a, n)) / torch.full_like(a, 2.0 * math.sqrt(3.0)))
    r_min = R * 0.5 * (1.0 - (n / m) ** 1.5)
    return R.to(torch.float32), r_min.to(torch.float32)


def sample_points_poisson_disk(meshes, number_of_points, init_factor=5, generator=None, return_indices=False):
    """`meshes.sample_points_poisson_disk(...)`"""
    return meshes.sample_points_poisson_disk(number_of_points, init_factor=init_factor, generator=generator,
                                             return_indices=return_indices)


def join_meshes_as_batch(meshes):
    """list of Meshes -> one Meshes holding all their meshes in order"""
    meshes = list(meshes)
    if len(meshes) == 1:
        return meshes[0]
    normals = [n for m in meshes for n in m.verts_normals_list()] if meshes and all(m._normals is not None for m in meshes) else None
    return Meshes([v for m in meshes for v in m.verts_list()], [f for m in meshes for f in m.faces_list()], normals)


# ----------------------------------------------------------------------------------------------------------- sampling
def _mesh_sample_raw(verts, u, st):
    """fsg_mesh_sample_f32 -> (pts, face, w, cdf): cdf (N, max_F) fp64 is the kernel's inclusive prefix sum of the face areas of
    every mesh (its workspace)"""
    vc, uc = _f32c(verts), _f32c(u)
    N, n = uc.shape[0], uc.shape[1]
    dev = vc.device
    pts = torch.empty(N, n, 3, dtype=torch.float32, device=dev)
    face = torch.empty(N, n, dtype=torch.int32, device=dev)
    w = torch.empty(N, n, 3, dtype=torch.float32, device=dev)
    ws = _lib.workspace("fsg_mesh_sample", N, st.max_F, device=dev)
    launch(dev, "fsg_mesh_sample_f32", _p(vc), _p(st.faces), _p(st.sdesc), N, st.max_F, _p(uc), n, _p(pts), _p(face),
           _p(w), _p(ws), ws.numel())
    return pts, face, w, ws.view(torch.float64).view(N, st.max_F)


class _MeshSample(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, verts, u, st):
        pts, face, w, _ = _mesh_sample_raw(verts, u, st)
        ctx.st, ctx.n = st, u.shape[1]
        ctx.save_for_backward(face, w)
        ctx.mark_non_differentiable(face, w)
        return pts, face, w

    @staticmethod
    @_amp_bwd
    def backward(ctx, g, _gf, _gw):
        face, w = ctx.saved_tensors
        st = ctx.st
        gc = _f32c(g)
        gv = torch.empty(st.total_verts, 3, dtype=torch.float32, device=gc.device)
        launch(gc.device, "fsg_mesh_sample_bwd_f32", _p(gc), _p(face), _p(w), _p(st.faces), _p(st.sdesc), st.N, st.max_V, ctx.n,
               _p(gv))
        return gv, None, None


def sample_points_from_uniforms(meshes, u, return_faces=False):
    """The sampler on caller-supplied uniforms u (B, n, 3) in [0, 1): face = min{ j : C[j] > u0 C[F-1] } over the inclusive
    prefix sum C of the face areas, barycentric weights (1 - sqrt u1, sqrt u1 (1 - u2), sqrt u1 u2)."""
    meshes._check_computable("sample_points", True)
    _need_gpu(u)
    if u.dim() != 3 or u.shape[0] != len(meshes) or u.shape[2] != 3 or u.shape[1] == 0:
        raise ValueError(f"uniforms must be (B, n, 3) with B = {len(meshes)} and n > 0, got {tuple(u.shape)}")
    pts, face, w = _MeshSample.apply(meshes.verts_packed(), u, meshes._sample_struct())
    return (pts, face, w) if return_faces else pts


def sample_points_from_meshes(meshes, num_samples=10000, generator=None):
    """pytorch3d.ops.sample_points_from_meshes without normals and textures -> (B, num_samples, 3)"""
    return meshes.sample_points(num_samples, generator=generator)


# ------------------------------------------------------------------------------------------------------- regularisers
class _MeshReg(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, verts, st):
        vc = _f32c(verts)
        dev = vc.device
        terms = torch.empty(st.N, 3, dtype=torch.float32, device=dev)
        mean = torch.empty(3, dtype=torch.float32, device=dev)
        grads = torch.empty(3, st.total_verts, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        ws = _lib.workspace("fsg_mesh_reg", st.N, st.max_V, device=dev)
        launch(dev, "fsg_mesh_reg_f32", _p(vc), st.total_verts, _p(st.desc), st.N, st.max_V, _p(st.nbr_off), _p(st.nbr),
               _p(st.pairs), _p(st.inc_off), _p(st.inc), _p(terms), _p(mean), _p(grads), _p(ws), ws.numel())
        ctx.N = st.N
        if grads is not None:
            ctx.save_for_backward(grads)
        ctx.mark_non_differentiable(terms)
        return mean, terms

    @staticmethod
    @_amp_bwd
    def backward(ctx, g, _gt):
        grads, = ctx.saved_tensors
        w = g.to(torch.float32) / ctx.N                                 # the value is the mean over the meshes
        return (grads[0] * w[0]).addcmul_(grads[1], w[1]).addcmul_(grads[2], w[2]), None


def mesh_regularizers(meshes, per_mesh=False):
    """(edge length, normal consistency, uniform Laplacian) of a batch, each the mean over the meshes of the per-mesh mean,
    from one kernel launch that also yields the vertex gradients.  per_mesh=True adds the (B, 3) per-mesh terms (no gradient)."""
    if not isinstance(meshes, Meshes):
        raise TypeError(f"expected fissure_segmentation_amd.mesh.Meshes, got {type(meshes).__name__}")
    if meshes._reg is None:
        meshes._check_computable("mesh_regularizers", False)
        meshes._reg = _MeshReg.apply(meshes.verts_packed(), meshes._reg_struct())
    mean, terms = meshes._reg
    out = (mean[0], mean[1], mean[2])
    return out + (terms,) if per_mesh else out


def mesh_edge_loss(meshes, target_length=0.0):
    if target_length != 0:
        raise NotImplementedError("mesh_edge_loss: only target_length = 0 (what the reference uses) is built")
    return mesh_regularizers(meshes)[0]


def mesh_normal_consistency(meshes):
    return mesh_regularizers(meshes)[1]


def mesh_laplacian_smoothing(meshes, method="uniform"):
    if method != "uniform":
        raise NotImplementedError(f'mesh_laplacian_smoothing: method "{method}" is not built, only "uniform"')
    return mesh_regularizers(meshes)[2]
