"""Checkers of the weighted sample elimination (csrc/poisson_disk.hip; the rule is stated in include/fsg_hip.h):

(a) `eliminate`       the kernel's rule restated in numpy, bit for bit: the same fp32 operation order, the same quantisation
                      rint(w 2^24) into int64 sums, the same tie rule (largest weight, lowest index).  Dense: the pair matrix
                      is formed `chunk` rows at a time, a round is one vector pass over all samples and an arg-max.
(b) `eliminate_heap`  an independent implementation on other data structures: neighbour lists from scipy.spatial.cKDTree radius
                      queries (a superset radius, then the same fp32 predicate), a binary heap keyed (-weight, index) with lazy
                      deletion, updates that walk the removed sample's list.  It consumes the same pair-weight function, so a
                      wrong update or tie rule shows, not a different rounding.
Integer sums do not depend on their order: (a) and (b) must agree exactly.

`radii` are open3d's constants from Yuksel's paper, `min_nn_distance` the blue-noise measure of the CPU tests."""
import heapq

import numpy as np

MAX_POINTS = 16384
Q_ONE = np.float32(2.0 ** 24)


def sq_dist(a, b):
    """((dx dx + dy dy) + dz dz) in fp32, in that order, of (.., 3) arrays that broadcast"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def pair_weight(d2, R, r_min):
    """fp32 w of neighbours at squared distance d2: d = max(sqrt d2, r_min), t = max(1 - d / R, 0), ((t^2)^2)^2"""
    d2, R, r_min = np.asarray(d2, np.float32), np.float32(R), np.float32(r_min)
    with np.errstate(all="ignore"):
        d = np.fmax(np.sqrt(d2), r_min)
        t = np.fmax(np.float32(1) - d / R, np.float32(0))
    t = t * t
    t = t * t
    return t * t


def pair_q(d2, R, r_min):
    """the quantised weight, int64"""
    return np.rint(pair_weight(d2, R, r_min) * Q_ONE).astype(np.int64)


def is_neighbour(d2, R):
    R = np.float32(R)
    return (d2 < R * R) if R > 0 else np.zeros(np.shape(d2), bool)


def _check(points, n_keep):
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] != 3 or not 1 <= len(p) <= MAX_POINTS:
        raise ValueError(f"points must be (M, 3) with 1 <= M <= {MAX_POINTS}, got {p.shape}")
    if not 1 <= n_keep <= len(p):
        raise ValueError(f"n_keep={n_keep} for {len(p)} points")
    if not np.isfinite(p).all():
        raise ValueError("coordinates must be finite")
    return p


def initial_weights(p, R, r_min, chunk=1024):
    """int64 (M,): row sums of the quantised pair matrix without its diagonal, `chunk` rows at a time"""
    M = len(p)
    w = np.zeros(M, np.int64)
    if not np.float32(R) > 0:
        return w
    for i0 in range(0, M, chunk):
        d2 = sq_dist(p[i0:i0 + chunk, None], p[None])
        nb = is_neighbour(d2, R)
        nb[np.arange(d2.shape[0]), i0 + np.arange(d2.shape[0])] = False
        r, c = np.nonzero(nb)
        q = pair_q(d2[r, c], R, r_min)
        # at most 16383 terms of at most 2^24: exact in the fp64 accumulator of bincount
        w[i0:i0 + d2.shape[0]] = np.bincount(r, weights=q.astype(np.float64), minlength=d2.shape[0]).astype(np.int64)
    return w


def eliminate(points, n_keep, R, r_min, chunk=1024):
    """(a) -> (keep (n_keep,) ascending, order (M - n_keep,)), int64"""
    p = _check(points, n_keep)
    M = len(p)
    if n_keep == M:
        return np.arange(M, dtype=np.int64), np.zeros(0, np.int64)
    w = initial_weights(p, R, r_min, chunk)
    alive = np.ones(M, bool)
    order = np.empty(M - n_keep, np.int64)
    for t in range(M - n_keep):
        i = int(np.argmax(np.where(alive, w, -1)))     # the first maximum: the lowest index
        order[t] = i
        alive[i] = False
        d2 = sq_dist(p, p[i])
        nb = is_neighbour(d2, R) & alive
        w[nb] -= pair_q(d2[nb], R, r_min)
    return np.nonzero(alive)[0].astype(np.int64), order


def eliminate_heap(points, n_keep, R, r_min):
    """(b) -> (keep, order)"""
    from scipy.spatial import cKDTree
    p = _check(points, n_keep)
    M = len(p)
    nbrs = [[] for _ in range(M)]
    weight = [0] * M
    if np.float32(R) > 0:
        pairs = cKDTree(p.astype(np.float64)).query_pairs(float(np.float32(R)) * (1 + 1e-4) + 1e-30, output_type="ndarray")
        if len(pairs):
            d2 = sq_dist(p[pairs[:, 0]], p[pairs[:, 1]])
            real = is_neighbour(d2, R)
            for (i, j), q in zip(pairs[real].tolist(), pair_q(d2[real], R, r_min).tolist()):
                nbrs[i].append((j, q))
                nbrs[j].append((i, q))
                weight[i] += q
                weight[j] += q
    heap = [(-weight[i], i) for i in range(M)]
    heapq.heapify(heap)
    alive = [True] * M
    order = []
    while len(order) < M - n_keep:
        negw, i = heapq.heappop(heap)
        if not alive[i] or -negw != weight[i]:
            continue                                   # a stale entry
        alive[i] = False
        order.append(i)
        for j, q in nbrs[i]:
            if alive[j]:
                weight[j] -= q
                heapq.heappush(heap, (-weight[j], j))
    return np.array([i for i in range(M) if alive[i]], np.int64), np.array(order, np.int64)


def radii(area, n, m):
    """open3d's constants: R = 2 sqrt((A / n) / (2 sqrt 3)) (twice the radius of n discs packed hexagonally into A),
    r_min = R / 2 (1 - (n / m)^1.5); fp64, then rounded to fp32 -> (R, r_min)"""
    area = np.asarray(area, np.float64)
    R = 2.0 * np.sqrt((area / n) / (2.0 * np.sqrt(3.0)))
    r_min = R * 0.5 * (1.0 - (n / m) ** 1.5)
    return R.astype(np.float32), r_min.astype(np.float32)


def min_nn_distance(p):
    """the smallest distance between two different rows, fp64"""
    p = np.asarray(p, np.float64)
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    d[np.arange(len(p)), np.arange(len(p))] = np.inf
    return float(d.min())


def unit_square(seed, m):
    """m uniform points of the unit square in the plane z = 0, fp32"""
    xy = np.random.default_rng(seed).random((m, 2))
    return np.concatenate([xy, np.zeros((m, 1))], 1).astype(np.float32)


def lattice(side=17):
    """side x side points of a square lattice with spacing 1/16 (exact in fp32): many samples share a weight, so nearly every
    round is decided by the tie rule -> (points, R, r_min)"""
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    p = np.stack([i.ravel() / 16, j.ravel() / 16, np.zeros(side * side)], 1).astype(np.float32)
    return p, np.float32(0.16), np.float32(0.01)


def duplicates_cloud(seed=3, m=96):
    """a cloud with exact duplicate rows and with pairs closer than r_min -> (points, R, r_min)"""
    rng = np.random.default_rng(seed)
    p = unit_square(seed, m)
    p[10] = p[3]
    p[11] = p[3]
    p[40] = p[77]
    p[50] = p[20] + np.float32(1e-4) * rng.standard_normal(3).astype(np.float32)
    p[60] = p[61] + np.float32([2e-3, 0, 0])
    return p, np.float32(0.25), np.float32(0.02)


# ------------------------------------------------------------------ register_all: test data and the pipeline on the CPU
REG_INSTANCES, REG_OBJECTS, REG_POINTS, REG_INIT_FACTOR = 3, 2, 64, 5


def grid_mesh(height, offset_y, nu=33, nv=2, half_width=1.0):
    """a strip of 120 x (2 half_width) units over u in [-1, 1] as nu x nv vertices, z = height(u), shifted by offset_y
    -> (verts (V,3) fp64, faces (F,3))"""
    u, v = np.meshgrid(np.linspace(-1, 1, nu), np.linspace(-1, 1, nv), indexing="ij")
    verts = np.stack([60 * u, offset_y + half_width * v, height(u) + 0 * v], -1).reshape(-1, 3)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return verts, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)


def fixed_surfaces():
    """the two objects: two curved strips 40 units apart.  A strip, because REG_POINTS = 64 points cover it with a spacing of
    about 2 units, a third of the 5 % of the bounding-box diagonal that counts as a correspondence: on a sheet of the same length
    the spacing would be 13 units, and whether a registered point counts would hinge on which sample it landed next to"""
    return [grid_mesh(lambda u: 15 * np.sin(2 * u), -20.0), grid_mesh(lambda u: 10 * np.cos(2.5 * u) + 6 * u, 20.0)]


def moving_surfaces():
    """REG_INSTANCES x REG_OBJECTS meshes: the fixed surfaces moved by one similarity per instance and bent by a smooth
    sinusoid of about a unit -> all_moving_meshes[instance][object] = (verts fp32, faces int64)"""
    out = []
    for i in range(REG_INSTANCES):
        ang, s = 0.06 * (i - 1), 1.0 + 0.04 * (i - 1)
        R = np.array([[np.cos(ang), -np.sin(ang), 0.], [np.sin(ang), np.cos(ang), 0.], [0., 0., 1.]])
        t = np.array([6.0 * i - 5.0, 4.0 - 3.0 * i, 2.0 * i - 3.0])
        inst = []
        for v, f in fixed_surfaces():
            w = s * v @ R.T + t
            bend = np.stack([0.8 * np.sin(w[:, 1] / 30), np.zeros(len(w)), 1.2 * np.sin(w[:, 0] / 40 + i)], 1)
            inst.append(((w + bend).astype(np.float32), f))
        out.append(inst)
    return out


def poisson_disk_cpu(verts, faces, u, n):
    """one mesh on the CPU: uniforms u (m,3) fp32 -> the fp32 restatement of the surface sampler (tests/mesh_oracle.sample),
    open3d's radii from the fp64 area, oracle (a) -> (points (n,3) fp32, kept rows)"""
    import torch
    import mesh_oracle
    v, f = torch.from_numpy(np.asarray(verts, np.float32)), torch.from_numpy(np.asarray(faces, np.int64))
    pts = mesh_oracle.sample(v, f, torch.from_numpy(np.asarray(u, np.float32)), torch.float32)[0].numpy()
    R, r_min = radii(float(mesh_oracle.face_cdf(v, f)[-1]), n, len(pts))
    keep, _ = eliminate(pts, n, R, r_min)
    return pts[keep], keep


def fixed_clouds(seed=11):
    """REG_POINTS blue-noise points of every fixed surface -> (objects, P, 3) fp64"""
    rng = np.random.default_rng(seed)
    return np.stack([poisson_disk_cpu(v, f, rng.random((REG_INIT_FACTOR * REG_POINTS, 3), np.float32), REG_POINTS)[0]
                     for v, f in fixed_surfaces()]).astype(np.float64)


def register_all_cpu(fixed, meshes, uniforms):
    """register_all from the oracles alone: uniforms[object] (instances, m, 3) fp32 -> dict with moving, moved (I,O,P,3) fp64,
    the nearest-neighbour distance of every moved point to its fixed cloud (I,O,P) and the heuristic distances (O,)"""
    import torch
    import cpd_oracle
    I, O, P = len(meshes), len(fixed), fixed.shape[1]
    moving = np.stack([np.stack([poisson_disk_cpu(*meshes[i][o], uniforms[o][i], P)[0] for o in range(O)])
                       for i in range(I)]).astype(np.float64)
    X = torch.from_numpy(fixed)
    moved = np.empty_like(moving)
    for i in range(I):
        pre = cpd_oracle.rigid(X.reshape(O * P, 3), torch.from_numpy(moving[i].reshape(O * P, 3)))["TY"].reshape(O, P, 3)
        for o in range(O):
            moved[i, o] = cpd_oracle.deformable(X[o], pre[o], alpha=0.01, beta=10)["TY"].numpy()
    nn = np.sqrt(((moved[:, :, :, None] - fixed[None, :, None]) ** 2).sum(-1)).min(-1)
    heur = 0.05 * np.linalg.norm(fixed.max(1) - fixed.min(1), axis=-1)
    return dict(moving=moving, moved=moved, nn=nn, heuristic=heur)
