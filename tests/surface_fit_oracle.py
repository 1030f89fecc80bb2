"""numpy / scipy restatement of the surface-fitting feature (csrc/mesh_cleanup.hip, functional.orient_normals_consistent,
mesh_face_components, mesh_component_stats, mesh_remove_vertices, utils.general_utils.remove_all_but_biggest_component) and the
seeded inputs of its tests.  It never imports the package.

Orientation: Kruskal over the kernel's key order (the key names its edge, so the order is strict and the forest unique), a walk
over the forest that carries the signs, and the root rule.  Everything that decides an ORDER is computed in fp32 exactly as the
kernel computes it (the dot product summed x, y, z; floor(v / spacing)); everything that is a VALUE (areas, centres) in fp64."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

AXES = (1.0, 0.7, 0.4)


# ------------------------------------------------------------------ orientation
def f2o(z):
    """the order-preserving uint32 image of fp32 values (csrc/fsg_device.h)"""
    u = np.asarray(z, np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dot32(normals, u, v):
    a, b = normals[u].astype(np.float32), normals[v].astype(np.float32)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def graph_edges(normals, idx, offset):
    """the undirected edges of the packed cloud's graph -> u, v (global, u < v), key (uint64), weight bits (the key's upper 24
    bits), dot (fp32), each edge once, in ascending key order PER SEGMENT (segments in order)"""
    normals = np.asarray(normals, np.float32)
    idx = np.asarray(idx)
    n, K = idx.shape
    us, vs, keys, wbits, dots = [], [], [], [], []
    st = 0
    for en in np.asarray(offset).tolist():
        ns = en - st
        ks = min(K, ns - 1)
        if ks > 1:
            u = np.repeat(np.arange(st, en), ks - 1)
            v = np.clip(idx[st:en, 1:ks].reshape(-1), st, en - 1).astype(np.int64)
            sel = u != v
            lo, hi = np.minimum(u, v)[sel], np.maximum(u, v)[sel]
            d = dot32(normals, lo, hi)
            w = np.maximum(np.float32(1) - np.abs(d), np.float32(0)).astype(np.float32)
            wb = (w.view(np.uint32) >> 8).astype(np.uint64)
            key = (wb << np.uint64(40)) | ((lo - st).astype(np.uint64) << np.uint64(20)) | (hi - st).astype(np.uint64)
            key, first = np.unique(key, return_index=True)
            us.append(lo[first]), vs.append(hi[first]), keys.append(key), wbits.append(wb[first]), dots.append(d[first])
        st = en
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)     # noqa: E731
    return cat(us, np.int64), cat(vs, np.int64), cat(keys, np.uint64), cat(wbits, np.uint64), cat(dots, np.float32)


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def orient(xyz, normals, idx, offset):
    """-> dict(signs int8 (n,), comp int32 (n,), oriented (n, 3) fp32, forest = indices into graph_edges' lists, edges = those
    lists)"""
    xyz, normals = np.asarray(xyz, np.float32), np.asarray(normals, np.float32)
    n = len(xyz)
    u, v, key, wb, d = edges = graph_edges(normals, idx, offset)
    parent = list(range(n))
    forest = []
    for e in range(len(u)):                                   # per segment in key order; segments never share a component
        a, b = _find(parent, int(u[e])), _find(parent, int(v[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            forest.append(e)
    comp = np.array([_find(parent, i) for i in range(n)], np.int32)      # the smaller root always stays: the smallest member
    adj = [[] for _ in range(n)]
    for e in forest:
        flip = bool(d[e] < 0)
        adj[int(u[e])].append((int(v[e]), flip))
        adj[int(v[e])].append((int(u[e]), flip))
    zkey = (f2o(xyz[:, 2]).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    signs = np.zeros(n, np.int8)
    for c in np.unique(comp):
        members = np.nonzero(comp == c)[0]
        top = int(members[np.argmax(zkey[members])])          # largest z, the lowest index on ties
        signs[top] = -1 if normals[top, 2] < 0 else 1
        stack = [top]
        while stack:
            a = stack.pop()
            for b, flip in adj[a]:
                if signs[b] == 0:
                    signs[b] = -signs[a] if flip else signs[a]
                    stack.append(b)
    assert (signs != 0).all()
    oriented = (normals.view(np.uint32) ^ ((signs < 0).astype(np.uint32) << np.uint32(31))[:, None]).view(np.float32)
    return dict(signs=signs, comp=comp, oriented=oriented, forest=np.array(forest, np.int64), edges=edges)


def knn(xyz, offset, K):
    """(n, K) int32 in fsg_knn_segment_f32's layout from fp64 distances: ascending, the point itself first, the lower index first
    on ties; columns beyond a short segment hold the segment's first row"""
    xyz = np.asarray(xyz, np.float64)
    out = np.zeros((len(xyz), K), np.int32)
    st = 0
    for en in np.asarray(offset).tolist():
        x = xyz[st:en]
        d = ((x[:, None] - x[None]) ** 2).sum(-1)
        d[np.arange(en - st), np.arange(en - st)] = -1.0
        order = np.argsort(d, axis=1, kind="stable")[:, :K] + st
        out[st:en] = st
        out[st:en, :order.shape[1]] = order
        st = en
    return out


# ------------------------------------------------------------------ seeded clouds with analytic normals
def ellipsoid(n, seed, axes=AXES):
    """n points on the ellipsoid (uniform directions scaled by the semi-axes) -> xyz (n, 3) fp32, outward unit normals (n, 3)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * np.array(axes)
    g = p / np.array(axes) ** 2
    return p.astype(np.float32), g / np.linalg.norm(g, axis=1, keepdims=True)


def wavy_sheet(n, seed):
    """n points on the open sheet z = 0.1 sin(3 x) cos(2 y) over [-1, 1]^2 -> xyz (n, 3) fp32, upward unit normals (n, 3)"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    z = 0.1 * np.sin(3 * x) * np.cos(2 * y)
    g = np.stack([-0.3 * np.cos(3 * x) * np.cos(2 * y), 0.2 * np.sin(3 * x) * np.sin(2 * y), np.ones(n)], 1)
    return np.stack([x, y, z], 1).astype(np.float32), g / np.linalg.norm(g, axis=1, keepdims=True)


def ellipsoid_distance(p, axes, centre=(0.0, 0.0, 0.0)):
    """distance of every point p (n, 3) to the surface of the axis-aligned ellipsoid: the closest point is
    x_i = a_i^2 y_i / (t + a_i^2) with t the largest root of sum (a_i y_i / (t + a_i^2))^2 = 1 (bisection, fp64)"""
    a = np.asarray(axes, np.float64)
    y = np.abs(np.asarray(p, np.float64) - np.asarray(centre, np.float64))
    y = np.maximum(y, 1e-12 * a.max())
    lo = np.full(len(y), -a.min() ** 2 + 1e-14)
    hi = np.full(len(y), (np.linalg.norm(y * a, axis=1)).max() + 1.0)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        f = ((a * y / (mid[:, None] + a ** 2)) ** 2).sum(1) - 1
        lo, hi = np.where(f > 0, mid, lo), np.where(f > 0, hi, mid)
    t = 0.5 * (lo + hi)
    x = a ** 2 * y / (t[:, None] + a ** 2)
    return np.linalg.norm(x - y, axis=1)


# ------------------------------------------------------------------ face clusters, statistics
def face_clusters(faces):
    """faces (F, 3) of ONE mesh -> clusters (F,) int32 numbered by their smallest face, count"""
    faces = np.asarray(faces, np.int64)
    F = len(faces)
    if F == 0:
        return np.zeros(0, np.int32), 0
    he = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    face = np.tile(np.arange(F), 3)
    V = int(faces.max()) + 1
    key = he[:, 0] * V + he[:, 1]
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    a, b = face[order][1:][same], face[order][:-1][same]
    g = coo_matrix((np.ones(len(a)), (a, b)), shape=(F, F))
    _, lab = connected_components(g, directed=False)
    _, first = np.unique(lab, return_index=True)              # the smallest face of every label
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[lab].astype(np.int32), len(first)


def cluster_stats(verts, faces, clusters, dtype=np.float64):
    """-> area (c,), distinct-vertex count (c,), distinct-vertex coordinate sum (c, 3) in `dtype`"""
    verts, faces = np.asarray(verts).astype(dtype), np.asarray(faces, np.int64)
    c = int(clusters.max()) + 1 if len(clusters) else 0
    area, num, vsum = np.zeros(c, dtype), np.zeros(c, np.int64), np.zeros((c, 3), dtype)
    for k in range(c):
        t = faces[clusters == k]
        v0, v1, v2 = verts[t[:, 0]], verts[t[:, 1]], verts[t[:, 2]]
        cr = np.cross(v1 - v0, v2 - v0)
        area[k] = (dtype(0.5) * np.sqrt((cr * cr).sum(1))).sum()
        uniq = np.unique(t)
        num[k] = len(uniq)
        vsum[k] = verts[uniq].sum(0)
    return area, num, vsum


def biggest_component(verts, faces, right=None, center_x=None):
    """utils/general_utils.py:171-209 -> (the chosen cluster, clusters, count); faces of ONE non-empty mesh"""
    clusters, c = face_clusters(faces)
    area, num, vsum = cluster_stats(verts, faces, clusters)
    value = area.copy()
    if center_x is not None and right is not None:
        cx = vsum[:, 0] / num
        for k in range(c):
            if (right and cx[k] > center_x) or (not right and cx[k] < center_x):
                value[k] = -1 / value[k]
    return int(value.argmax()), clusters, c


# ------------------------------------------------------------------ keep flags, compaction
def keep_flags(verts, box=None, mask=None, spacing=None):
    """verts (V, 3) fp32 in (x, y, z); box (2, 3) inclusive; mask (D, H, W) bool with spacing (sx, sy, sz): floor(v / s) in
    fp32, clamped from above, negative = outside"""
    v = np.asarray(verts, np.float32)
    keep = np.ones(len(v), bool)
    if box is not None:
        b = np.asarray(box, np.float32)
        keep &= ((v >= b[0]) & (v <= b[1])).all(1)
    if mask is not None:
        q = np.floor(v / np.asarray(spacing, np.float32))
        inside = (q >= 0).all(1)
        top = np.array(mask.shape[::-1], np.float32) - 1
        i = np.minimum(np.where(q >= 0, q, 0), top).astype(np.int64)
        keep &= inside & mask[i[:, 2], i[:, 1], i[:, 0]]
    return keep


def compact(verts, faces, vert_keep, face_keep=None, drop_unreferenced=False, normals=None):
    """-> verts, faces (re-indexed, int64)[, normals] of the survivors in their old order"""
    verts, faces = np.asarray(verts), np.asarray(faces, np.int64)
    fk = vert_keep[faces].all(1) if len(faces) else np.zeros(0, bool)
    if face_keep is not None:
        fk &= face_keep
    vk = vert_keep.copy()
    if drop_unreferenced:
        vk = np.zeros(len(verts), bool)
        vk[faces[fk].reshape(-1)] = True
    new = np.cumsum(vk) - 1
    out = (verts[vk], new[faces[fk]].reshape(-1, 3))
    return out if normals is None else out + (np.asarray(normals)[vk],)


# ------------------------------------------------------------------ the clean-up fixture
FIELD_SHAPE = (24, 20, 28)           # D, H, W


def blob_field():
    """a 24 x 20 x 28 field (inside = negative) with three disjoint blobs and a fourth whose corner node is the diagonal
    neighbour of a corner node of the third: they touch at one grid vertex of the cell between them"""
    D, H, W = FIELD_SHAPE
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    f = np.full(FIELD_SHAPE, 1.0)
    for (cz, cy, cx), r in (((6, 6, 6), 3.6), ((16, 12, 8), 4.3), ((8, 11, 20), 3.2)):
        f = np.minimum(f, (np.sqrt((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2) - r) / r)
    # third-and-a-half: two boxes of inside nodes, corners (18, 4, 22) and (19, 5, 23) diagonal across one cell
    rng = np.random.default_rng(5)
    depth = -rng.uniform(0.3, 0.9, FIELD_SHAPE)
    box_a = (z >= 15) & (z <= 18) & (y >= 2) & (y <= 4) & (x >= 19) & (x <= 22)
    box_b = (z >= 19) & (z <= 21) & (y >= 5) & (y <= 8) & (x >= 23) & (x <= 25)
    f = np.where(box_a | box_b, depth, f)
    return f.astype(np.float32)


def fan_mesh():
    """a non-manifold fan (three faces on the edge 0-1), two triangles that share only vertex 5, and a lone triangle"""
    verts = np.array([[0, 0, 0], [0, 0, 2], [2, 0, 1], [-1, 1.5, 1], [-1, -1.5, 1],
                      [5, 0, 0], [6, 1, 0], [6, -1, 0], [4, 1, 0.5], [4, -1, 0.5],
                      [8, 0, 0], [9, 0, 0], [8, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [5, 6, 7], [0, 1, 3], [10, 11, 12], [1, 0, 4], [5, 8, 9]], np.int64)
    return verts, faces
