"""Marching cubes restated in numpy, vectorised over cells (a loop over the 256 cases, none over cells), in fp64 or fp32.  The
case table comes from the package's generator (fissure_segmentation_amd._mc_table), the orders are the canonical ones of
csrc/marching_cubes.hip -- vertices by (z, y, x, axis) of the lower node of their grid edge, faces by (cell, table order) --
so faces compare as exact integers.  The fp32 run performs the kernel's operations in the kernel's order:

  inside      = fp32(value) < fp32(isolevel)                                  (always decided in fp32: it is the method's topology)
  t           = (iso - v_a) / (v_b - v_a)
  position    = p_a + t (p_b - p_a),   p = 2 i / (S - 1) - 1 (local) or i * spacing
  face normal = (v1 - v0) x (v2 - v0), each component  a b - c d
  normal      = sum over the incident faces in face order, / max(sqrt((nx nx + ny ny) + nz nz), 1e-6)
"""
import numpy as np

from fissure_segmentation_amd._mc_table import CORNERS, EDGE_AXIS, EDGES, TRIANGLES


def _coord(i, S, local, sp, dtype):
    i = i.astype(dtype)
    if local:
        return dtype(2) * i / dtype(S - 1) - dtype(1)
    return i * dtype(sp)


def cell_cases(field, iso, mask=None):
    """field (D, H, W) -> (D - 1, H - 1, W - 1) uint8 cases; a cell with a corner outside the mask has case 0"""
    D, H, W = field.shape
    inside = field.astype(np.float32) < np.float32(iso)
    case = np.zeros((D - 1, H - 1, W - 1), np.uint8)
    active = np.ones(case.shape, bool)
    for c, (cx, cy, cz) in enumerate(CORNERS):
        sl = (slice(cz, D - 1 + cz), slice(cy, H - 1 + cy), slice(cx, W - 1 + cx))
        case |= inside[sl].astype(np.uint8) << c
        if mask is not None:
            active &= mask[sl] != 0
    return np.where(active, case, 0).astype(np.uint8)


def marching_cubes_item(field, iso=0.0, local=True, mask=None, dtype=np.float64, spacing=(1.0, 1.0, 1.0)):
    """one item: field (D, H, W) fp32 -> verts (V, 3) dtype in (x, y, z) columns, faces (F, 3) int64, normals (V, 3) dtype"""
    field = np.asarray(field, np.float32)
    D, H, W = field.shape
    case = cell_cases(field, iso, mask)
    # which grid edges carry a vertex: an active cell in which the edge's two corners differ
    used = np.zeros((D, H, W, 3), bool)
    for (a, b), axis in zip(EDGES, EDGE_AXIS):
        ax, ay, az = CORNERS[a]
        cross = ((case >> a) & 1) != ((case >> b) & 1)
        used[az:D - 1 + az, ay:H - 1 + ay, ax:W - 1 + ax, axis] |= cross
    vid = (np.cumsum(used.reshape(-1)) - 1).reshape(D, H, W, 3)
    z, y, x, axis = np.nonzero(used)
    step = [(axis == 0).astype(np.int64), (axis == 1).astype(np.int64), (axis == 2).astype(np.int64)]   # along x, y, z
    va = field[z, y, x].astype(dtype)
    vb = field[z + step[2], y + step[1], x + step[0]].astype(dtype)
    t = (dtype(np.float32(iso)) - va) / (vb - va)
    cols = []
    for k, (i, S) in enumerate(((x, W), (y, H), (z, D))):
        pa = _coord(i, S, local, spacing[k], dtype)
        pb = _coord(i + step[k], S, local, spacing[k], dtype)
        cols.append(np.where(step[k] == 1, pa + t * (pb - pa), pa))
    verts = np.stack(cols, 1).astype(dtype) if len(z) else np.zeros((0, 3), dtype)
    # faces, case by case
    rows = []
    lin = np.arange(D * H * W).reshape(D, H, W)[:D - 1, :H - 1, :W - 1]
    for c in range(1, 255):
        sel = case == c
        if not sel.any():
            continue
        cz, cy, cx = np.nonzero(sel)
        for k, tri in enumerate(TRIANGLES[c]):
            ids = []
            for e in tri:
                ox, oy, oz = CORNERS[EDGES[e][0]]
                ids.append(vid[cz + oz, cy + oy, cx + ox, EDGE_AXIS[e]])
            rows.append(np.stack([lin[sel], np.full(len(cz), k)] + ids, 1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
        faces = rows[:, 2:].astype(np.int64)
    else:
        faces = np.zeros((0, 3), np.int64)
    return verts, faces, vertex_normals(verts, faces)


def vertex_normals(verts, faces):
    dtype = verts.dtype.type
    n = np.zeros_like(verts)
    if len(faces):
        v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
        a, b = v1 - v0, v2 - v0
        fn = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                       a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        np.add.at(n, faces.reshape(-1), np.repeat(fn, 3, axis=0))      # unbuffered: in face order
    norm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n / np.maximum(norm, dtype(1e-6))[:, None]


def marching_cubes(field, iso=0.0, local=True, mask=None, dtype=np.float64, spacing=(1.0, 1.0, 1.0)):
    """field (B, D, H, W) -> lists of per-item verts, faces, normals"""
    out = [marching_cubes_item(f, iso, local, None if mask is None else mask[b], dtype, spacing) for b, f in enumerate(field)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def packed(lists, width=3, dtype=None):
    return np.concatenate(lists) if lists else np.zeros((0, width), dtype)


def directed_edge_defect(faces):
    """(number of directed edges that occur more than once, number whose reverse does not occur exactly once)"""
    he = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    V = int(faces.max()) + 1 if len(faces) else 1
    key, cnt = np.unique(he[:, 0] * V + he[:, 1], return_counts=True)
    rev = np.isin(he[:, 1] * V + he[:, 0], key)
    return int((cnt > 1).sum()), int((~rev).sum())


def euler_characteristic(faces):
    he = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    E = len(np.unique(he, axis=0))
    return len(np.unique(faces)) - E + len(faces)


def signed_volume(verts, faces):
    v0, v1, v2 = (verts[faces[:, k]].astype(np.float64) for k in range(3))
    return float(np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6)
