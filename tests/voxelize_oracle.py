"""CPU oracle of the mesh -> label map conversions (csrc/voxelize.hip), fp64, written from the geometry.

* `distances` / `check_dist`: the distance of every voxel centre to every mesh through metrics_oracle.point_mesh_dist2, and
  the rule a distance label map is held to: exact, except where the fp64 distance is within a tolerance of the threshold
  (0 or the label) or where two meshes are within a tolerance of each other (either label).
* `tri_box_overlap`: triangle against axis-aligned box by separating axes (3 box axes, the face normal, 9 cross products of
  a box axis and an edge), with the box's half size as an argument so that it can be shrunk and grown, and with the
  half-open reading [lo, hi) of the box axes that floor(x / spacing) means.  A triangle without area needs no case: its
  projections are those of its longest edge and its normal, 0, separates nothing.
* `cover` / `check_cover`: the cells a set of meshes passes through and the rule a coverage map is held to.
* `sample_surface` / `sampled_labelmap`: the reference's route restated (data_processing/surface_fitting.py:19-39,
  :144-169): seeded uniform surface samples, floor(sample / spacing), out-of-range dropped, later meshes overwrite.
* the seeded inputs shared by the tests and tools/make_golden_voxelize.py.
"""
import numpy as np
import torch

import metrics_oracle as mo

SHAPE = (24, 20, 28)
SPACING = (1.25, 0.8, 1.0)        # volume order: non-cubic and anisotropic, so a swapped axis cannot pass
SHEETS = ((1, 0.6), (2, -0.7), (3, 0.1))   # (seed, tilt)
SHEET_N = 11                       # 11 x 11 vertices, 200 faces
DIST_TOL = 1e-3                    # mm: 10 x the 1e-4 the same arithmetic is held to in test_metrics_gpu.py
COVER_TOL = 1e-3                   # by which a cell is shrunk / grown per side
EXCUSED_SHARE = 0.01               # of the oracle's labelled voxels
N_SAMPLES = 200_000
MASK_SEED, SAMPLE_SEED = 1301, 1302


def extent(shape=SHAPE, spacing=SPACING):
    return [n * s for n, s in zip(shape, spacing)]


def sheet(seed, tilt, shape=SHAPE, spacing=SPACING, n=SHEET_N):
    """(verts (n*n, 3) fp64 in volume order, faces (2 (n-1)^2, 3)): a noisy tilted sheet across axes 1 and 2 that leaves the
    volume on all sides.

    The noise array is drawn (n, n) and indexed [along axis 2, along axis 1].  Of the two layouts of the same stream this is
    the one under which every sheet of SHEETS meets the precondition of the coverage tests -- the cells whose answer depends
    on +-COVER_TOL are at most 1 % of the labelled ones: 10 / 1129, 3 / 1234, 3 / 804 against 12 / 1126, 8 / 1229, 0 / 809
    the other way round.  That is a property of these inputs and of the fp64 oracle alone, no kernel is involved in it, and
    tests/test_voxelize_cpu.py pins it."""
    e0, e1, e2 = extent(shape, spacing)
    u, v = np.meshgrid(np.linspace(-1.3, e1 + 1.3, n), np.linspace(-1.3, e2 + 1.3, n), indexing="ij")
    rng = np.random.default_rng(seed)
    h = e0 * (0.5 + tilt * (u / e1 - 0.5) + 0.12 * np.sin(5.1 * v / e2 + seed)) + 0.3 * rng.random((n, n)).T
    return np.stack([h, u, v], -1).reshape(-1, 3) + 0.0137, mo.plane_faces(n)


def sheets():
    return [sheet(seed, tilt) for seed, tilt in SHEETS]


def random_mask(shape=SHAPE, seed=MASK_SEED):
    return np.random.default_rng(seed).random(shape) < 0.6


def voxel_centres(shape, spacing):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    return idx * np.asarray(spacing, dtype=np.float64)


# ---------------------------------------------------------------- distance band
def distances(meshes, shape, spacing):
    """(M, voxels) fp64 distance of every voxel centre to every mesh; Inf for a mesh without vertices or faces"""
    q = voxel_centres(shape, spacing)
    out = np.full((len(meshes), len(q)), np.inf)
    for m, (verts, faces) in enumerate(meshes):
        if len(verts) and len(faces):
            out[m] = mo.point_mesh_dist2(q, verts, faces)[0].sqrt().numpy()
    return out


def labelmap_dist(dist, shape, threshold, mask=None):
    """the label map of the definition: 1 + argmin (lowest on ties) where the minimum is <= threshold and the mask is set"""
    best = dist.argmin(0)
    lab = np.where(dist.min(0) <= threshold, best + 1, 0).reshape(shape)
    return lab if mask is None else np.where(mask, lab, 0)


def check_dist(got, dist, shape, threshold, mask=None, tol=DIST_TOL):
    """`got` against the distance label map -> (labelled voxels of the oracle, excused voxels, voxels of `got` that carry a value
    the rule does not allow, the excused voxels as a bool volume)"""
    got = np.asarray(got).reshape(-1)
    want = labelmap_dist(dist, shape, threshold, mask).reshape(-1)
    dmin = dist.min(0)
    allowed = np.zeros((dist.shape[0] + 1, dist.shape[1]), dtype=bool)          # [label, voxel]
    allowed[want, np.arange(len(want))] = True
    near_thr = np.abs(dmin - threshold) <= tol
    allowed[0] |= near_thr
    for m in range(dist.shape[0]):                                               # within tol of the nearest: may win
        allowed[m + 1] |= (dist[m] - dmin <= tol) & (dist[m] <= threshold + tol)
    if mask is not None:
        allowed[1:, ~np.asarray(mask).reshape(-1)] = False
        allowed[0, ~np.asarray(mask).reshape(-1)] = True
    excused = allowed.sum(0) > 1
    ok = (got >= 0) & (got <= dist.shape[0]) & allowed[np.clip(got, 0, dist.shape[0]), np.arange(len(got))]
    return int((want != 0).sum()), int(excused.sum()), int((~ok).sum()), excused.reshape(shape)


# ---------------------------------------------------------------- triangle against box
def tri_box_overlap(tri, centre, half, half_open=False):
    """tri (F,3,3), centre (C,3), half (3,) fp64 -> (C,F) bool: does triangle f meet the box centre[c] +- half?  Closed box,
    or with `half_open` the box [centre - half, centre + half) along its own three axes."""
    tri, centre, half = np.asarray(tri, dtype=np.float64), np.asarray(centre, dtype=np.float64), np.asarray(half, dtype=np.float64)
    v = tri[None] - centre[:, None, None, :]                                      # (C,F,3 vertices,3)
    lo, hi = v.min(2), v.max(2)
    if half_open:
        hit = ((lo < half) & (hi >= -half)).all(-1)
    else:
        hit = ((lo <= half) & (hi >= -half)).all(-1)
    edges = tri[:, [1, 2, 0]] - tri                                               # (F,3 edges,3)
    axes = [np.cross(edges[:, 0], edges[:, 1])]                                   # the normal
    for k in range(3):
        for unit in np.eye(3):
            axes.append(np.cross(unit[None], edges[:, k]))
    for a in axes:                                                                # (F,3)
        p = (v * a[None, :, None, :]).sum(-1)                                     # (C,F,3)
        rad = (np.abs(a) * half).sum(-1)[None]
        hit &= ~((p.min(-1) > rad) | (p.max(-1) < -rad))
    return hit


def cover_hits(verts, faces, shape, spacing, grow=0.0):
    """bool `shape`: the cells that a triangle of the mesh meets; grow 0: the half-open cell, else the closed cell grown
    (shrunk, if negative) by `grow` per side.  Face by face over the cells around the face's bounding box (one cell of
    margin; the test itself decides)."""
    out = np.zeros(shape, dtype=bool)
    if not (len(verts) and len(faces)):
        return out
    s = np.asarray(spacing, dtype=np.float64)
    for tri in np.asarray(verts, dtype=np.float64)[np.asarray(faces)]:
        first = np.maximum(np.floor(tri.min(0) / s).astype(np.int64) - 1, 0)
        last = np.minimum(np.floor(tri.max(0) / s).astype(np.int64) + 1, np.asarray(shape) - 1)
        if (first > last).any():
            continue
        idx = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(first, last)], indexing="ij"), -1).reshape(-1, 3)
        hit = tri_box_overlap(tri[None], (idx + 0.5) * s, s / 2 + grow, half_open=grow == 0.0)[:, 0]
        out[idx[hit, 0], idx[hit, 1], idx[hit, 2]] = True
    return out


def cover_bounds(meshes, shape, spacing, tol=COVER_TOL):
    """per mesh (must, may): the cells hit with the cell shrunk by tol (must be labelled) and grown by tol (may be)"""
    return [(cover_hits(v, f, shape, spacing, -tol), cover_hits(v, f, shape, spacing, tol)) for v, f in meshes]


def check_cover(got, bounds):
    """`got` against the coverage rule, the highest label winning: -> (labelled, excused, wrong) counts.  A cell is excused
    where the shrunk and the grown cell disagree for a mesh that could decide its label."""
    got = np.asarray(got)
    lo = np.zeros(got.shape, dtype=np.int64)     # the label if only the certain hits counted
    hi = np.zeros(got.shape, dtype=np.int64)     # the label if every possible hit counted
    for m, (must, may) in enumerate(bounds):
        lo[must] = m + 1
        hi[may] = m + 1
    ok = np.zeros(got.shape, dtype=bool)
    # allowed: lo itself, or the label of a mesh above lo whose hit is possible but not certain
    ok |= got == lo
    for m, (must, may) in enumerate(bounds):
        ok |= (got == m + 1) & may & (m + 1 >= lo)
    return int((lo != 0).sum()), int((lo != hi).sum()), int((~ok).sum())


# ---------------------------------------------------------------- the reference's sampling, restated
def sample_surface(verts, faces, n, seed):
    """n points uniform on the surface, fp64: faces in proportion to their area, uniform barycentric coordinates"""
    rng = np.random.default_rng(seed)
    tri = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    pick = rng.choice(len(tri), n, p=area / area.sum())
    r, t = np.sqrt(rng.random(n)), rng.random(n)
    w = np.stack([1 - r, r * (1 - t), r * t], 1)
    return (tri[pick] * w[:, :, None]).sum(1)


def sampled_labelmap(meshes, shape, spacing, n=N_SAMPLES, seed=SAMPLE_SEED):
    """floor(sample / spacing) scattered mesh after mesh (later ones overwrite), samples outside the volume dropped"""
    out = np.zeros(shape, dtype=np.int64)
    for m, (verts, faces) in enumerate(meshes):
        if not (len(verts) and len(faces)):
            continue
        idx = np.floor(sample_surface(verts, faces, n, seed + m) / np.asarray(spacing)).astype(np.int64)
        idx = idx[((idx >= 0) & (idx < np.asarray(shape))).all(1)]
        out[idx[:, 0], idx[:, 1], idx[:, 2]] = m + 1
    return out


# ---------------------------------------------------------------- inputs of mask_to_points / points_to_label_map
UTIL_SEED, UTIL_SHAPE, UTIL_SPACING_XYZ = 1303, (6, 7, 5), (0.8, 1.25, 1.5)


def util_inputs():
    """(mask (D,H,W) bool, points (N,3) fp32 xyz with one point per voxel at most, some outside the volume, labels (N,) int64)"""
    rng = np.random.default_rng(UTIL_SEED)
    mask = rng.random(UTIL_SHAPE) < 0.2
    d, h, w = UTIL_SHAPE
    outside = [[-2.2, 1.0, 1.1], [d + 1.4, 2.2, 0.1], [1.1, h + 3.0, w + 0.2]]          # clamped into (0,1,1), (d-1,2,0), (1,h-1,w-1)
    taken = np.ravel_multi_index(([0, d - 1, 1], [1, 2, h - 1], [1, 0, w - 1]), UTIL_SHAPE)
    vox = rng.permutation(d * h * w)
    vox = vox[~np.isin(vox, taken)][:40]
    zyx = np.stack(np.unravel_index(vox, UTIL_SHAPE), 1).astype(np.float64) + rng.uniform(-0.3, 0.3, (40, 3))
    zyx[:3] = outside
    pts = (zyx[:, ::-1] * np.asarray(UTIL_SPACING_XYZ)).astype(np.float32)
    return mask, pts, rng.integers(1, 4, 40).astype(np.int64)
