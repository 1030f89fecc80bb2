"""Checkers for csrc/kmeans.hip and functional.kmeans, numpy on the CPU.

* `sheets` / `pooled`: seeded inputs as the reference's 'kmeans' mode sees them -- I instances of P points on perturbed copies of
  one curved sheet, coordinates up to a few hundred (millimetres), concatenated per object.
* `lloyd64`: Lloyd's algorithm in fp64 (direct-form distances, first minimum, an empty cluster keeps its centre): the oracle.
* `Restatement`: the kernel restated BIT FOR BIT -- fp32 distances ((dx dx + dy dy) + dz dz) in that order, the lowest index on
  ties, int64 fixed-point sums at the per-item scales, the fp64 divide rounded to fp32, the empty-cluster rule, the stopping rule
  with the kernel's fixed-order fp64 reductions.  DESIGN.md ("k-means") states the same rules in words.
* `fps32`: farthest point sampling in fp32 (first point = row `start`, first maximum), for deterministic centres on the CPU.
"""
import numpy as np

MAX_K, MAX_POINTS = 4096, 1 << 24
RED_THREADS = 1024   # csrc/kmeans.hip: kRed, the width of the fixed-order fp64 reductions


# ------------------------------------------------------------------ inputs
def sheets(instances, P, seed, dtype=np.float32):
    """(instances, P, 3): every instance is its own sampling of z = 0.3 sin(2u) + 0.2 v^2 over [-1, 1]^2, scaled to about
    240 x 180 x 60 mm around (150, 120, 140), with a per-instance similarity perturbation and 0.5 mm of noise"""
    rng = np.random.default_rng(seed)
    out = np.empty((instances, P, 3))
    for i in range(instances):
        u, v = rng.uniform(-1, 1, P), rng.uniform(-1, 1, P)
        z = 0.3 * np.sin(2 * u) + 0.2 * v * v
        pts = np.stack([120 * u, 90 * v, 80 * z], 1)
        a = rng.normal(0, 0.03)
        R = np.array([[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]])
        pts = (1 + rng.normal(0, 0.02)) * pts @ R.T + rng.normal(0, 2., 3) + rng.normal(0, 0.5, (P, 3))
        out[i] = pts + np.array([150., 120., 140.])
    return out.astype(dtype)


def pooled(instances, P, seed, dtype=np.float32):
    """(instances * P, 3): the clouds of all instances concatenated, as generate_corresponding_points.py:44 pools them"""
    return sheets(instances, P, seed, dtype).reshape(instances * P, 3)


def fps32(points, K, start=0):
    """rows of K farthest-point samples of points (n,3), distances in fp32 direct form, first maximum on ties"""
    p = np.asarray(points, np.float32)
    rows = [int(start)]
    d = np.full(len(p), np.inf, np.float32)
    for _ in range(K - 1):
        q = p - p[rows[-1]]
        d = np.minimum(d, (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        rows.append(int(np.argmax(d)))
    return np.array(rows, np.int64)


# ------------------------------------------------------------------ inputs of data_set_correspondences
CORR_SEED, CORR_INSTANCES, CORR_OBJECTS, CORR_POINTS, CORR_GRID = 20260, 5, 2, 48, 9


class DuckMesh:
    """what the reference reads of an open3d TriangleMesh"""

    def __init__(self, vertices, triangles):
        self.vertices, self.triangles = vertices, triangles


def _sheet_z(u, v, amp, obj):
    return amp * np.sin(2 * u + obj) + 0.2 * v * v


def correspondence_inputs(seed=CORR_SEED, instances=CORR_INSTANCES, objects=CORR_OBJECTS, P=CORR_POINTS, grid=CORR_GRID):
    """seeded fp64 inputs in the layout the reference's driver loads them: dict(fixed_pcs (O,P,3), meshes [instance][object]
    DuckMesh, moving_pcs / moved_pcs / displacements (I,O,P,3), transforms: a list of dicts with scale, rotation, translation).
    Pre-registered = scale * rotation @ x + translation, moved = pre-registered + a smooth displacement; the moved clouds lie on
    the fixed sheet, an instance's mesh is the grid x grid triangulation of that sheet taken back to the moving space."""
    rng = np.random.default_rng(seed)
    cell = (np.arange(grid - 1)[:, None] * grid + np.arange(grid - 1)[None, :]).reshape(-1)
    faces = np.stack([np.stack([cell, cell + 1, cell + grid], 1), np.stack([cell + 1, cell + grid, cell + 1 + grid], 1)],
                     1).reshape(-1, 3).astype(np.int32)
    lin = np.linspace(-1, 1, grid)
    gu, gv = (a.reshape(-1) for a in np.meshgrid(lin, lin, indexing="ij"))
    offs = np.array([[150., 120., 140.], [170., 100., 90.]])[:objects]

    def lift(u, v, amp, obj):
        return np.stack([60 * u, 45 * v, 40 * _sheet_z(u, v, amp, obj)], 1) + offs[obj]

    fixed = np.stack([lift(rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), 0.3, o) for o in range(objects)])
    meshes, transforms = [], []
    moving = np.empty((instances, objects, P, 3))
    moved, disp = np.empty_like(moving), np.empty_like(moving)
    for i in range(instances):
        a, b = rng.normal(0, 0.2), rng.normal(0, 0.1)
        Rz = np.array([[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]])
        Rx = np.array([[1., 0., 0.], [0., np.cos(b), -np.sin(b)], [0., np.sin(b), np.cos(b)]])
        t = dict(scale=float(1 + rng.normal(0, 0.08)), rotation=Rz @ Rx, translation=rng.normal(0, 6., 3))
        transforms.append(t)
        meshes.append([])
        field = lambda q: np.stack([3 * np.sin(q[:, 1] / 25 + i), 2 * np.cos(q[:, 0] / 20), 0.02 * (q[:, 0] - 150)], 1)  # noqa: E731
        back = lambda q: ((q - t['translation']) / t['scale']) @ np.linalg.inv(t['rotation']).T                            # noqa: E731
        for o in range(objects):
            # a successful registration: the moved cloud lies on the fixed sheet (0.2 mm of noise), the displacement is a smooth
            # field of the moved position, and the instance's own surface is the fixed sheet taken back through both
            moved[i, o] = lift(rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), 0.3, o) + rng.normal(0, 0.2, (P, 3))
            disp[i, o] = field(moved[i, o])
            moving[i, o] = back(moved[i, o] - disp[i, o])
            grid_pts = lift(1.15 * gu, 1.15 * gv, 0.3, o)
            meshes[i].append(DuckMesh(back(grid_pts - field(grid_pts)), faces.copy()))
    return dict(fixed_pcs=fixed, meshes=meshes, moving_pcs=moving, moved_pcs=moved, displacements=disp, transforms=transforms)


def chamfer_pair(x, y):
    """pytorch3d.loss.chamfer_distance with its defaults for one pair of clouds (1,N,3), (1,M,3): squared distances, mean over the
    points, both directions added -- evaluated in fp64"""
    x, y = np.asarray(x, np.float64)[0], np.asarray(y, np.float64)[0]
    d = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    return d.min(1).mean() + d.min(0).mean()


# ------------------------------------------------------------------ fp64 oracle
def sq_dist(points, centres, dtype):
    """(n, K) squared distances ((dx dx + dy dy) + dz dz) evaluated in `dtype`, chunked over the points"""
    p, c = np.asarray(points, dtype), np.asarray(centres, dtype)
    out = np.empty((len(p), len(c)), dtype)
    for i0 in range(0, len(p), 1024):
        d = p[i0:i0 + 1024, None, :] - c[None, :, :]
        out[i0:i0 + 1024] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return out


def assign64(points, centres):
    """-> labels (first minimum), squared distance to the nearest and to the second nearest centre (inf for K = 1), fp64"""
    d = sq_dist(points, centres, np.float64)
    lab = d.argmin(1)
    best = d[np.arange(len(d)), lab]
    if d.shape[1] > 1:
        d[np.arange(len(d)), lab] = np.inf
        second = d.min(1)
    else:
        second = np.full(len(d), np.inf)
    return lab, best, second


def lloyd64(points, centres, max_iter=300, tol=1e-4):
    """Lloyd in fp64 from `centres`: an empty cluster keeps its centre; stops when no label changes, or the summed squared
    shift is <= tol * mean(var(points, 0)), or after max_iter iterations -> dict(centres, labels, inertia, n_iter, inertias);
    labels and inertia belong to the returned centres, inertias[t] to the centres iteration t started from"""
    p, c = np.asarray(points, np.float64), np.array(centres, np.float64)
    thr = tol * p.var(0).mean()
    prev, n_iter, inertias = None, 0, []
    for _ in range(max_iter):
        lab, best, _ = assign64(p, c)
        inertias.append(best.sum())
        cnt = np.bincount(lab, minlength=len(c))
        new = c.copy()
        for a in range(3):
            s = np.bincount(lab, weights=p[:, a], minlength=len(c))
            new[cnt > 0, a] = s[cnt > 0] / cnt[cnt > 0]
        shift = ((new - c) ** 2).sum()
        unchanged = prev is not None and np.array_equal(prev, lab)
        c, prev, n_iter = new, lab, n_iter + 1
        if unchanged or shift <= thr:
            break
    lab, best, _ = assign64(p, c)
    return dict(centres=c, labels=lab, inertia=best.sum(), n_iter=n_iter, inertias=inertias)


# ------------------------------------------------------------------ the kernel, bit for bit
def block_sum(values):
    """the kernel's fixed-order fp64 sum: thread t of RED_THREADS adds values[t], values[t + RED_THREADS], ... in that order,
    then the halving tree over the thread index"""
    v = np.asarray(values, np.float64)
    pad = (-len(v)) % RED_THREADS
    rows = np.concatenate([v, np.zeros(pad)]).reshape(-1, RED_THREADS)   # adding +0.0 changes no bit of a partial sum
    acc = np.zeros(RED_THREADS)
    for r in rows:
        acc = acc + r
    step = RED_THREADS // 2
    while step:
        acc[:step] = acc[:step] + acc[step:2 * step]
        step //= 2
    return float(acc[0])


def check_args(points, centres):
    p, c = np.asarray(points), np.asarray(centres)
    if p.ndim != 2 or p.shape[1] != 3 or c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"expected points (n,3) and centres (K,3), got {p.shape} and {c.shape}")
    n, K = len(p), len(c)
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"n={n} outside [1, {MAX_POINTS}]")
    if not 1 <= K <= min(n, MAX_K):
        raise ValueError(f"K={K} outside [1, min(n, {MAX_K})]")
    if not (np.isfinite(p).all() and np.isfinite(c).all()):
        raise ValueError("coordinates must be finite")
    return n, K


def scales(points, centres):
    """-> (s, si): x -> rint(x 2^s), d -> rint(d 2^si);  e = frexp exponent of the largest |coordinate| of points and
    centres (0 if that is 0), L = ceil(log2 n), s = 62 - L - e, si = 62 - L - (2 e + 4)"""
    m = max(float(np.abs(np.asarray(points, np.float32)).max()), float(np.abs(np.asarray(centres, np.float32)).max()))
    e = int(np.frexp(np.float32(m))[1]) if m > 0 else 0
    L = int(len(points) - 1).bit_length()
    return 62 - L - e, 62 - L - (2 * e + 4)


def to_fixed(x, s):
    """round half to even of x 2^s, evaluated in fp64 (where the product is exact)"""
    return np.rint(np.ldexp(np.asarray(x, np.float32).astype(np.float64), s)).astype(np.int64)


def threshold(points, tol):
    """tol * mean over the axes of the variance, two passes in the kernel's reduction order"""
    p = np.asarray(points, np.float32).astype(np.float64)
    n = len(p)
    var = []
    for a in range(3):
        mean = block_sum(p[:, a]) / n
        d = p[:, a] - mean
        var.append(block_sum(d * d) / n)
    return tol * (((var[0] + var[1]) + var[2]) / 3.0)


class Restatement:
    """one item of a run: `step()` is fsg_kmeans_step_f32, `assign()` fsg_kmeans_assign_f32"""

    def __init__(self, points, centres, tol=1e-4, prev_labels=None):
        self.n, self.K = check_args(points, centres)
        self.p = np.ascontiguousarray(points, np.float32)
        self.c = np.array(centres, np.float32)
        self.s, self.si = scales(self.p, self.c)
        self.thr = threshold(self.p, tol)
        self.fixed = to_fixed(self.p, self.s)
        self.labels = np.full(self.n, -1, np.int32) if prev_labels is None else np.asarray(prev_labels, np.int32).copy()
        self.active, self.n_iter = True, 0
        self.counts = self.inertia = self.n_changed = self.n_empty = self.shift = None

    def _assign(self):
        d = sq_dist(self.p, self.c, np.float32)
        lab = d.argmin(1).astype(np.int32)                  # numpy's argmin returns the first minimum
        best = d[np.arange(self.n), lab]
        self.n_changed = int((lab != self.labels).sum())
        self.labels = lab
        self.counts = np.bincount(lab, minlength=self.K).astype(np.int32)
        sums = np.zeros((self.K, 3), np.int64)
        np.add.at(sums, lab, self.fixed)
        self.inertia = float(np.ldexp(np.float64(to_fixed(best, self.si).sum()), -self.si))
        return sums

    def step(self):
        if not self.active:
            return
        sums = self._assign()
        new = self.c.copy()
        full = self.counts > 0
        new[full] = np.ldexp(sums[full].astype(np.float64) / self.counts[full, None].astype(np.float64), -self.s).astype(np.float32)
        d = new.astype(np.float64) - self.c.astype(np.float64)
        self.shift = block_sum((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        self.n_empty = int((~full).sum())
        self.c = new
        self.n_iter += 1
        if self.n_changed == 0 or self.shift <= self.thr:
            self.active = False

    def assign(self):
        self._assign()
        self.n_empty = int((self.counts == 0).sum())


def run(points, centres, max_iter=300, tol=1e-4):
    """functional.kmeans for one item -> dict(centres fp32, labels int64, inertia, n_iter, inertias, counts, n_empty)"""
    r = Restatement(points, centres, tol)
    inertias = []
    for _ in range(max_iter):
        if not r.active:
            break
        r.step()
        inertias.append(r.inertia)
    r.assign()
    return dict(centres=r.c, labels=r.labels.astype(np.int64), inertia=r.inertia, n_iter=r.n_iter, inertias=inertias,
                counts=r.counts, n_empty=r.n_empty)
