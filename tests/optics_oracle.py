"""Oracle of the OPTICS port (csrc/optics.hip, shape_model/optics.py): the rule of the kernel restated bit for bit in numpy,
twice -- `graph_brute` with the whole (n, n) matrix of squared distances, `graph` with KD-tree candidates and a heap --, the
inputs of the tests and the host pipeline from a graph to cluster centroids.

The rule: d2(i, j) = ((dx dx + dy dy) + dz dz) in fp64 in that order with dx = (double) x_i - (double) x_j; e2 = eps eps;
N(i) = { j : d2 <= e2 }, i included; core2(i) = the k-th smallest d2 over N(i) (i itself is the first), +inf if |N(i)| < k;
reach2 = +inf, pred = -1; n times: p = the unprocessed point with the smallest (reach2, index), lowest index on ties; p is
appended; if core2(p) < inf every unprocessed q in N(p) with v = max(core2(p), d2(p, q)) < reach2(q) gets reach2(q) = v and
pred(q) = p.  Squares everywhere; numpy's element-wise fp64 arithmetic neither fuses nor reorders."""
import heapq

import numpy as np

BRUTE_MAX = 2048


def _check(X, k, eps):
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != 3 or X.dtype != np.float32 or not np.isfinite(X).all():
        raise ValueError(f"points must be finite fp32 (n, 3), got {X.shape} {X.dtype}")
    n = len(X)
    if not 2 <= k <= n:
        raise ValueError(f"min_samples={k} must be in 2 .. n={n}")
    eps = np.float64(eps)
    if not eps > 0:
        raise ValueError(f"max_eps={eps} must be positive")
    return X.astype(np.float64), n, eps * eps


def d2_to(X64, i, idx):
    """squared distances of point i to the points idx, in the rule's order of operations"""
    dx, dy, dz = X64[i, 0] - X64[idx, 0], X64[i, 1] - X64[idx, 1], X64[i, 2] - X64[idx, 2]
    return (dx * dx + dy * dy) + dz * dz


def _result(order, core2, reach2, pred):
    return dict(ordering=np.asarray(order, np.int64), core2=core2, reach2=reach2, pred=pred)


def graph_brute(X, k, eps):
    """the rule with the full matrix, n <= BRUTE_MAX -> dict(ordering int64, core2, reach2 fp64, pred int64)"""
    X64, n, e2 = _check(X, k, eps)
    if n > BRUTE_MAX:
        raise ValueError(f"graph_brute is for n <= {BRUTE_MAX}")
    all_idx = np.arange(n)
    D = np.stack([d2_to(X64, i, all_idx) for i in range(n)])
    inside = D <= e2
    core2 = np.full(n, np.inf)
    for i in range(n):
        near = np.sort(D[i, inside[i]])
        if len(near) >= k:
            core2[i] = near[k - 1]
    reach2, pred, done, order = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, bool), []
    for _ in range(n):
        left = np.flatnonzero(~done)
        p = int(left[np.argmin(reach2[left])])   # the first minimum: the lowest index on ties
        done[p] = True
        order.append(p)
        if core2[p] < np.inf:
            q = np.flatnonzero(inside[p] & ~done)
            v = np.maximum(core2[p], D[p, q])
            better = v < reach2[q]
            reach2[q[better]] = v[better]
            pred[q[better]] = p
    return _result(order, core2, reach2, pred)


def graph(X, k, eps):
    """the same rule for any n: candidates from scipy's KD-tree (a ball a little larger than eps), re-tested with the rule's own
    d2 <= e2; the arg-min is a heap of (reach2, index) with lazy deletion"""
    from scipy.spatial import cKDTree
    X64, n, e2 = _check(X, k, eps)
    if np.isinf(e2):
        cand = None
    else:
        r = float(np.sqrt(e2)) * (1 + 1e-9) + 1e-300
        cand = cKDTree(X64).query_ball_point(X64, r, return_sorted=True)
    all_idx = np.arange(n)
    near, near_d2, core2 = [None] * n, [None] * n, np.full(n, np.inf)
    for i in range(n):
        idx = all_idx if cand is None else np.asarray(cand[i], np.int64)
        d = d2_to(X64, i, idx)
        keep = d <= e2
        near[i], near_d2[i] = idx[keep], d[keep]
        if len(near[i]) >= k:
            core2[i] = np.partition(near_d2[i], k - 1)[k - 1]
    reach2, pred, done, order = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, bool), []
    heap = [(np.inf, i) for i in range(n)]   # already a heap: equal keys, ascending indices
    while len(order) < n:
        _, p = heapq.heappop(heap)
        if done[p]:
            continue   # an entry that a later, smaller one of the same point has overtaken
        done[p] = True
        order.append(p)
        if core2[p] < np.inf:
            q, d = near[p], near_d2[p]
            v = np.maximum(core2[p], d)
            better = (v < reach2[q]) & ~done[q]
            reach2[q[better]] = v[better]
            pred[q[better]] = p
            for vv, qq in zip(v[better].tolist(), q[better].tolist()):
                heapq.heappush(heap, (vv, qq))
    return _result(order, core2, reach2, pred)


def same_graph(a, b):
    return all(np.array_equal(np.asarray(a[f]).view(np.int64) if np.asarray(a[f]).dtype == np.float64 else np.asarray(a[f]),
                              np.asarray(b[f]).view(np.int64) if np.asarray(b[f]).dtype == np.float64 else np.asarray(b[f]))
               for f in ("ordering", "core2", "reach2", "pred"))


# ------------------------------------------------------------------ inputs
def heuristic_eps(X):
    """the reference's max_eps: 5 % of the range of all coordinates of the pool (generate_corresponding_points.py:52)"""
    X = np.asarray(X, np.float64)
    return float((X.max() - X.min()) * 0.05)


def sheet(n, seed, noise=0.5, outliers=0, size=100.0):
    """a curved sheet with Gaussian noise across it and `outliers` uniform points in its bounding cube"""
    rng = np.random.default_rng(seed)
    m = n - outliers
    u, v = rng.uniform(0, size, m), rng.uniform(0, size, m)
    z = 0.1 * size * np.sin(u / size * 3.0) * np.cos(v / size * 2.0) + rng.normal(0, noise, m)
    pts = np.stack([u, v, z], 1)
    if outliers:
        pts = np.concatenate([pts, rng.uniform(-0.3 * size, 1.3 * size, (outliers, 3))])
    return pts[rng.permutation(n)].astype(np.float32)


def blobs(n, seed, centres=4, spread=2.0, outliers=0, size=100.0):
    """Gaussian blobs of different widths around random centres, plus uniform outliers"""
    rng = np.random.default_rng(seed)
    m = n - outliers
    c = rng.uniform(0, size, (centres, 3))
    which = rng.integers(0, centres, m)
    pts = c[which] + rng.normal(0, 1, (m, 3)) * (spread * (1 + which))[:, None]
    if outliers:
        pts = np.concatenate([pts, rng.uniform(0, size, (outliers, 3))])
    return pts[rng.permutation(n)].astype(np.float32)


def pooled(instances, points, seed, jitter=0.6):
    """what data_set_correspondences pools: `instances` noisy copies of one sheet of `points` points"""
    rng = np.random.default_rng(seed)
    base = sheet(points, seed + 1000, noise=0.0).astype(np.float64)
    return (base[None] + rng.normal(0, jitter, (instances, points, 3))).reshape(-1, 3).astype(np.float32)


def lattice(nx, ny=1, nz=1, spacing=1.0):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g * spacing).astype(np.float32)


# (name, points, min_samples, eps): the five kinds of input the rule was checked on against sklearn, n <= BRUTE_MAX
def cpu_cases():
    return [
        ("tight_sheet_k5", sheet(1536, 1, noise=0.2), 5, heuristic_eps(sheet(1536, 1, noise=0.2))),
        ("loose_sheet_k8", sheet(1800, 2, noise=3.0), 8, 9.0),
        ("sheet_outliers_k4", sheet(2048, 3, noise=0.5, outliers=200), 4, 8.0),
        ("blobs_k2", blobs(1600, 4, centres=5, outliers=100), 2, 6.0),
        ("pooled_k6_inf", pooled(12, 128, 5), 6, np.inf),
    ]


# ------------------------------------------------------------------ the host pipeline: graph -> labels -> centroids
def centroids_sequential(X, labels):
    """mean of every cluster in fp64, the points added one after the other in ascending order"""
    X64 = np.asarray(X, np.float64)
    C = int(labels.max()) + 1 if len(labels) else 0
    sums, counts = np.zeros((C, 3)), np.zeros(C, np.int64)
    for i in range(len(X64)):
        if labels[i] >= 0:
            sums[labels[i]] = sums[labels[i]] + X64[i]
            counts[labels[i]] += 1
    return sums / counts[:, None].astype(np.float64)


def pipeline(X, k, eps, xi=0.05):
    """oracle graph -> square roots on the host -> the package's xi extraction -> sequential fp64 means"""
    from fissure_segmentation_amd.shape_model.optics import optics_xi_labels
    g = graph(X, k, eps)
    labels = optics_xi_labels(np.sqrt(g["reach2"]), g["pred"], g["ordering"], k, xi=xi)
    return centroids_sequential(X, labels), labels
