"""Point-cloud normal estimation restated in numpy, independent of the kernel's eigensolver (csrc/pcl_normals.hip uses cyclic
Jacobi; this uses numpy.linalg.eigh): brute-force stable-sorted kNN or given indices, the covariance of the k neighbours about
their mean, eigh, the majority rule applied literally.  `dtype` float64 is the reference, float32 the "fp32 restatement" whose
own error sets the bar (dpsr_oracle.bar).  Semantics: pytorch3d's ops/points_normals.py, restated (parity unpinned).

Shared seeded inputs for tests/test_normals_cpu.py, tests/test_normals_gpu.py and tests/test_dpsrnet_gpu.py live here too."""
import numpy as np

AXES = (0.8, 0.6, 0.5)
# (n, k, sigma) of the ellipsoid cases: the first three compare vectors and signs, the fourth (k = n - 1) and the fifth (odd k,
# genuine ties of the sign rule) vectors up to sign where the margin is small / everywhere
TABLE = [(512, 30, 0.005), (512, 16, 0.005), (256, 8, 0.002), (31, 30, 0.005), (96, 7, 0.002)]


# ------------------------------------------------------------------ inputs
def ellipsoid(n, sigma, seed=1, axes=AXES, centre=(0.0, 0.0, 0.0)):
    """n points on an ellipsoid (uniform directions scaled by the semi-axes) plus Gaussian noise sigma -> (n, 3) float32.
    The noise is drawn before the directions: with default_rng(1) in this order the fp64 oracle alone keeps every case of
    tests/test_normals_gpu.py inside its caps (at most 5 % of the points with gap < 0.05 or margin <= 2); with the directions
    first the (256, k = 8) case has 5.9 % of its points at margin <= 2."""
    rng = np.random.default_rng(seed)
    noise = rng.normal(scale=sigma, size=(n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * np.asarray(axes) + np.asarray(centre) + noise).astype(np.float32)


def sheet(n=512, sigma=0.002, seed=2):
    """a noisy flat sheet z ~ 0 over [-0.5, 0.5]^2"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, (n, 3))
    p[:, 2] = rng.normal(scale=sigma, size=n)
    return p.astype(np.float32)


def planar_grid(m=8, z=0.25):
    """m x m grid points with irregular (seeded) spacing in an exact plane z = const: no distance ties to speak of"""
    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(-0.5, 0.5, m))
    y = np.sort(rng.uniform(-0.5, 0.5, m))
    g = np.stack(np.meshgrid(x, y, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.full((m * m, 1), z)], 1).astype(np.float32)


RAGGED_SIZES = [3, 4, 10, 31, 257, 64]


def ragged(sizes=RAGGED_SIZES, sigma=0.005, seed=4):
    """one packed cloud of ellipsoid segments -> xyz (n, 3) float32, offset (b,) int32 cumulative ends"""
    parts = [ellipsoid(s, sigma, seed + i, centre=(0.05 * i, 0.0, 0.0)) for i, s in enumerate(sizes)]
    return np.concatenate(parts), np.cumsum(sizes).astype(np.int32)


# ------------------------------------------------------------------ the oracle
def knn(xyz, k):
    """(n, k) int64: the k nearest points of every point, itself included, by fp64 squared distance, stable order (ascending
    distance, the lower index first on ties; the point itself first)"""
    x = xyz.astype(np.float64)
    d2 = ((x[:, None] - x[None]) ** 2).sum(-1)
    d2[np.arange(len(x)), np.arange(len(x))] = -1.0
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def _flip(v, d, k):
    """the majority rule, literally: proj_j = v . (x_j - p); flip when #{proj_j > 0} < 0.5 k -> (v, n_pos before the flip)"""
    proj = (v[:, None, :] * d).sum(-1)
    n_pos = (proj > 0).sum(1)
    flip = n_pos < 0.5 * k
    return np.where(flip[:, None], -v, v), n_pos


def frames(xyz, k, idx=None, dtype=np.float64, disambiguate=True):
    """xyz (n, 3), one segment; idx (n, >= k) or None (own kNN) -> dict of
      normals (n, 3), curvatures (n, 3) ascending, frames (n, 3, 3) with columns (n, y = z x n, z),
      gap (n,) = (l1 - l0) / l2, gap_z (n,) = (l2 - l1) / l2, margin, margin_z (n,) = |2 n_pos - (k - 1)| of the sign rule for
      the normal and for z (k - 1 = the neighbours other than the point itself, whose projection is 0)"""
    idx = knn(xyz, k) if idx is None else np.asarray(idx)[:, :k]
    x = xyz.astype(dtype)
    nb = x[idx]                                               # (n, k, 3)
    mean = nb.mean(1, keepdims=True)
    c = nb - mean
    C = (c[:, :, :, None] * c[:, :, None, :]).mean(1)
    w, V = np.linalg.eigh(C)
    w, V = w.astype(dtype), V.astype(dtype)
    n, z = V[:, :, 0], V[:, :, 2]
    d = nb - x[:, None]
    k_eff = idx.shape[1]
    margin = margin_z = np.zeros(len(x), np.int64)
    if disambiguate:
        n, pn = _flip(n, d, k_eff)
        z, pz = _flip(z, d, k_eff)
        margin, margin_z = np.abs(2 * pn - (k_eff - 1)), np.abs(2 * pz - (k_eff - 1))
    y = np.cross(z, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
        gap_z = np.where(w[:, 2] > 0, (w[:, 2] - w[:, 1]) / w[:, 2], 0.0)
    return dict(normals=n, curvatures=w, frames=np.stack([n, y, z], -1), gap=gap, gap_z=gap_z, margin=margin, margin_z=margin_z,
                idx=idx)


def frames_packed(xyz, offset, K, idx=None, dtype=np.float64, disambiguate=True):
    """the packed form: every segment on its own with k_s = max(1, min(K, n_s - 1)); idx (n, K) global indices or None ->
    the same dict, concatenated, plus idx (n, K) int32 global, the columns beyond k_s filled with -1"""
    outs, st = [], 0
    for en in offset:
        en = int(en)
        ns = en - st
        if ns:
            ks = max(1, min(K, ns - 1))
            seg_idx = None if idx is None else np.asarray(idx)[st:en, :ks] - st
            o = frames(xyz[st:en], ks, seg_idx, dtype, disambiguate)
            full = np.full((ns, K), -1, np.int32)
            full[:, :ks] = o["idx"] + st
            o["idx"] = full
            o["k"] = np.full(ns, ks)
            outs.append(o)
        st = en
    return {key: np.concatenate([o[key] for o in outs]) for key in outs[0]}
