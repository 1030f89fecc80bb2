"""Thin-plate-spline interpolation restated on the CPU: the checker for csrc/tps.hip, functional.tps_* and the 'tps' interpolation
mode of shape_model/point_cloud_registration.py.

Three things live here.
* The fp64 ORACLE: `system64`, `fit64`, `z64`, and the two routes from a fitted spline to samples -- `dense_route64` (the spline on
  the coarse lattice, torch's trilinear align_corners=True upsample to the whole image, torch's grid_sample, all in fp64: the
  reference's recipe) and `sparse_route64` (per sample the composite weights of both interpolations over at most 3 coarse nodes
  per axis, written out by hand: what the fused kernel does).  Distances are sums of squared differences.
* The fp32 YARDSTICK: `fit32`, `z32`, `route32`, the same formulas the way a straightforward fp32 composition writes them
  (distances expanded to ra + rb - 2 ab, an fp32 solve).  `rel_err(yardstick, oracle)` on an input is "the fp32 arithmetic's own
  error" there, and `bar(own)` = max(4.8e-7, 4 own) is what a kernel may be off by against the oracle.
* The seeded inputs and the case lists of tests/test_tps_cpu.py, tests/test_tps_gpu.py and tools/make_golden_tps.py.

u(r) = r^2 log(r + 1e-6).  theta (n+4, C): n spline weights, then the affine rows (1, x, y, z).  A lattice (D1, H1, W1) has its
nodes in z-major order with (x, y, z) coordinates, x along W1, at -1 + 2 i / (L - 1) rounded to fp32 (one node: 0)."""
import numpy as np
import torch
from torch.nn import functional as F

FLOOR = 4.8e-7            # 4 fp32 ulps: below it the comparison measures the rounding of the output itself
STEP, LAMBDA = 4, 0.1     # the reference's interpolate_displacements_tps
GRID_SHAPES = [(22, 30, 37), (20, 28, 36), (8, 9, 11)]   # fine sizes (D, H, W) on which the two routes are compared
ONE_NODE_SHAPE = (13, 6, 9)                              # 6 // 4 = 1: a coarse axis with a single node
GOLDEN_FIT = (5, 257)
GOLDEN_DENSE_SHAPE = (36, 28, 20)                        # (9, 7, 5) lattice
GOLDEN_IMG_SHAPES = [(22, 30, 37), (64, 64, 64)]         # img_shape = (D, H, W) in voxel units
GOLDEN_CORR_SHAPE = (256, 256, 256)                      # fixed_img_shape of the data_set_correspondences fixture


def rel_err(got, want):
    """largest deviation relative to the largest entry of `want`"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), np.finfo(np.float64).tiny))


def bar(own, factor=4):
    return max(FLOOR, factor * own)


# ------------------------------------------------------------------ inputs
def control_points(n, seed, duplicates=0):
    """(n,3) fp32 in [-0.9, 0.9]^3; the last `duplicates` rows repeat the first ones"""
    c = np.random.default_rng(seed).uniform(-0.9, 0.9, (n, 3)).astype(np.float32)
    if duplicates:
        c[n - duplicates:] = c[:duplicates]
    return c


def rough_values(n, C, seed):
    """(n,C) fp32, independent normal values: a rough field, large spline weights"""
    return np.random.default_rng(seed + 1).normal(0, 0.05, (n, C)).astype(np.float32)


def random_theta(n, C, seed):
    """(n+4,C) fp64: weights that sum to zero per channel (as a fit's do), affine rows of order one"""
    rng = np.random.default_rng(seed + 2)
    w = rng.normal(0, 1, (n, C))
    if n > 1:
        w -= w.mean(0)
    return np.concatenate([w, rng.normal(0, 1, (4, C))])


def queries(Q, seed, control=None):
    """(Q,3) fp32 in [-1,1]^3; with `control`, row 0 sits ON control point 0 (r = 0)"""
    q = np.random.default_rng(seed + 3).uniform(-1, 1, (Q, 3)).astype(np.float32)
    if control is not None:
        q[0] = control[0]
    return q


def far_queries():
    """|x| = 50: every u is about 1e4 while the weights sum to zero -- the cancellation case"""
    return np.array([[50., -50., 50.], [-50., 0.25, 0.], [0., 0., 50.]], np.float32)


def lattice(D1, H1, W1):
    """(D1 H1 W1, 3) fp32 nodes"""
    lin = lambda L: ((-1.0 + 2.0 * np.arange(L) / (L - 1)) if L > 1 else np.zeros(1)).astype(np.float32)   # noqa: E731
    z, y, x = np.meshgrid(lin(D1), lin(H1), lin(W1), indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3)


def sample_grid(size, seed, Q=40):
    """normalised sample coordinates (x,y,z) for a fine grid size = (D,H,W): the eight corners, the centres of seeded fine voxels
    (integer pixel positions), the outermost voxel centres, seeded points inside, points up to 1.5 voxels outside each face
    (partly in the zero padding) and points far outside (wholly in it) -> (Q', 3) fp32, and the rows that lie wholly outside"""
    D, H, W = size
    rng = np.random.default_rng(seed + 4)
    corners = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)
    vox = np.stack([rng.integers(0, L, 8) for L in (W, H, D)], 1)
    vox = np.concatenate([vox, [[0, 0, 0], [W - 1, H - 1, D - 1]]])
    centres = (2 * vox + 1) / np.array([W, H, D]) - 1
    inside = rng.uniform(-1, 1, (Q, 3))
    edge = rng.uniform(-1, 1, (12, 3))
    for k in range(12):   # one axis pushed up to 1.5 fine voxels beyond a face
        a = k % 3
        edge[k, a] = (1 + rng.uniform(0, 3) / (W, H, D)[a]) * (1 if k % 2 else -1)
    far = rng.uniform(-1, 1, (4, 3))
    far[:, 0] = [1.5, -1.5, 7., -1 - 2.01 / W]
    g = np.concatenate([corners, centres, inside, edge, far]).astype(np.float32)
    return g, np.arange(len(g) - 4, len(g))


def voxel_case(img_shape, n, Q, seed):
    """inputs of interpolate_displacements_tps for an image img_shape = (D,H,W): existing points (n,3) in voxel units,
    (x,y,z) with x in [0, W-1], rough displacements (n,3) of a few voxels, and Q sampling locations, the first ones on the
    corners of the volume and a few outside -> fp32 arrays"""
    D, H, W = img_shape
    rng = np.random.default_rng(seed + 5)
    hi = np.array([W - 1, H - 1, D - 1], np.float64)
    e = rng.uniform(0, 1, (n, 3)) * hi
    v = rng.normal(0, 2.0, (n, 3))
    q = rng.uniform(-0.05, 1.05, (Q, 3)) * hi
    k = min(Q, 8)
    q[:k] = (np.array([[sx, sy, sz] for sz in (0, 1) for sy in (0, 1) for sx in (0, 1)]) * hi)[:k]
    return e.astype(np.float32), v.astype(np.float32), q.astype(np.float32)


def normalise(e, v, q, img_shape):
    """the reference's normalisation, in fp32 as it (and the package) computes it: control = e / [W-1,H-1,D-1] * 2 - 1, values
    without the -1, samples like the control points -> fp32 arrays"""
    D, H, W = img_shape
    norm = torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float32)
    n = lambda a: (torch.from_numpy(np.asarray(a, np.float32)) / norm) * 2   # noqa: E731
    return (n(e) - 1).numpy(), n(v).numpy(), (n(q) - 1).numpy()


def unnormalise(s, img_shape):
    D, H, W = img_shape
    return np.asarray(s, np.float64) * np.array([H - 1, W - 1, D - 1], np.float64) / 2


# ------------------------------------------------------------------ fp64 oracle
def u(r):
    return r * r * np.log(r + 1e-6)


def dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = a[:, None, :] - b[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def system64(c, lambd):
    c = np.asarray(c, np.float64)
    n = len(c)
    A = np.zeros((n + 4, n + 4))
    A[:n, :n] = u(dist(c, c))
    A[np.arange(n), np.arange(n)] = lambd
    A[:n, n] = A[n, :n] = 1.0
    A[:n, n + 1:] = c
    A[n + 1:, :n] = c.T
    return A


def fit64(c, f, lambd):
    f = np.asarray(f, np.float64)
    rhs = np.zeros((len(c) + 4, f.shape[1]))
    rhs[:len(c)] = f
    return np.linalg.solve(system64(c, lambd), rhs)


def z64(x, c, theta):
    x, theta = np.asarray(x, np.float64), np.asarray(theta, np.float64)
    n = len(c)
    return u(dist(x, c)) @ theta[:n] + theta[n] + x @ theta[n + 1:]


def coarse_size(size, step=STEP):
    return tuple(s // step for s in size)


def dense_field64(c, theta, size, step=STEP):
    """the spline on the lattice, upsampled to size = (D,H,W) -> (C,D,H,W) fp64 tensor"""
    D1, H1, W1 = coarse_size(size, step)
    y2 = torch.from_numpy(z64(lattice(D1, H1, W1), c, theta)).view(1, D1, H1, W1, -1).permute(0, 4, 1, 2, 3)
    return F.interpolate(y2, tuple(size), mode="trilinear", align_corners=True)[0]


def dense_route64(c, theta, grid, size, step=STEP):
    """(Q,C): grid_sample(align_corners=False, zeros) of the dense field at grid (Q,3)"""
    g = torch.from_numpy(np.asarray(grid, np.float64)).view(1, -1, 1, 1, 3)
    out = F.grid_sample(dense_field64(c, theta, size, step)[None], g, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out.reshape(out.shape[1], -1).t().numpy()


def axis_weights(g, L, L1):
    """one axis of both interpolations: normalised coordinate g on L fine voxels over L1 coarse nodes -> {node: weight}"""
    pix = ((float(g) + 1.0) * L - 1.0) / 2.0
    i0 = int(np.floor(pix))
    f = pix - i0
    scale = (L1 - 1) / (L - 1) if L > 1 else 0.0
    w = {}
    for i, tw in ((i0, 1.0 - f), (i0 + 1, f)):
        if 0 <= i < L:
            src = scale * i
            j0 = min(int(src), L1 - 1)
            j1 = j0 + (1 if j0 < L1 - 1 else 0)
            lam = src - j0
            w[j0] = w.get(j0, 0.0) + tw * (1.0 - lam)
            w[j1] = w.get(j1, 0.0) + tw * lam
    return w


def sparse_route64(c, theta, grid, size, step=STEP):
    """(Q,C) by the composite weights, and the largest number of coarse nodes one sample touched"""
    D, H, W = size
    D1, H1, W1 = coarse_size(size, step)
    nodes = lattice(D1, H1, W1)
    theta = np.asarray(theta, np.float64)
    out, most = np.zeros((len(grid), theta.shape[1])), 0
    for s, g in enumerate(np.asarray(grid, np.float64)):
        wx, wy, wz = axis_weights(g[0], W, W1), axis_weights(g[1], H, H1), axis_weights(g[2], D, D1)
        assert all(max(w) - min(w) <= 2 for w in (wx, wy, wz) if w)
        idx = [(jz * H1 + jy) * W1 + jx for jz in wz for jy in wy for jx in wx]
        wts = np.array([(wz[jz] * wy[jy]) * wx[jx] for jz in wz for jy in wy for jx in wx])
        most = max(most, len(idx))
        if idx:
            out[s] = wts @ z64(nodes[idx], c, theta)
    return out, most


def interpolate64(e, v, q, img_shape, sparse=False):
    """interpolate_displacements_tps: fp32 normalisation (the input every implementation shares), then the fp64 dense route --
    or, for an image whose dense fp64 field would be large, the sparse route that equals it"""
    D, H, W = img_shape
    c, f, g = normalise(e, v, q, img_shape)
    theta = fit64(c, f, LAMBDA)
    return unnormalise(sparse_route64(c, theta, g, (W, H, D))[0] if sparse else dense_route64(c, theta, g, (W, H, D)), img_shape)


# ------------------------------------------------------------------ fp32 yardstick: a straightforward fp32 composition
def _u32(r):
    return r.square() * torch.log(r + 1e-6)


def _dist32(a, b):
    sq = a.square().sum(1)[:, None] + b.square().sum(1)[None, :] - 2.0 * (a @ b.t())
    return sq.clamp_(min=0.0).sqrt()


def fit32(c, f, lambd):
    c, f = (torch.from_numpy(np.asarray(a, np.float32)) for a in (c, f))
    n = len(c)
    A = torch.zeros(n + 4, n + 4)
    A[:n, :n] = _u32(_dist32(c, c)) + lambd * torch.eye(n)
    A[:n, n] = A[n, :n] = 1.0
    A[:n, n + 1:] = c
    A[n + 1:, :n] = c.t()
    rhs = torch.zeros(n + 4, f.shape[1])
    rhs[:n] = f
    return torch.linalg.solve(A, rhs).numpy()


def z32(x, c, theta):
    x, c, theta = (torch.from_numpy(np.asarray(a, np.float32)) for a in (x, c, theta))
    n = len(c)
    return (_u32(_dist32(x, c)) @ theta[:n] + theta[n] + x @ theta[n + 1:]).numpy()


def route32(c, f, grid, size, lambd=LAMBDA, step=STEP):
    """fit, lattice evaluation, upsample and grid_sample, all fp32 -> (Q,C)"""
    D1, H1, W1 = coarse_size(size, step)
    y2 = torch.from_numpy(z32(lattice(D1, H1, W1), c, fit32(c, f, lambd))).view(1, D1, H1, W1, -1).permute(0, 4, 1, 2, 3)
    field = F.interpolate(y2, tuple(size), mode="trilinear", align_corners=True)
    g = torch.from_numpy(np.asarray(grid, np.float32)).view(1, -1, 1, 1, 3)
    out = F.grid_sample(field, g, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out.reshape(out.shape[1], -1).t().numpy()


def interpolate32(e, v, q, img_shape):
    D, H, W = img_shape
    c, f, g = normalise(e, v, q, img_shape)
    return unnormalise(route32(c, f, g, (W, H, D)), img_shape)


# ------------------------------------------------------------------ the inputs of the recorded reference runs (tools/make_golden_tps.py)
def golden_fit_inputs(n):
    c = control_points(n, 100 + n)
    return c, rough_values(n, 3, 100 + n), queries(33, 100 + n, c)


def golden_dense_inputs():
    c = control_points(40, 300)
    idx = np.random.default_rng(301).integers(0, int(np.prod(GOLDEN_DENSE_SHAPE)), 256)
    return c, rough_values(40, 3, 300), idx


def golden_voxel_inputs(img_shape):
    return voxel_case(img_shape, 40 if img_shape[0] < 64 else 257, 50, 400 + img_shape[0])
