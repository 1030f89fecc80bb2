"""fp64 restatement of the reference's random walker and lobes-to-fissures (data_processing/random_walk.py:15-116,
find_lobes.py:17-88) in numpy / scipy, for the tests of csrc/random_walk.hip.

The matrix entries are the reference's fp32 values (its weights and degrees are fp32 tensors); everything downstream of them
-- the blocks, the direct solve, the residuals -- is fp64.  The reference solves with a pyamg Ruge-Stueben hierarchy stopped at
a relative tolerance of 1e-3; pyamg is not a dependency here, so THAT iterate is not pinned: the yardstick is the direct solve
(scipy's splu) of the same system, and `pcg` is the same Jacobi-preconditioned conjugate-gradient recurrence as the kernels in
a chosen dtype (its fp32 run is the error an fp32 solver is allowed)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl
import torch

SIGMA = 8.0
DIRECT_SOLVE_MAX_UNKNOWNS = 15000


def edge_weights(a, b, mode):
    """fp32 weights of the edges between the voxel values a and b (random_walk.py:47-55)"""
    if mode == "intensity":   # torch's fp32 exp, as the reference evaluates it
        ta, tb = torch.from_numpy(np.ascontiguousarray(a, np.float32)), torch.from_numpy(np.ascontiguousarray(b, np.float32))
        return torch.exp(-(ta - tb).pow(2) / (2 * 8 ** 2)).numpy()
    if mode == "binary":
        return np.where(a == b, np.float32(1.0), np.float32(0.01))
    raise ValueError(f'No edge weights named "{mode}" known.')


def laplacian(im, mode):
    """L = diag(1e-5 + deg) - A over all voxels of an n-d image -> csr fp64 holding the fp32 values.  The degree is the fp32
    sum of a voxel's weights.  No fixed neighbour order reproduces the last bit of the reference's degrees (it sums a torch
    sparse matrix), so the degree alone is taken from the same torch call on the same per-axis sum of sparse matrices."""
    im = np.asarray(im)
    n = im.size
    ind = np.arange(n).reshape(im.shape)
    rows, cols, vals = [], [], []
    At = None
    for d in range(im.ndim):
        lo = [slice(None)] * im.ndim
        hi = [slice(None)] * im.ndim
        lo[d], hi[d] = slice(None, -1), slice(1, None)
        i, j = ind[tuple(lo)].ravel(), ind[tuple(hi)].ravel()
        w = edge_weights(im[tuple(lo)].ravel(), im[tuple(hi)].ravel(), mode).astype(np.float32)
        rows += [i, j]
        cols += [j, i]
        vals += [w, w]
        a = torch.sparse_coo_tensor(torch.from_numpy(np.stack((i, j))), torch.from_numpy(w), (n, n))
        a = a + a.t()
        At = a if At is None else At + a
    deg = torch.sparse.sum(At, 0).to_dense().numpy()
    A = sp.csr_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    diag = (np.float32(1e-5) + deg).astype(np.float64)
    return (sp.diags(diag) - A).tocsr()


def blocks(L, labels, mask=None, num_labels=None):
    """random_walk.py:91-111 -> dict(Lu csc, b (n_unknown, K) = -B^T onehot, xu, xs, onehot (n_seeded, K), K)"""
    lab = np.asarray(labels).ravel()
    m = np.ones(lab.size, bool) if mask is None else np.asarray(mask).ravel() != 0
    seeded = (lab != 0) & m
    xs, xu = np.where(seeded)[0], np.where(~seeded & m)[0]
    K = int(lab[xs].max()) if num_labels is None else int(num_labels)
    onehot = np.zeros((xs.size, K))
    onehot[np.arange(xs.size), lab[xs] - 1] = 1.0
    Lr = L.tocsr()[xu]
    return dict(Lu=Lr[:, xu].tocsc(), b=-(Lr[:, xs] @ onehot), xu=xu, xs=xs, onehot=onehot, K=K)


def direct_solve(blk):
    if blk["xu"].size > DIRECT_SOLVE_MAX_UNKNOWNS:
        raise ValueError(f"{blk['xu'].size} unknowns: the direct solve is meant for at most {DIRECT_SOLVE_MAX_UNKNOWNS}")
    return spl.splu(blk["Lu"]).solve(blk["b"])


def pcg(A, b, tol, dtype=np.float64, max_iter=20000):
    """Jacobi-preconditioned conjugate gradients from x = 0 on one right-hand side, vectors in `dtype`, dot products in fp64;
    stops at |r| <= tol |b| on the recurrence's r -> (x, iterations)"""
    A = A.tocsr().astype(dtype)
    b = b.astype(dtype)
    dinv = (1 / A.diagonal()).astype(dtype)
    x, r = np.zeros_like(b), b.copy()
    bb = float(b.astype(np.float64) @ b.astype(np.float64))
    if bb == 0.0:
        return x, 0
    p = np.zeros_like(b)
    rz_old, beta = 1.0, 0.0
    for it in range(max_iter):
        z = dinv * r
        rz = float(r.astype(np.float64) @ z.astype(np.float64))
        if it:
            beta = rz / rz_old
        p = z + dtype(beta) * p
        q = A @ p
        alpha = rz / float(p.astype(np.float64) @ q.astype(np.float64))
        x = x + dtype(alpha) * p
        r = r - dtype(alpha) * q
        rz_old = rz
        if float(r.astype(np.float64) @ r.astype(np.float64)) <= tol * tol * bb:
            return x, it + 1
    return x, max_iter


def pcg_all(blk, tol, dtype=np.float64):
    cols = [pcg(blk["Lu"], blk["b"][:, k], tol, dtype) for k in range(blk["K"])]
    return np.stack([c[0] for c in cols], 1).astype(np.float64), [c[1] for c in cols]


def probabilities(blk, X, shape):
    """random_walk.py:113-116: (*shape, K) with the one-hot rows at seeds, X at unknowns, 0 elsewhere"""
    prob = np.zeros((int(np.prod(shape)), blk["K"]))
    prob[blk["xs"]] = blk["onehot"]
    prob[blk["xu"]] = X
    return prob.reshape(*shape, blk["K"])


def true_residuals(blk, X):
    """|b - Lu x| / |b| per system in fp64 (0 for an all-zero right-hand side)"""
    res = np.linalg.norm(blk["b"] - blk["Lu"] @ X, axis=0)
    nb = np.linalg.norm(blk["b"], axis=0)
    return np.where(nb > 0, res / np.where(nb > 0, nb, 1), 0.0)


def fill_lobes(prob, mask):
    """find_lobes.py:27: first-index argmax + 1 inside the mask, 0 outside"""
    return np.where(np.asarray(mask) != 0, prob.argmax(-1) + 1, 0)


def top_two_gap(prob):
    s = np.sort(prob, -1)
    return s[..., -1] - s[..., -2] if prob.shape[-1] > 1 else np.full(prob.shape[:-1], np.inf)


def fissures_from_lobes(lobes_filled):
    """find_lobes.py:47-88 with conv3d: (D, H, W) integer labels -> uint8 fissure labels"""
    lf = torch.as_tensor(np.asarray(lobes_filled)).long()
    one_hot = torch.nn.functional.one_hot(lf).permute(3, 0, 1, 2).unsqueeze(0)
    n_lobes = one_hot.shape[1] - 1
    cross = torch.zeros(3, 3, 3)
    cross[1, 1, :] = 1
    cross[1, :, 1] = 1
    cross[:, 1, 1] = 1
    kernel = cross.view(1, 1, 3, 3, 3).repeat(n_lobes + 1, 1, 1, 1, 1)
    dil = torch.nn.functional.conv3d(torch.nn.functional.pad(one_hot.float(), (1, 1, 1, 1, 1, 1)), kernel, groups=n_lobes + 1)[0] > 0
    out = torch.zeros_like(lf)
    out[dil[3] & dil[4]] = 1
    rof = dil[1] & dil[2]
    if n_lobes == 5:
        rof = rof | (dil[1] & dil[5])
    out[rof] = 2
    if n_lobes == 5:
        out[dil[2] & dil[5]] = 3
    return out.numpy().astype(np.uint8)


def make_volume(shape, n_seeds, n_lobes=4, seed=0, radius=0.45, island=False):
    """an ellipsoid mask cut into 4 or 5 regions by planes, `n_seeds` labelled voxels drawn inside the mask, and a smooth
    intensity image with a step at the region borders -> dict(mask bool, region, labels int64, im fp32).  `island` adds a
    small block of mask in a corner that holds no seed (the corner lies outside the ellipsoid)."""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    c = (np.array(shape) - 1) / 2
    ext = [max(s * radius, 0.75) for s in shape]
    mask = ((zz - c[0]) / ext[0]) ** 2 + ((yy - c[1]) / ext[1]) ** 2 + ((xx - c[2]) / ext[2]) ** 2 < 1
    right = xx > W / 2
    upper = zz + 0.3 * yy > D * 0.6
    region = np.where(right, np.where(upper, 4, 3), np.where(upper, 2, 1))
    if n_lobes == 5:
        region = np.where((region == 2) & (yy > H * 0.55), 5, region)
    labels = np.zeros(shape, np.int64)
    inside = np.where(mask.ravel())[0]
    pick = rng.choice(inside, min(n_seeds, inside.size), replace=False)
    labels.ravel()[pick] = region.ravel()[pick]
    if island:
        mask = mask.copy()
        mask[:2, :2, :3] = True
        labels[:2, :2, :3] = 0
    im = (40.0 * region + 3.0 * np.sin(zz / 3.0) * np.cos(xx / 4.0) + rng.standard_normal(shape)).astype(np.float32)
    return dict(mask=mask, region=region, labels=labels, im=im)
