"""Coherent point drift restated in plain torch, written from Myronenko & Song (TPAMI 2010, figures 2 and 4) with pycpd's
defaults and stopping rules: the checker for shape_model/point_cloud_registration.py and fsg_cpd_estep_f32.

`dtype` is the precision of the E-step: float64 is the oracle, float32 the yardstick (what a straightforward fp32 composition
of the responsibilities achieves on the same inputs).  The M-step -- centring, the 3 x 3 SVD, the kernel matrix G and the
M x M solve -- is float64 in both, the precision split of the package.  (With the M-step in float32 as well, the runs are not a
yardstick: the solve's condition number reaches 1e5..1e6 at the end of a deformable run, and over seeds of the test data the
float32 run then ends 1e-4 to 1e-1 units from the float64 one after 100 iterations.)  The E-step is the textbook formula on the
dense (M, N) matrix -- no shifted exponent, no clamp of small denominators -- so in float32 it underflows once 2 sigma^2 is
small against the squared distances; callers check `column_sums_survive` before they use it as a reference there.  One item
at a time, on the CPU."""
import math

import torch


# ------------------------------------------------------------------ test data: two samplings of one curved sheet
def sheet(n, seed, dtype=torch.float64):
    """n points of z = 0.3 sin(2u) + 0.2 v^2 over [-1, 1]^2, scaled to about 120 x 90 x 30 units"""
    g = torch.Generator().manual_seed(seed)
    u, v = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1 for _ in range(2))
    z = 0.3 * torch.sin(2 * u) + 0.2 * v * v
    return torch.stack([60 * u, 45 * v, 40 * z], 1).to(dtype)


def rot_z(angle):
    c, s = math.cos(angle), math.sin(angle)
    return torch.tensor([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]], dtype=torch.float64)


def similarity(P, scale, R, t):
    """rows of P moved by p -> scale R p + t"""
    return scale * P @ R.T + t


def sheet_pair(N=193, M=161, seed=0, dtype=torch.float64):
    """-> fixed X (N,3), moving Y (M,3): another sampling of the sheet, scaled by 0.9, rotated 0.25 rad about z, shifted by
    (8, -5, 4) and bent by a smooth sinusoid of a few units"""
    X, Y = sheet(N, 1000 + seed), sheet(M, 2000 + seed)
    Y = similarity(Y, 0.9, rot_z(0.25), torch.tensor([8., -5., 4.], dtype=torch.float64))
    bend = torch.stack([2.0 * torch.sin(Y[:, 1] / 30), torch.zeros(M, dtype=torch.float64), 3.0 * torch.sin(Y[:, 0] / 40)], 1)
    return X.to(dtype), (Y + bend).to(dtype)


# ------------------------------------------------------------------ E-step
def sq_dist(X, TY):
    """(M, N): |x_n - ty_m|^2 as a sum of squared differences"""
    return (X[None, :, :] - TY[:, None, :]).square().sum(2)


def outlier_constant(sigma2, w, N, M):
    return (2 * math.pi * sigma2) ** 1.5 * w / (1 - w) * M / N


def responsibilities(X, TY, sigma2, w=0.):
    """P (M, N) in the dtype of X"""
    N, M = X.shape[0], TY.shape[0]
    sigma2 = torch.as_tensor(sigma2, dtype=X.dtype, device=X.device)
    K = torch.exp(-sq_dist(X, TY) / (2 * sigma2))
    return K / (K.sum(0, keepdim=True) + outlier_constant(sigma2, w, N, M))


def column_sums_survive(X, TY, sigma2):
    """True when no fixed point's sum of Gaussians underflows to 0 in the dtype of X (then 0 / 0 would follow for w = 0)"""
    sigma2 = torch.as_tensor(sigma2, dtype=X.dtype, device=X.device)
    return bool((torch.exp(-sq_dist(X, TY) / (2 * sigma2)).sum(0) > 0).all())


def estep(X, TY, sigma2, w=0., dtype=None):
    """-> P1 (M), Pt1 (N), PX (M,3), Np, evaluated in `dtype` (default: that of X) and returned in the dtype of X"""
    out = X.dtype
    if dtype is not None:
        X, TY, sigma2 = X.to(dtype), TY.to(dtype), torch.as_tensor(sigma2).to(dtype)
    P = responsibilities(X, TY, sigma2, w)
    P1 = P.sum(1)
    return P1.to(out), P.sum(0).to(out), (P @ X).to(out), P1.sum().to(out)


def initial_sigma2(X, Y):
    return sq_dist(X, Y).sum() / (3 * X.shape[0] * Y.shape[0])


# ------------------------------------------------------------------ registrations
def rigid(X, Y, max_iterations=100, tolerance=1e-3, w=0., sigma2=None, dtype=torch.float64):
    """-> dict: TY, scale, rotation (TY = scale * Y @ rotation + translation), translation, iterations, sigma2 and `diffs`,
    the stopping quantity |q - q_prev| after every iteration"""
    est, dtype = dtype, torch.float64
    X, Y = X.to(dtype), Y.to(dtype)
    s, R, t = torch.ones((), dtype=dtype), torch.eye(3, dtype=dtype), torch.zeros(3, dtype=dtype)
    sigma2 = initial_sigma2(X, Y) if sigma2 is None else torch.as_tensor(sigma2, dtype=dtype)
    q, diff, it, TY, diffs = math.inf, math.inf, 0, Y.clone(), []
    while it < max_iterations and diff > tolerance:
        P1, Pt1, PX, Np = estep(X, TY, sigma2, w, dtype=est)
        muX, muY = PX.sum(0) / Np, (P1[:, None] * Y).sum(0) / Np
        Xh, Yh = X - muX, Y - muY
        A = (PX - P1[:, None] * muX).T @ Yh                      # Xh^T P^T Yh
        U, _, Vh = torch.linalg.svd(A)
        C = torch.ones(3, dtype=dtype)
        C[2] = torch.linalg.det(U @ Vh)
        R = U @ torch.diag(C) @ Vh
        trAR = torch.trace(A.T @ R)
        yPy = (P1 * Yh.square().sum(1)).sum()
        xPx = (Pt1 * Xh.square().sum(1)).sum()
        s = trAR / yPy
        t = muX - s * (R @ muY)
        TY = s * Y @ R.T + t
        q_new = float((xPx - 2 * s * trAR + s * s * yPy) / (2 * sigma2) + 1.5 * Np * torch.log(sigma2))
        diff, q = abs(q_new - q), q_new
        diffs.append(diff)
        sigma2 = (xPx - s * trAR) / (3 * Np)
        if sigma2 <= 0:
            sigma2 = torch.as_tensor(tolerance / 10, dtype=dtype)
        it += 1
    return dict(TY=TY, scale=s, rotation=R.T.contiguous(), translation=t, iterations=it, sigma2=sigma2, diffs=diffs)


def gaussian_kernel(Y, beta):
    return torch.exp(-sq_dist(Y, Y) / (2 * beta ** 2))


def deformable(X, Y, alpha, beta, max_iterations=100, tolerance=1e-3, w=0., sigma2=None, dtype=torch.float64):
    """-> dict: TY = Y + G @ W, G, W, iterations, sigma2 and `diffs`, the stopping quantity |sigma2 - sigma2_prev|"""
    est, dtype = dtype, torch.float64
    X, Y = X.to(dtype), Y.to(dtype)
    M = Y.shape[0]
    G, W = gaussian_kernel(Y, beta), torch.zeros(M, 3, dtype=dtype)
    sigma2 = initial_sigma2(X, Y) if sigma2 is None else torch.as_tensor(sigma2, dtype=dtype)
    diff, it, TY, diffs = math.inf, 0, Y.clone(), []
    eye = torch.eye(M, dtype=dtype)
    while it < max_iterations and diff > tolerance:
        P1, Pt1, PX, Np = estep(X, TY, sigma2, w, dtype=est)
        W = torch.linalg.solve(P1[:, None] * G + alpha * sigma2 * eye, PX - P1[:, None] * Y)
        TY = Y + G @ W
        prev = sigma2
        xPx = (Pt1 * X.square().sum(1)).sum()
        yPy = (P1 * TY.square().sum(1)).sum()
        sigma2 = (xPx - 2 * (TY * PX).sum() + yPy) / (3 * Np)
        if sigma2 <= 0:
            sigma2 = torch.as_tensor(tolerance / 10, dtype=dtype)
        diff = float((sigma2 - prev).abs())
        diffs.append(diff)
        it += 1
    return dict(TY=TY, G=G, W=W, iterations=it, sigma2=sigma2, diffs=diffs)


# ------------------------------------------------------------------ inverse-distance interpolation, dense
def interpolate_weighted_knn(existing, values, query, k=5):
    """the k nearest existing points of every query point by a dense sort, weights 1 / (distance + 1e-8)
    -> (values (Nq, C), indices (Nq, k), distances (Nq, k + 1): one more, so that callers can look at the gap)"""
    dist = sq_dist(existing, query).sqrt()                        # (Nq, Ne)
    top, idx = dist.topk(k + 1, dim=1, largest=False)
    wgt = 1 / (top[:, :k] + 1e-8)
    return (wgt[:, :, None] * values[idx[:, :k]]).sum(1) / wgt.sum(1, keepdim=True), idx[:, :k], top
