"""The symmetric positive definite route through deformable CPD's M-step, restated in plain torch fp64 on the CPU, and the residual
helpers of the Cholesky tests: the checker for csrc/cholesky.hip and `DeformableRegistration(solver='cholesky')`.

The M-step matrix A = diag(P1) G + alpha sigma2 I is similar to S = D G D + alpha sigma2 I with D = diag(sqrt(P1)):
A = D (S) D^-1 where P1 > 0, and a row with P1 = 0 decouples in both (its W is 0).  With S V = rhs and
rhs = (PX - P1 Y) / d (0 where d = 0), W = d V.  Everything else -- E-step, sigma2, stopping rule -- is cpd_oracle's."""
import math

import numpy as np
import torch

import cpd_oracle

ALPHA, BETA = 0.01, 10.

# (N, M, w, far): sheet pairs of cpd_oracle; `far` pushes two moving points 900 and 1500 units away, which takes their P1 to
# exactly 0 once sigma2 has shrunk
CASES = [(193, 161, 0., False), (193, 161, 0.1, False), (1025, 1023, 0., False), (70, 300, 0.1, True), (193, 161, 0., True)]


def case_pair(N, M, far, seed=0):
    X, Y = cpd_oracle.sheet_pair(N=N, M=M, seed=seed)
    if far:
        Y = push_far(Y)
    return X, Y


def push_far(Y):
    Y = Y.clone()
    Y[0, 0] += 900.
    Y[1, 1] -= 1500.
    return Y


def spd_system(G, P1, PX, Y, sigma2, alpha):
    """-> S (M,M) full and symmetric, rhs (M,3), d (M); fp64"""
    d = P1.sqrt()
    S = (d[:, None] * G) * d[None, :]
    S = S + alpha * sigma2 * torch.eye(G.shape[0], dtype=G.dtype)
    num = PX - P1[:, None] * Y
    rhs = torch.where(d[:, None] > 0, num / d[:, None], torch.zeros_like(num))
    return S, rhs, d


def lu_system(G, P1, PX, Y, sigma2, alpha):
    return P1[:, None] * G + alpha * sigma2 * torch.eye(G.shape[0], dtype=G.dtype), PX - P1[:, None] * Y


def spd_mstep(G, P1, PX, Y, sigma2, alpha):
    """-> W (M,3) and LAPACK's status of the factorisation"""
    S, rhs, d = spd_system(G, P1, PX, Y, sigma2, alpha)
    L, info = torch.linalg.cholesky_ex(S)
    return d[:, None] * torch.cholesky_solve(rhs, L), int(info)


def deformable_spd(X, Y, alpha=ALPHA, beta=BETA, max_iterations=100, tolerance=1e-3, w=0., sigma2=None, dtype=torch.float64,
                   keep_systems=False):
    """cpd_oracle.deformable with the M-step solved through S.  -> its dict, plus `info` (the largest LAPACK status),
    `zero_rows` (the number of exactly-zero entries of P1 per iteration) and, with keep_systems, `systems`: the
    (G, P1, PX, Y, sigma2) of the first and the last iteration"""
    est, dtype = dtype, torch.float64
    X, Y = X.to(dtype), Y.to(dtype)
    M = Y.shape[0]
    G, W = cpd_oracle.gaussian_kernel(Y, beta), torch.zeros(M, 3, dtype=dtype)
    sigma2 = cpd_oracle.initial_sigma2(X, Y) if sigma2 is None else torch.as_tensor(sigma2, dtype=dtype)
    diff, it, TY, diffs, worst, zero_rows, systems = math.inf, 0, Y.clone(), [], 0, [], []
    while it < max_iterations and diff > tolerance:
        P1, Pt1, PX, Np = cpd_oracle.estep(X, TY, sigma2, w, dtype=est)
        zero_rows.append(int((P1 == 0).sum()))
        if keep_systems:
            systems = systems[:1] + [(G, P1, PX, Y, sigma2.clone())]
        W, info = spd_mstep(G, P1, PX, Y, sigma2, alpha)
        worst = max(worst, info)
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
    return dict(TY=TY, G=G, W=W, iterations=it, sigma2=sigma2, diffs=diffs, info=worst, zero_rows=zero_rows, systems=systems)


def condition_pair(G, P1, PX, Y, sigma2, alpha=ALPHA):
    """(cond_2 of A, cond_2 of S) of one M-step system; rows with P1 = 0 decouple in both and are left out"""
    keep = P1 > 0
    A = lu_system(G, P1, PX, Y, sigma2, alpha)[0][keep][:, keep]
    S = spd_system(G, P1, PX, Y, sigma2, alpha)[0][keep][:, keep]
    return float(torch.linalg.cond(A)), float(torch.linalg.cond(S))


# ------------------------------------------------------------------ test matrices and residuals
def random_spd(n, cond, seed, B=1):
    """(B,n,n) fp64: orthogonal x log-spaced spectrum in [1 / cond, 1], symmetrised bit for bit"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        Q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
        ev = torch.logspace(0, -math.log10(cond), n, dtype=torch.float64) if n > 1 else torch.ones(1, dtype=torch.float64)
        A = (Q * ev) @ Q.T
        out.append(torch.tril(A) + torch.tril(A, -1).T)
    return torch.stack(out)


def lower_symmetric(A):
    """the symmetric matrix whose lower triangle is that of A (whatever the strict upper triangle holds)"""
    low = torch.tril(A)
    return low + torch.tril(A, -1).transpose(-1, -2)


def _wide(t):
    """np.longdouble for n <= 257, fp64 above"""
    a = t.detach().cpu().numpy()
    return a.astype(np.longdouble) if a.shape[-2] <= 257 else a


def factor_residual(A, L):
    """max |A - L L^T| / max |A| for one (n,n) matrix, both taken from their lower triangles"""
    a, low = _wide(lower_symmetric(A)), _wide(torch.tril(L))
    return float(np.abs(a - low @ low.T).max() / np.abs(a).max())


def solve_residual(A, X, b):
    """max |A X - b| / (max |A| max |X| + max |b|) for one system; A from its lower triangle"""
    a = _wide(lower_symmetric(A))
    x, rhs = X.detach().cpu().numpy().astype(a.dtype), b.detach().cpu().numpy().astype(a.dtype)
    return float(np.abs(a @ x - rhs).max() / (np.abs(a).max() * np.abs(x).max() + np.abs(rhs).max()))
