"""The null-space Cholesky route of the thin-plate-spline fit restated in numpy: the checker for csrc/tps_nullspace.hip and
functional.tps_nullspace_system / tps_nullspace_fit / tps_fit(solver='nullspace').

The saddle system [[K, P], [P^T, 0]] [w; a] = [f; 0] with K = u(|c_i - c_j|) + lambda I and P = [1 | c] (n x 4) is solved by
eliminating P: with P = Q [R; 0] (Householder, LAPACK dgeqr2's convention: v_k[k] = 1, beta = -sign(alpha) |x|,
tau = (beta - alpha) / beta, tau = 0 where nothing lies below alpha), P^T w = 0 means w = Q [0; y], and the rows 4.. of
Q^T K Q [0; y] + [R a; 0] = Q^T f are S y = g with S = (Q^T K Q)[4:, 4:] symmetric positive definite (u is conditionally positive
definite of order 2).  The rows 0..3 give R a = (Q^T (f - K w))[:4].  `stages` follows the kernels' launch sequence step by step:
QR of P, X = K V, the dlatrd recurrence for W with Q^T K Q = K - V W^T - W V^T, S, Cholesky, the two sweeps, the affine rows.

Every sum over the points goes through `_sum`, so that the same restatement runs in another summation order (`order='reversed'`)
and in longdouble: `own_error(case)` is what the reversed-order fp64 run is off by against the longdouble run, relative to the
largest entry, per output.  A kernel, whose order is a third one, may be off by `bar(own)` = max(8.9e-16, 4 own)."""
import functools

import numpy as np

import tps_oracle as to

FLOOR = 8.9e-16           # 4 fp64 ulps of the largest entry
RESIDUAL_FLOOR = 8.9e-16  # the Cholesky tests' own bar: max(floor, 4 x LU's residual on the same system)
SOLVE_NS = [4, 5, 6, 67, 68, 69, 132, 133, 261, 1028]
SOLVE_LAMBDAS = [0.1, 0.0]
SYSTEM_NS = [4, 5, 67, 68, 69, 133, 261]
FIT_CASES = [(4, 0.1), (5, 0.1), (68, 0.1), (69, 0.0), (261, 0.1), (1028, 0.1)]
FIT_CHANNELS = [1, 3, 4]


def bar(own, floor=FLOOR):
    return max(floor, 4 * own)


# ------------------------------------------------------------------ inputs
def sheet(n, seed):
    """(n,3) fp32 on a curved sheet z = 0.3 sin(2x) cos(y): far from a plane, close to a surface"""
    xy = np.random.default_rng(seed).uniform(-0.9, 0.9, (n, 2))
    return np.concatenate([xy, 0.3 * np.sin(2 * xy[:, :1]) * np.cos(xy[:, 1:])], 1).astype(np.float32)


def small_cloud(n, seed):
    """the uniform cube scaled by 1e-2"""
    return (to.control_points(n, seed).astype(np.float64) * 1e-2).astype(np.float32)


def coplanar(n, seed):
    """(n,3) fp32 in the plane z = 0.25: P has rank 3, and its fourth column the third's exact multiple of the first"""
    c = to.control_points(n, seed)
    c[:, 2] = 0.25
    return c


def solve_cases():
    """(name, control (n,3) fp32, lambda) of the CPU residual test"""
    cases = [(f"cube-n{n}-l{lam}", to.control_points(n, 500 + n), lam) for n in SOLVE_NS for lam in SOLVE_LAMBDAS]
    cases += [(f"sheet-n64-l{lam}", sheet(64, 601), lam) for lam in SOLVE_LAMBDAS]
    cases += [(f"small-n64-l{lam}", small_cloud(64, 602), lam) for lam in SOLVE_LAMBDAS]
    return cases


# ------------------------------------------------------------------ the restatement
def _sum(x, order):
    """sum over axis 0 in one of two orders (numpy's pairwise sum, of the rows as they are or reversed)"""
    return np.sum(x[::-1] if order == "reversed" else x, axis=0)


def k_lambda(c, lambd, dtype=np.float64):
    """K + lambda I as fsg_tps_system_f64 writes it: u of the fp64 distances, the diagonal exactly lambda"""
    c = np.asarray(c, np.float64).astype(dtype)
    d = c[:, None, :] - c[None, :, :]
    r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    K = r * r * np.log(r + dtype(1e-6))
    K[np.arange(len(c)), np.arange(len(c))] = dtype(lambd)
    return K


def householder_qr(c, dtype=np.float64, order="forward"):
    """P = [1 | c] -> V (n,4) unit lower trapezoidal, tau (4), R (4,4) upper, info (0 or -k, 1-based, for the first
    |R_kk| <= n eps max_j |R_jj|; a NaN counts)"""
    c = np.asarray(c, np.float64).astype(dtype)
    n = len(c)
    A = np.concatenate([np.ones((n, 1), dtype), c], 1)
    V, tau, R = np.zeros((n, 4), dtype), np.zeros(4, dtype), np.zeros((4, 4), dtype)
    for k in range(4):
        if k >= n:
            continue                                        # no row left: R_kk = 0, H_k = I
        alpha = A[k, k]
        x2 = _sum(A[k + 1:, k] ** 2, order) if k + 1 < n else dtype(0)
        V[k, k] = 1
        if x2 == 0:
            beta = alpha                                    # tau = 0
        else:
            beta = -np.copysign(np.sqrt(alpha * alpha + x2), alpha)
            tau[k] = (beta - alpha) / beta
            V[k + 1:, k] = A[k + 1:, k] / (alpha - beta)
        R[k, k] = beta
        for j in range(k + 1, 4):
            s = _sum(V[k:, k] * A[k:, j], order)
            A[k:, j] = A[k:, j] - (tau[k] * s) * V[k:, k]
            R[k, j] = A[k, j]
    diag = np.abs(np.diag(R)).astype(np.float64)
    thr = n * 2.0 ** -52 * np.nanmax(diag) if np.isfinite(diag).any() else np.nan
    info = 0
    for k in range(4):
        if not diag[k] > thr:
            info = -(k + 1)
            break
    return V, tau, R, info


def w_recurrence(X, V, tau, order="forward"):
    """the dlatrd recurrence: X = K V -> W with Q^T K Q = K - V W^T - W V^T"""
    W = np.zeros_like(X)
    for k in range(4):
        p = X[:, k].copy()
        if k:
            p = p - V[:, :k] @ _sum(W[:, :k] * V[:, k:k + 1], order) - W[:, :k] @ _sum(V[:, :k] * V[:, k:k + 1], order)
        p = tau[k] * p
        W[:, k] = p - (tau[k] / 2 * _sum(p * V[:, k], order)) * V[:, k]
    return W


def apply_qt(x, V, tau, order="forward"):
    """Q^T x = H_3 H_2 H_1 H_0 x"""
    x = x.copy()
    for k in range(4):
        x = x - V[:, k:k + 1] * (tau[k] * _sum(V[:, k:k + 1] * x, order))[None]
    return x


def apply_q(x, V, tau, order="forward"):
    """Q x = H_0 H_1 H_2 H_3 x"""
    x = x.copy()
    for k in range(3, -1, -1):
        x = x - V[:, k:k + 1] * (tau[k] * _sum(V[:, k:k + 1] * x, order))[None]
    return x


def cholesky_lower(S):
    """-> (L, info): unblocked, reading the lower triangle only; info = j (1-based) at the first pivot that is not positive (the
    factor is then unspecified from column j on, as fsg_cholesky_f64 has it)"""
    L = np.tril(S).copy()
    m = len(L)
    for j in range(m):
        p = L[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0:
            return L, j + 1
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, 0


def system_stages(c, lambd, dtype=np.float64, order="forward"):
    """steps 1-4 -> dict(V, tau, R, X, W, S, info); S holds its LOWER triangle, zeros above"""
    V, tau, R, info = householder_qr(c, dtype, order)
    K = k_lambda(c, lambd, dtype)
    X = np.stack([_sum(K.T * V[:, k:k + 1], order) for k in range(4)], 1) if order == "reversed" else K @ V
    W = w_recurrence(X, V, tau, order)
    S = np.tril((K - V @ W.T - W @ V.T)[4:, 4:])
    return dict(V=V, tau=tau, R=R, X=X, W=W, S=S, K=K, info=info)


def fit(c, f, lambd, dtype=np.float64, order="forward"):
    """the whole route -> (theta (n+4, C), info): 0, -k (rank) or j (the reduced system's leading minor of order j)"""
    st = system_stages(c, lambd, dtype, order)
    V, tau, R, K = st["V"], st["tau"], st["R"], st["K"]
    f = np.asarray(f, np.float64).astype(dtype)
    n = len(f)
    info = st["info"]
    w = np.zeros_like(f)
    if n > 4:
        L, cinfo = cholesky_lower(st["S"])
        info = info or cinfo
        g = apply_qt(f, V, tau, order)[4:]
        with np.errstate(all="ignore"):
            y = np.linalg.solve(L.T, np.linalg.solve(L, g)) if dtype == np.float64 else _tri_solve(L, g)
        w = apply_q(np.concatenate([np.zeros_like(f[:4]), y]), V, tau, order)
    t = apply_qt(f - K @ w, V, tau, order)[:4]
    a = np.zeros_like(t)
    with np.errstate(all="ignore"):
        for k in range(3, -1, -1):
            a[k] = (t[k] - R[k, k + 1:] @ a[k + 1:]) / R[k, k]
    return np.concatenate([w, a]), info


def _tri_solve(L, g):
    """L L^T y = g by substitution (numpy.linalg does not take longdouble)"""
    m = len(L)
    y = g.copy()
    for i in range(m):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(m - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def residual(A, theta, b):
    """max|A theta - b| / (max|A| max|theta|) of the full saddle system"""
    return float(np.abs(A @ theta - b).max() / (np.abs(A).max() * np.abs(theta).max()))


def saddle(c, f, lambd):
    A = to.system64(c, lambd)
    b = np.zeros((len(c) + 4, np.shape(f)[1]))
    b[:len(c)] = f
    return A, b


# ------------------------------------------------------------------ the restatement's own error (what another order is off by)
def _rel(got, want):
    want = np.asarray(want, np.longdouble)
    if want.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, np.longdouble) - want).max() / max(np.abs(want).max(), np.finfo(np.float64).tiny))


@functools.lru_cache(maxsize=None)
def system_inputs(n):
    """the two clouds (B = 2) of the stage test at n points, and its lambda"""
    return np.stack([to.control_points(n, 700 + n), sheet(n, 800 + n) if n > 4 else to.control_points(n, 900 + n)]), 0.1


@functools.lru_cache(maxsize=None)
def own_error(n):
    """per item of `system_inputs(n)`: {output: error of the reversed-order fp64 run against the longdouble run}.  Recorded by
    tests/test_tps_ns_cpu.py (which prints them); the GPU test holds the kernels to `bar` of these."""
    cs, lambd = system_inputs(n)
    out = []
    for c in cs:
        a = system_stages(c, lambd, np.float64, "reversed")
        b = system_stages(c, lambd, np.longdouble, "forward")
        out.append({k: _rel(a[k], b[k]) for k in ("V", "tau", "R", "S")})
    return out
