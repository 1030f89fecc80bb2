"""The null-space Cholesky route of the thin-plate-spline fit, without a GPU: tests/tps_ns_oracle.py (the numpy restatement of the
launch sequence of csrc/tps_nullspace.hip) is pinned against LAPACK's LU on tps_oracle.system64, its reduced matrix against
numpy.linalg.qr, its status codes on the degenerate inputs; and the C ABI carries the two entries.

Bars.  Residual max|A theta - b| / (max|A| max|theta|) of the full saddle system: max(8.9e-16, 4 x LU's residual on the same
system), the Cholesky tests' own.  The two solutions: 1e-9 of the largest entry.  S against numpy's Q^T K Q: both are fp64
computations of a congruence with entries of the size of max|K| n; 64 n ulps of the largest entry of Q^T K Q (an elementwise
bound on the rounding of two n-term products)."""
import ctypes
import os

import numpy as np
import pytest

import tps_ns_oracle as ns
import tps_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ns.solve_cases()
ULP64 = np.finfo(np.float64).eps


@pytest.mark.parametrize("name,c,lambd", CASES, ids=[k[0] for k in CASES])
def test_solve_against_lapack_lu(name, c, lambd):
    n = len(c)
    f = to.rough_values(n, 3, 40 + n)
    A, b = ns.saddle(c, f, lambd)
    lu = np.linalg.solve(A, b)
    theta, info = ns.fit(c, f, lambd)
    r_ns, r_lu = ns.residual(A, theta, b), ns.residual(A, lu, b)
    apart = to.rel_err(theta, lu)
    print(f"{name}: residual {r_ns:.3e}, LU's {r_lu:.3e} (bar {max(ns.RESIDUAL_FLOOR, 4 * r_lu):.3e}); solutions {apart:.3e} apart")
    assert info == 0
    assert r_ns <= max(ns.RESIDUAL_FLOOR, 4 * r_lu)
    assert apart <= 1e-9
    assert n > 4 or not theta[:n].any()   # n = 4: the reduced system is empty and w = 0 exactly


@pytest.mark.parametrize("name,c,lambd", CASES, ids=[k[0] for k in CASES])
def test_reduced_matrix(name, c, lambd):
    n = len(c)
    st = ns.system_stages(c, lambd)
    V, tau, R, S = st["V"], st["tau"], st["R"], st["S"]
    P = np.concatenate([np.ones((n, 1)), np.asarray(c, np.float64)], 1)
    # the reflectors reproduce P, and V has the stated form
    QR = ns.apply_q(np.concatenate([R, np.zeros((n - 4, 4))]), V, tau)
    assert np.abs(QR - P).max() <= 64 * ULP64 * np.abs(P).max() * np.sqrt(n)
    assert np.array_equal(np.triu(V[:4], 1), np.zeros((4, 4))) and np.array_equal(np.diag(V[:4]), np.ones(4))
    assert np.array_equal(np.tril(R, -1), np.zeros((4, 4)))
    if n == 4:
        assert S.shape == (0, 0)
        return
    Q2, R2 = np.linalg.qr(P, mode="complete")
    full = Q2.T @ st["K"] @ Q2
    want = full[4:, 4:]
    sym = S + np.tril(S, -1).T
    allowed = 64 * n * ULP64 * np.abs(full).max()
    ev, ev_want = np.linalg.eigvalsh(sym), np.linalg.eigvalsh((want + want.T) / 2)
    print(f"{name}: smallest eigenvalue {ev[0]:.3e}; eigenvalues off by {np.abs(ev - ev_want).max():.3e} (bar {allowed:.3e})")
    assert ev[0] > 0
    assert np.abs(ev - ev_want).max() <= allowed
    # S itself: the last n - 4 columns of the two Q span the same space, related by an orthogonal m x m matrix
    Qn = ns.apply_q(np.eye(n), V, tau)
    T = Q2[:, 4:].T @ Qn[:, 4:]
    assert np.abs(np.tril(T.T @ want @ T - sym)).max() <= allowed
    # and the signs of R: |R_kk| agree, R = D R2 with D = diag(+-1)
    D = np.sign(np.diag(R)) * np.sign(np.diag(R2))
    assert np.abs(R - D[:, None] * R2[:4]).max() <= 64 * ULP64 * np.abs(R2).max() * np.sqrt(n)


def test_status_codes():
    assert ns.householder_qr(ns.coplanar(20, 1))[3] == -4
    assert ns.householder_qr(to.control_points(3, 1))[3] < 0
    bad = to.control_points(20, 2)
    bad[7, 1] = np.nan
    assert ns.householder_qr(bad)[3] != 0
    f = to.rough_values(40, 3, 1)
    assert ns.fit(to.control_points(40, 3, duplicates=2), f, 0.0)[1] > 0      # a singular reduced system
    assert ns.fit(to.control_points(40, 3), f, -1.0)[1] > 0                   # an indefinite one
    assert ns.fit(to.control_points(40, 3, duplicates=2), f, 0.1)[1] == 0     # the ridge makes duplicates regular
    assert ns.fit(ns.coplanar(20, 1), f[:20], 0.1)[1] == -4


@pytest.mark.parametrize("n", ns.SYSTEM_NS)
def test_own_error_of_the_restatement(n):
    """the figures the GPU test's bars are built on: another summation order against longdouble"""
    for b, own in enumerate(ns.own_error(n)):
        print(f"n={n} item {b}: " + ", ".join(f"{k} {v:.3e}" for k, v in own.items()))
        for k, v in own.items():
            assert np.isfinite(v) and v < 1e-12, (k, v)


def test_abi_carries_the_entries():
    from fissure_segmentation_amd import _abi
    defines, _, signatures = _abi.load(os.path.join(ROOT, "include", "fsg_hip.h"))
    lib = ctypes.CDLL(os.path.join(ROOT, "fissure-segmentation_amd", "libfsg_hip.so"))
    for name, nargs in (("fsg_tps_ns_system_f64", 11), ("fsg_tps_ns_solve_f64", 13)):
        assert hasattr(lib, name), f"{name} is not exported"
        args, res = signatures[name]
        assert len(args) == nargs and res is ctypes.c_int
    assert defines["FSG_TPS_NS_SYSTEM_WORK_PER_POINT"] == 4 and defines["FSG_TPS_NS_SOLVE_WORK_PER_VALUE"] == 2


def test_unknown_solver_is_a_value_error_without_a_gpu():
    import torch
    from fissure_segmentation_amd import functional as F
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    assert pcr.TPS_SOLVERS == ['lu', 'nullspace']
    c, f = torch.zeros(5, 3), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="solver"):
        F.tps_fit(c, f, solver='qr')
    with pytest.raises(ValueError, match="solver"):
        pcr.TPS.fit(c, f, solver='qr')
