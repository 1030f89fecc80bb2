"""CPU pins of the symmetric positive definite route through deformable CPD (tests/chol_oracle.py) and of the Cholesky entries'
declarations.  The bar of the run-level comparison: cond(S) <= 1.7e6 at the end of a run, times the fp64 unit roundoff 1.1e-16,
times coordinates of magnitude 60, is 1e-8 units; the two routes solve the same systems and differ by rounding alone."""
import os
import re

import numpy as np
import pytest
import torch

import chol_oracle as co
import cpd_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs():
    out = {}
    for N, M, w, far in co.CASES:
        X, Y = co.case_pair(N, M, far)
        out[(N, M, w, far)] = (cpd_oracle.deformable(X, Y, co.ALPHA, co.BETA, w=w), co.deformable_spd(X, Y, w=w, keep_systems=True))
    return out


def test_the_cases_are_the_five_of_the_design_check():
    assert len(co.CASES) == 5 and {c[:2] for c in co.CASES} == {(193, 161), (1025, 1023), (70, 300)}
    assert {c[2] for c in co.CASES} == {0., 0.1} and sum(c[3] for c in co.CASES) == 2


@pytest.mark.parametrize("case", co.CASES, ids=lambda c: "%dx%d_w%g_%s" % (c[0], c[1], c[2], "far" if c[3] else "near"))
def test_symmetrised_run_ends_where_the_lu_run_ends(runs, case):
    lu, spd = runs[case]
    diff = float((lu["TY"] - spd["TY"]).abs().max())
    print(f"{case}: |TY_spd - TY_lu| = {diff:.3e} after {spd['iterations']} iterations, {sum(spd['zero_rows'])} zero rows of P1")
    assert spd["info"] == 0
    assert spd["iterations"] == lu["iterations"] and 1 < lu["iterations"] < 100
    assert diff <= 1e-8, diff
    assert float(lu["TY"].abs().max()) > 30   # the scale the bar was worked out for


def test_far_away_points_give_exact_zero_rows(runs):
    far = [runs[c][1]["zero_rows"] for c in co.CASES if c[3]]
    assert all(sum(z) > 0 for z in far) and sum(sum(z) for z in far) > 100, far
    # such a row decouples: W is 0 there -- exactly in the symmetric route, to the rounding of a pivoted elimination in the other
    for c in co.CASES:
        if c[3]:
            G, P1, PX, Y, sigma2 = runs[c][1]["systems"][-1]
            zero = P1 == 0
            assert zero.any()
            W, info = co.spd_mstep(G, P1, PX, Y, sigma2, co.ALPHA)
            A, b = co.lu_system(G, P1, PX, Y, sigma2, co.ALPHA)
            assert info == 0 and not W[zero].any() and float(torch.linalg.solve(A, b)[zero].abs().max()) < 1e-10


@pytest.mark.parametrize("case", co.CASES, ids=lambda c: "%dx%d_w%g_%s" % (c[0], c[1], c[2], "far" if c[3] else "near"))
def test_s_is_no_worse_conditioned_than_a(runs, case):
    for which, system in zip(("first", "last"), runs[case][1]["systems"]):
        cond_a, cond_s = co.condition_pair(*system)
        print(f"{case} {which} iteration: cond(A) = {cond_a:.4e}, cond(S) = {cond_s:.4e}")
        assert cond_s <= cond_a * (1 + 1e-12), (which, cond_s, cond_a)


def test_restatement_is_the_similarity_transform():
    X, Y = co.case_pair(193, 161, False)
    G = cpd_oracle.gaussian_kernel(Y, co.BETA)
    P1, _, PX, _ = cpd_oracle.estep(X, Y, torch.tensor(50., dtype=torch.float64), 0.)
    S, rhs, d = co.spd_system(G, P1, PX, Y, torch.tensor(50., dtype=torch.float64), co.ALPHA)
    A, b = co.lu_system(G, P1, PX, Y, torch.tensor(50., dtype=torch.float64), co.ALPHA)
    torch.testing.assert_close(S, S.T, rtol=2.0 ** -51, atol=0)   # (d_i G_ij) d_j and (d_j G_ji) d_i: two roundings each
    torch.testing.assert_close(d[:, None] * S / d[None, :], A, rtol=1e-13, atol=0)
    torch.testing.assert_close(d[:, None] * rhs, b, rtol=1e-13, atol=1e-13)


def test_residual_helpers_on_lapack():
    A = co.random_spd(40, 1e6, 3)[0]
    L = torch.linalg.cholesky(A)
    b = torch.randn(40, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert co.factor_residual(A, L) < 1e-15 and co.solve_residual(A, torch.cholesky_solve(b, L), b) < 1e-15
    assert co.factor_residual(A, 1.001 * L) > 1e-4 and co.solve_residual(A, b, b) > 1e-3
    junk = A + torch.triu(torch.full_like(A, float("nan")), 1)     # the strict upper triangle is not looked at
    assert co.factor_residual(junk, L) == co.factor_residual(A, L)
    assert float(torch.linalg.cond(A)) == pytest.approx(1e6, rel=1e-6)


def test_header_declares_the_entries_and_the_limits():
    text = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    for entry in ("fsg_cholesky_f64", "fsg_cholesky_solve_f64", "fsg_cpd_spd_system_f64"):
        assert re.search(r"^int %s\(" % entry, text, re.M), entry
    defines = dict(re.findall(r"^#define (FSG_CHOL_\w+) (\d+)", text, re.M))
    assert defines == {"FSG_CHOL_BLOCK": "64", "FSG_CHOL_MAX_N": "8192", "FSG_CHOL_MAX_BATCH": "65535", "FSG_CHOL_MAX_RHS": "8"}
    assert int(defines["FSG_CHOL_BLOCK"]) % 16 == 0
    from fissure_segmentation_amd import _lib, functional
    assert functional.CHOL_BLOCK == _lib.CHOL_BLOCK == 64 and functional.CHOL_MAX_RHS == 8
    for entry in ("fsg_cholesky_f64", "fsg_cholesky_solve_f64", "fsg_cpd_spd_system_f64"):
        assert entry in _lib.SIGNATURES and hasattr(_lib.lib, entry)
    for name in ("cholesky_factor", "cholesky_solve", "spd_solve", "cpd_spd_system"):
        assert callable(getattr(functional, name))


def test_unknown_solver_is_refused_before_any_gpu_use():
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    X, Y = (t.numpy() for t in co.case_pair(70, 30, False))
    with pytest.raises(ValueError, match="solver"):
        pcr.DeformableRegistration(X, Y, alpha=co.ALPHA, beta=co.BETA, solver="qr")
    with pytest.raises(ValueError, match="solver"):
        pcr.register_cpd_deformable(X, Y, solver="qr")
    with pytest.raises(ValueError, match="solver"):
        pcr.register_all([X], [[(np.zeros((3, 3)), np.zeros((1, 3), dtype=np.int64))]], solver="qr")
    assert pcr.SOLVERS == ["lu", "cholesky"]
    assert pcr.DeformableRegistration(X, Y, alpha=co.ALPHA, beta=co.BETA).solver == "lu"


def test_wrappers_refuse_bad_arguments_before_any_gpu_use():
    from fissure_segmentation_amd import functional as F
    A, b = torch.eye(4, dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64)
    for bad in (A.float(), torch.ones(4, 5, dtype=torch.float64), torch.ones(4, dtype=torch.float64),
                torch.ones(2, 2, 4, 4, dtype=torch.float64), A.numpy()):
        with pytest.raises(ValueError):
            F.cholesky_factor(bad)
    with pytest.raises(ValueError):
        F.cholesky_solve(A, torch.ones(4, F.CHOL_MAX_RHS + 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        F.cholesky_solve(A, b.float())
    with pytest.raises(ValueError):
        F.cholesky_solve(A, torch.ones(5, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        F.cholesky_solve(A[None], b)                  # a batch of matrices, right-hand sides without the batch axis
    with pytest.raises(ValueError):
        F.cpd_spd_system(A[None], torch.ones(1, 4, dtype=torch.float64), b[None], b[None].float(), torch.ones(1, dtype=torch.float64), 0.01)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.cholesky_factor(A)
