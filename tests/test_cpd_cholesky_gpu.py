"""GPU tests of deformable CPD with solver='cholesky' (shape_model/point_cloud_registration.py on csrc/cholesky.hip).

The bar of the 30-iteration run is test_cpd_gpu.py's: at most twice the error of the fp64 oracle run with an fp32 E-step.  Between
the two solvers the bar is 1e-6 units: the routes differ by about 1e-10 in fp64 arithmetic (tests/test_chol_oracle_cpu.py), and
the fp32 E-step that follows every M-step may amplify a last-bit difference over 30 iterations.  Measured values are printed
and, when FSG_CHOL_PARITY names a file, appended to it."""
import os

import numpy as np
import pytest
import torch

import chol_oracle as co
import cpd_oracle as oracle
import poisson_disk_oracle as po

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.01, 10.
BETWEEN_SOLVERS = 1e-6


def record(line):
    print(line)
    path = os.environ.get("FSG_CHOL_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def test_deformable_registration_30_iterations_cholesky(device):
    from fissure_segmentation_amd.shape_model.point_cloud_registration import DeformableRegistration
    X, Y = oracle.sheet_pair()
    Y = oracle.rigid(X, Y, 30, 0.)["TY"]
    ref = oracle.deformable(X, Y, ALPHA, BETA, 30, 0.)
    yard = oracle.deformable(X, Y, ALPHA, BETA, 30, 0., dtype=torch.float32)
    reg = DeformableRegistration(X.to(device), Y.to(device), alpha=ALPHA, beta=BETA, max_iterations=30, tolerance=0, solver='cholesky')
    TY, (G, W) = reg.register()
    assert reg.iteration == 30 and G.shape == (161, 161) and W.shape == (161, 3) and not reg._info.any()
    e_got, e_yard = float((TY.cpu() - ref["TY"]).abs().max()), float((yard["TY"] - ref["TY"]).abs().max())
    record(f"deformable 30 iterations TY, solver='cholesky': package {e_got:.3e} fp32-oracle {e_yard:.3e}")
    assert e_got <= 2 * e_yard, (e_got, e_yard)
    torch.testing.assert_close(G.cpu(), ref["G"], rtol=0, atol=1e-14)
    lu = DeformableRegistration(X.to(device), Y.to(device), alpha=ALPHA, beta=BETA, max_iterations=30, tolerance=0)
    TY_lu, (G_lu, _) = lu.register()
    between = float((TY - TY_lu).abs().max())
    record(f"deformable 30 iterations TY: |cholesky - lu| = {between:.3e}")
    assert torch.equal(G, G_lu) and lu.solver == 'lu' and between <= BETWEEN_SOLVERS, between


def test_default_stopping_batch_with_far_away_points(device):
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    pairs = [oracle.sheet_pair(seed=s) for s in range(3)]
    X = torch.stack([p[0] for p in pairs])
    Y = torch.stack([oracle.rigid(p[0], p[1], 30, 0.)["TY"] for p in pairs])
    Y[1] = co.push_far(Y[1])
    runs = {}
    for solver in pcr.SOLVERS:
        reg = pcr.DeformableRegistration(X.to(device), Y.to(device), alpha=ALPHA, beta=BETA, solver=solver)
        TY, (G, W) = reg.register()
        runs[solver] = (TY, reg.iteration.clone(), reg)
        assert TY.shape == (3, 161, 3) and torch.isfinite(TY).all()
        torch.testing.assert_close(reg.displacements(), TY - Y.to(device), rtol=0, atol=1e-9)
    chol = runs['cholesky'][2]
    assert chol._info.dtype == torch.int32 and chol._info.is_cuda and chol._info.tolist() == [0, 0, 0]
    its = [r[1].tolist() for r in runs.values()]
    between = float((runs['cholesky'][0] - runs['lu'][0]).abs().max())
    record(f"deformable default stopping B=3 (item 1 with two far-away points): iterations lu {its[0]} cholesky {its[1]}, "
           f"|cholesky - lu| = {between:.3e}")
    assert its[0] == its[1] and all(1 < i < 100 for i in its[0])
    assert between <= BETWEEN_SOLVERS
    # the reference's call: numpy in, numpy out
    with torch.cuda.device(device):
        deformed, disp = pcr.register_cpd_deformable(X.numpy(), Y.numpy(), solver='cholesky')
    assert isinstance(deformed, np.ndarray) and isinstance(disp, np.ndarray) and deformed.dtype == np.float64
    assert deformed.shape == disp.shape == (3, 161, 3)
    np.testing.assert_allclose(disp, deformed - Y.numpy(), rtol=0, atol=1e-9)
    assert np.array_equal(deformed, runs['cholesky'][0].cpu().numpy())
    assert np.abs(disp).max() > 1.


def test_a_rejected_system_is_reported_at_the_end(device):
    """the reporting path alone (a Gaussian kernel matrix and P1 >= 0 never give such a system; the kernels' own status is
    tested in test_cholesky_gpu.py): the status accumulated over the iterations is read once, and the items are named"""
    from fissure_segmentation_amd.shape_model.point_cloud_registration import DeformableRegistration
    pairs = [oracle.sheet_pair(N=70, M=40, seed=s) for s in range(2)]
    X, Y = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    reg = DeformableRegistration(X.to(device), Y.to(device), alpha=ALPHA, beta=BETA, max_iterations=3, tolerance=0, solver='cholesky')
    reg.register()
    assert reg._info.tolist() == [0, 0]
    reg._info = torch.maximum(reg._info, torch.tensor([0, 17], dtype=torch.int32, device=device))   # what an iteration does
    with pytest.raises(RuntimeError, match=r"item\(s\) \[1\].*\[17\]"):
        reg._check_run()
    reg.solver = 'lu'
    reg._check_run()


def test_register_all_with_the_cholesky_solver(device):
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    I, O, P = po.REG_INSTANCES, po.REG_OBJECTS, po.REG_POINTS
    fixed, meshes = po.fixed_clouds(), po.moving_surfaces()
    outs = {}
    for solver in pcr.SOLVERS:
        gen = torch.Generator(device=device).manual_seed(7)
        outs[solver] = pcr.register_all(list(fixed), meshes, generator=gen, pair_batch=4, solver=solver)
    lu, chol = outs['lu'], outs['cholesky']
    assert set(chol) == set(lu)
    for k in ("displacements", "moved_pcs", "moving_pcs"):
        assert isinstance(chol[k], np.ndarray) and chol[k].shape == lu[k].shape == (I, O, P, 3) and chol[k].dtype == np.float64
    assert np.array_equal(chol["moving_pcs"], lu["moving_pcs"])
    assert chol["n_correspondences"].shape == (I, O) and np.array_equal(chol["n_correspondences"], lu["n_correspondences"])
    assert chol["correspondences"] == lu["correspondences"]
    between = float(np.abs(chol["moved_pcs"] - lu["moved_pcs"]).max())
    record(f"register_all {I} x {O} x {P}: |cholesky - lu| of the deformed clouds = {between:.3e}")
    assert between <= BETWEEN_SOLVERS
    np.testing.assert_allclose(chol["displacements"], lu["displacements"], rtol=0, atol=BETWEEN_SOLVERS)
