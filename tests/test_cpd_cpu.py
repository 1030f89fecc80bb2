"""CPU tests of the coherent-point-drift port (shape_model/point_cloud_registration.py): the torch oracle (tests/cpd_oracle.py)
on a known transform, the stability of its fp32 yardstick, the numpy / torch helpers and the argument checks that run before
any launch."""
import numpy as np
import pytest
import torch

import cpd_oracle as oracle

ALPHA, BETA = 0.01, 10.


@pytest.fixture(scope="module")
def pair():
    return oracle.sheet_pair()


def test_oracle_recovers_a_known_similarity_transform():
    """X is a permuted exact copy of Y under scale 0.9, 0.25 rad about z and a shift.  The fp64 run (it ends through the
    sigma2 <= 0 -> tolerance / 10 branch after 16 iterations) recovers scale, rotation, translation and TY to 2.2e-16,
    3.3e-16, 1.8e-15 and 2.8e-14; asserted at 10 x those."""
    Y = oracle.sheet(161, 5)
    R, t = oracle.rot_z(0.25), torch.tensor([8., -5., 4.], dtype=torch.float64)
    perm = torch.randperm(161, generator=torch.Generator().manual_seed(3))
    X = oracle.similarity(Y, 0.9, R, t)[perm]
    r = oracle.rigid(X, Y)
    errs = (abs(float(r["scale"]) - 0.9), float((r["rotation"] - R.T).abs().max()), float((r["translation"] - t).abs().max()),
            float((r["TY"][perm] - X).abs().max()))
    print("known transform: iterations", r["iterations"], "errors (scale, rotation, translation, TY)", errs)
    assert r["iterations"] < 100
    for e, bound in zip(errs, (2.2e-15, 3.3e-15, 1.8e-14, 2.8e-13)):
        assert e <= bound, errs
    # the convention: TY = scale * Y @ rotation + translation
    torch.testing.assert_close(r["TY"], r["scale"] * Y @ r["rotation"] + r["translation"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind,bounds", [("rigid", (2.1e-6, 2.3e-6, 2.8e-6)), ("deformable", (2.5e-5, 5.2e-5, 2.7e-5))])
def test_yardstick_is_stable(pair, kind, bounds):
    """the oracle with an fp32 E-step against its fp64 run after 10, 30 and 100 iterations, max |TY32 - TY64|.  Measured with
    this oracle on this data: 2.1e-6, 2.3e-6, 2.8e-6 rigid and 2.5e-5, 5.2e-5, 2.7e-5 deformable -- no growth with the
    iteration count; asserted at 5 x those (fp32 library kernels differ between hosts in the last bits, and 100 EM
    iterations carry such a difference along).  That is inside the 5 x (1.0e-4, 1.1e-4, 1.0e-4) and 5 x (1.9e-5, 8.0e-5,
    6.8e-5) first set for an oracle whose M-step was fp32 as well."""
    X, Y = pair
    if kind == "deformable":
        Y = oracle.rigid(X, Y, 30, 0.)["TY"]
    run = (lambda it, dt: oracle.rigid(X, Y, it, 0., dtype=dt)) if kind == "rigid" else \
        (lambda it, dt: oracle.deformable(X, Y, ALPHA, BETA, it, 0., dtype=dt))
    for it, bound in zip((10, 30, 100), bounds):
        a, b = run(it, torch.float64), run(it, torch.float32)
        assert a["iterations"] == b["iterations"] == it
        err = float((a["TY"] - b["TY"]).abs().max())
        print(kind, it, "iterations: max |TY32 - TY64| =", err)
        assert err <= 5 * bound, (kind, it, err)


def test_test_data_keeps_every_column_sum_in_fp64(pair):
    X, Y = pair
    assert X.shape == (193, 3) and Y.shape == (161, 3)
    ext = X.max(0).values - X.min(0).values
    assert 110 < ext[0] < 125 and 80 < ext[1] < 95 and 25 < ext[2] < 35
    for s2 in (400., 25., 1.):
        assert oracle.column_sums_survive(X, Y, s2)
    assert not oracle.column_sums_survive(X.float(), Y.float(), 1.)   # why the fp32 composition is no yardstick at sigma2 = 1


def test_inverse_affine_transform_numpy_and_torch_round_trip():
    from fissure_segmentation_amd.utils.general_utils import inverse_affine_transform
    pts = oracle.sheet(50, 11)
    R, t = oracle.rot_z(0.4), torch.tensor([3., -2., 7.], dtype=torch.float64)
    moved = oracle.similarity(pts, 1.3, R, t)
    back = inverse_affine_transform(moved, 1.3, R, t)
    assert isinstance(back, torch.Tensor) and back.shape == (50, 3)
    torch.testing.assert_close(back, pts, rtol=0, atol=1e-12)
    back_np = inverse_affine_transform(moved.numpy(), 1.3, R.numpy(), t.numpy())
    assert isinstance(back_np, np.ndarray) and back_np.dtype == np.float64
    np.testing.assert_allclose(back_np, pts.numpy(), rtol=0, atol=1e-12)
    # with what the reference stores for a rigid pre-registration: scale, rotation.T, translation of TY = s Y @ rotation + t
    r = oracle.rigid(moved, pts, 40)
    undone = inverse_affine_transform(r["TY"], r["scale"], r["rotation"].T, r["translation"])
    torch.testing.assert_close(undone, pts, rtol=0, atol=1e-9)


def test_argument_checks_run_before_any_launch():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    X, Y = (a.numpy() for a in oracle.sheet_pair(N=12, M=9))
    reg = pcr.RigidRegistration(X, Y)                       # numpy goes in as the reference passes it; nothing runs yet
    assert (reg.max_iterations, reg.tolerance, reg.w) == (100, 1e-3, 0.) and reg.iteration == 0
    assert (reg.B, reg.N, reg.M) == (1, 12, 9)
    d = pcr.DeformableRegistration(X[None], Y[None], alpha=ALPHA, beta=BETA, max_iterations=7)
    assert (d.alpha, d.beta, d.max_iterations, d.B) == (ALPHA, BETA, 7, 1)
    with pytest.raises(RuntimeError, match="GPU only"):     # torch tensors must be on the device
        pcr.RigidRegistration(torch.from_numpy(X), torch.from_numpy(Y))
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.cpd_estep(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3), torch.ones(1))
    with pytest.raises(TypeError):
        pcr.RigidRegistration(X, torch.from_numpy(Y))
    with pytest.raises(TypeError):
        pcr.RigidRegistration(X.tolist(), Y)
    for bad in (dict(X=X[:, :2]), dict(Y=Y[None, None]), dict(X=np.stack([X, X])), dict(X=X.astype(np.int64)),
                dict(max_iterations=-1), dict(max_iterations=2.5), dict(tolerance=-1e-3), dict(w=1.), dict(w=-0.1),
                dict(sigma2=0.), dict(sigma2=[1., 2.])):
        with pytest.raises(ValueError):
            pcr.RigidRegistration(**{**dict(X=X, Y=Y), **bad})
    for bad in (dict(alpha=0.), dict(beta=-1.), dict(alpha="1")):
        with pytest.raises(ValueError):
            pcr.DeformableRegistration(**{**dict(X=X, Y=Y, alpha=ALPHA, beta=BETA), **bad})
    with pytest.raises(NotImplementedError, match="tps.*out of scope"):
        pcr.inverse_transformation_at_sampled_points(Y, Y, X, None, interpolation_mode='tps')
    with pytest.raises(ValueError, match="interpolation_mode must be one of"):
        pcr.inverse_transformation_at_sampled_points(Y, Y, X, None, interpolation_mode='linear')
    assert pcr.INTERPOLATION_MODES == ['knn', 'tps']


def test_host_side_checks_of_the_entry_point():
    from fissure_segmentation_amd import _lib
    assert _lib.lib.fsg_cpd_estep_workspace_bytes(3, 193, 161) == 3 * 193 * 16
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("fsg_cpd_estep_f32", 1, 0, 1, 1, 0., 1, 0, 5, 1, 1, 1, 1, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="outlier weight"):
        _lib.call("fsg_cpd_estep_f32", 1, 0, 1, 1, 1., 1, 4, 5, 1, 1, 1, 1, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="x_batch_stride"):
        _lib.call("fsg_cpd_estep_f32", 1, 6, 1, 1, 0., 2, 4, 5, 1, 1, 1, 1, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_cpd_estep_f32", None, 0, 1, 1, 0., 1, 4, 5, 1, 1, 1, 1, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("fsg_cpd_estep_f32", 1, 0, 1, 1, 0., 1, 4, 5, 1, 1, 1, 1, 8, 63, None)


def test_reference_import_name_resolves():
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from shape_model.point_cloud_registration import (DeformableRegistration, RigidRegistration,  # noqa: F401
                                                          inverse_transformation_at_sampled_points, register_cpd_deformable,
                                                          interpolate_displacements_weighted_knn)
        from utils.general_utils import inverse_affine_transform  # noqa: F401
    finally:
        sys.modules.clear()
        sys.modules.update(saved)
