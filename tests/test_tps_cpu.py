"""CPU tests of the thin-plate-spline interpolation: the oracle of tests/tps_oracle.py against the outputs the REAL reference gave
(tests/golden/tps_ref.npz, written by tools/make_golden_tps.py), the sparse route against the dense one, and the host-side
refusals of functional.tps_* and the 'tps' interpolation mode.  Nothing here touches a GPU."""
import os

import numpy as np
import pytest
import torch

import kmeans_oracle as ko
import tps_oracle as to
from golden_util import GOLDEN_DIR


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "tps_ref.npz"))


def _within_own_error(name, fixture, yardstick, oracle):
    """the house bar, read from the reference's side: the fp32 restatement is the reference's arithmetic up to the order of its
    operations, so the two fp32 runs differ by no more than 4 x what the restatement itself is off the fp64 oracle"""
    own = to.rel_err(yardstick, oracle)
    err = to.rel_err(yardstick, fixture)
    print(f"{name}: fp32 restatement vs fixture {err:.3e}, its own error {own:.3e} (bar {to.bar(own):.3e})")
    assert err <= to.bar(own), name


# ------------------------------------------------------------------ the fixtures are what the oracle says they are
@pytest.mark.parametrize("n", to.GOLDEN_FIT)
def test_fit_and_z_fixtures(golden, n):
    c, f, x = to.golden_fit_inputs(n)
    _within_own_error(f"fit{n}_z", golden[f"fit{n}_z"], to.z32(x, c, to.fit32(c, f, to.LAMBDA)), to.z64(x, c, to.fit64(c, f, to.LAMBDA)))
    assert golden[f"fit{n}_theta"].shape == (n + 4, 3)
    # z of the RECORDED theta: the evaluation alone
    theta = golden[f"fit{n}_theta"]
    _within_own_error(f"fit{n}_z at the recorded theta", golden[f"fit{n}_z"], to.z32(x, c, theta), to.z64(x, c, theta))


def test_dense_field_fixture(golden):
    c, f, idx = to.golden_dense_inputs()
    size = to.GOLDEN_DENSE_SHAPE
    field64 = to.dense_field64(c, to.fit64(c, f, to.LAMBDA), size).reshape(3, -1).t().numpy()[idx]
    D1, H1, W1 = to.coarse_size(size)
    y2 = torch.from_numpy(to.z32(to.lattice(D1, H1, W1), c, to.fit32(c, f, to.LAMBDA))).view(1, D1, H1, W1, 3).permute(0, 4, 1, 2, 3)
    field32 = torch.nn.functional.interpolate(y2, size, mode="trilinear", align_corners=True)[0].reshape(3, -1).t().numpy()[idx]
    _within_own_error("thin_plate_dense", golden["dense_at_voxels"], field32, field64)


@pytest.mark.parametrize("shape", to.GOLDEN_IMG_SHAPES)
def test_interpolate_fixtures(golden, shape):
    e, v, q = to.golden_voxel_inputs(shape)
    want, yard = to.interpolate64(e, v, q, shape), to.interpolate32(e, v, q, shape)
    _within_own_error(f"interpolate_displacements_tps {shape}", golden["interp_" + "_".join(map(str, shape))], yard, want)
    if shape == to.GOLDEN_IMG_SHAPES[0]:
        _within_own_error("inverse_transformation_at_sampled_points", q.astype(np.float64) - golden["inverse"], yard, want)


def test_correspondence_fixture(golden):
    """one (instance, object) pair of the data_set_correspondences run (an fp32 field of the whole 256^3 image per pair)"""
    inp = ko.correspondence_inputs()
    i, o, P = 1, 1, ko.CORR_POINTS
    t = inp["transforms"][i]
    sampled = t["scale"] * golden["corr_pcs"][i, o * P:(o + 1) * P] @ t["rotation"].T + t["translation"]
    fixed = inp["fixed_pcs"][o]
    assert np.array_equal(golden["corr_fixed"], inp["fixed_pcs"].reshape(-1, 3)) and golden["corr_labels"].tolist() == [1] * P + [2] * P
    args = (inp["moved_pcs"][i, o], inp["displacements"][i, o], fixed, to.GOLDEN_CORR_SHAPE)
    _within_own_error("data_set_correspondences", fixed - sampled, to.interpolate32(*args), to.interpolate64(*args, sparse=True))


# ------------------------------------------------------------------ the sparse route is the dense route
@pytest.mark.parametrize("size", to.GRID_SHAPES + [to.ONE_NODE_SHAPE])
def test_sparse_route_equals_dense_route(size):
    c, f = to.control_points(40, 11), to.rough_values(40, 3, 11)
    theta = to.fit64(c, f, to.LAMBDA)
    grid, outside = to.sample_grid(size, 12)
    dense = to.dense_route64(c, theta, grid, size)
    sparse, most = to.sparse_route64(c, theta, grid, size)
    print(f"{size}: sparse vs dense {np.abs(dense - sparse).max():.3e} of {np.abs(dense).max():.3e}, at most {most} nodes a sample")
    assert np.abs(dense - sparse).max() <= 1e-12 * np.abs(dense).max()
    assert most <= 27
    zero = (dense == 0).all(1)
    assert zero[outside].all() and not zero[:8].any()                  # wholly outside: 0; a corner: half a voxel inside
    assert np.array_equal(zero, (sparse == 0).all(1))


@pytest.mark.filterwarnings("ignore:Since version 1.3.0")
def test_lattice_is_affine_grid():
    """the implied lattice is the reference's F.affine_grid(identity, align_corners=True) up to the rounding of its linspace"""
    for D1, H1, W1 in ((5, 7, 9), (2, 2, 2), (1, 3, 1)):
        ref = torch.nn.functional.affine_grid(torch.eye(3, 4)[None], (1, 1, D1, H1, W1), align_corners=True).view(-1, 3).numpy()
        assert np.abs(ref - to.lattice(D1, H1, W1)).max() <= 1.2e-7


# ------------------------------------------------------------------ refusals before any launch
def test_python_refusals():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.shape_model import generate_corresponding_points as gcp
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    c, v, q = torch.zeros(2, 6, 3), torch.zeros(2, 6, 3), torch.zeros(2, 5, 3)
    th = torch.zeros(2, 10, 3, dtype=torch.float64)
    for call in (lambda: F_hip.tps_system(c), lambda: F_hip.tps_fit(c, v), lambda: F_hip.tps_eval(q, c, th),
                 lambda: F_hip.tps_eval((2, 3, 4), c, th), lambda: F_hip.tps_grid_sample(q, c, th, (8, 8, 8)),
                 lambda: pcr.TPS.fit(c[0], v[0]), lambda: pcr.TPS.z(q[0], c[0], th[0]),
                 lambda: pcr.thin_plate_dense(c, v, (8, 8, 8), 4), lambda: pcr.interpolate_displacements_tps(c, v, q, (8, 9, 10)),
                 lambda: pcr.inverse_transformation_at_sampled_points(c[0], v[0], q[0], (8, 9, 10), 'tps')):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    bad = [lambda: F_hip.tps_system(c[..., :2]), lambda: F_hip.tps_system(c.long()), lambda: F_hip.tps_system(c[None]),
           lambda: F_hip.tps_fit(c, v[:, :5]), lambda: F_hip.tps_fit(c, torch.zeros(2, 6, 5)), lambda: F_hip.tps_fit(c, v, fit_batch=0),
           lambda: F_hip.tps_fit(c, v[0]), lambda: F_hip.tps_eval(q, c, th.float()), lambda: F_hip.tps_eval(q, c, th[:, :9]),
           lambda: F_hip.tps_eval(q[:1], c, th), lambda: F_hip.tps_eval(q, c, torch.zeros(2, 10, 5, dtype=torch.float64)),
           lambda: F_hip.tps_eval((2, 3), c, th), lambda: F_hip.tps_eval((0, 3, 4), c, th),
           lambda: F_hip.tps_grid_sample(q, c, th, (8, 8)), lambda: F_hip.tps_grid_sample(q, c, th, (8, 3, 8)),
           lambda: F_hip.tps_grid_sample(q, c, th, (8, 8, 8), step=0), lambda: F_hip.tps_grid_sample(q[..., :2], c, th, (8, 8, 8)),
           lambda: pcr.interpolate_displacements_tps(c, v, q, (8, 3, 10)), lambda: pcr.interpolate_displacements_tps(c, v, q, (8, 10)),
           lambda: pcr.interpolate_displacements_tps(c, v[:, :5], q, (8, 9, 10)),
           lambda: pcr.thin_plate_dense(c, v, (8, 3, 8), 4)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")
    # 'tps' without an image shape stays what it was: refused before anything touches a device
    X, Y = np.zeros((5, 3)), np.zeros((6, 3))
    with pytest.raises(NotImplementedError, match="tps.*out of scope.*pass the image shape"):
        pcr.inverse_transformation_at_sampled_points(Y, Y, X, None, interpolation_mode='tps')
    a4, a3 = np.zeros((2, 1, 6, 3)), np.zeros((1, 6, 3))
    with pytest.raises(NotImplementedError, match="tps.*out of scope.*pass the image shape"):
        gcp.data_set_correspondences(a3, [[None]] * 2, a4, [{}] * 2, a4, a4, None, None, mode="simple", interpolation_mode="tps")
    with pytest.raises(NotImplementedError, match="tps.*out of scope"):
        gcp.object_correspondences(c[0], c, c, c, [None] * 2, None, None, None, interpolation_mode='tps')
    with pytest.raises(ValueError, match="interpolation_mode must be one of"):
        gcp.object_correspondences(c[0], c, c, c, [None] * 2, None, None, None, interpolation_mode='linear')
    assert pcr.INTERPOLATION_MODES == ['knn', 'tps'] and gcp.INTERPOLATION_MODES is pcr.INTERPOLATION_MODES
    assert (pcr.TPS_STEP, pcr.TPS_LAMBDA) == (to.STEP, to.LAMBDA) == (4, 0.1)
    # the two plain formulas run anywhere
    r = pcr.TPS.d(torch.tensor([[0., 0., 0.], [3., 4., 0.]]), torch.tensor([[0., 0., 0.]]))
    assert r.tolist() == [[0.], [5.]] and pcr.TPS.u(r)[0, 0] == 0 and abs(float(pcr.TPS.u(r)[1, 0]) - 25 * np.log(5 + 1e-6)) < 1e-5


def test_host_side_checks_of_the_entry_points():
    from fissure_segmentation_amd import _lib
    null = None
    for name, args in (("fsg_tps_system_f64", (null, 1, 0, 0.1, null, null)), ("fsg_tps_system_f64", (null, 1, 40000, 0.1, null, null)),
                       ("fsg_tps_system_f64", (null, 1, 5, float("nan"), null, null)), ("fsg_tps_system_f64", (null, 1, 5, 0.1, null, null)),
                       ("fsg_tps_eval_f32", (null, null, null, 1, 5, 4, 5, 0, 0, 0, null, null)),
                       ("fsg_tps_eval_f32", (null, null, null, 1, 5, 4, 3, 1, 2, 2, null, null)),
                       ("fsg_tps_eval_f32", (null, null, null, 1, 4, 0, 3, 1, 2, 2, null, null)),
                       ("fsg_tps_grid_sample_f32", (null, null, null, 1, 5, 4, 3, 8, 8, 8, 2, 0, 2, null, null)),
                       ("fsg_tps_grid_sample_f32", (null, null, null, 1, 5, 4, 3, 8, 8, 8, 2, 9, 2, null, null)),
                       ("fsg_tps_grid_sample_f32", (null, null, null, 1, 5, 4, 3, 8, 8, 8, 2, 2, 2, null, null))):
        with pytest.raises(RuntimeError, match="bad shape|NULL pointer|not a number|lattice"):
            _lib.call(name, *args)
    assert _lib.lib.fsg_tps_system_f64(None, 0, 5, 0.1, None, None) == 0       # an empty batch launches nothing
