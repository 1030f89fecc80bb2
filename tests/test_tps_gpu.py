"""GPU tests of the thin-plate-spline kernels (csrc/tps.hip), functional.tps_* and the 'tps' interpolation mode.

The bar is the house bar: against the fp64 oracle of tests/tps_oracle.py, relative to the largest output entry, a kernel may be off
by max(4.8e-7, 4 x what the fp32 reference-form restatement is off on the same input); against the outputs of the real reference
(tests/golden/tps_ref.npz) the factor is 5 (ours at 4 plus its own 1).  The fp64 system matrix: 64 fp64 ulps of its largest entry
(sqrt is exact, log and the product within an ulp or two each; the margin covers another log implementation).  Every measured
figure is printed before it is asserted."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import kmeans_oracle as ko
import tps_oracle as to
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu
ULP64 = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "tps_ref.npz"))


@pytest.fixture(scope="module")
def F_hip():
    from fissure_segmentation_amd import functional
    return functional


@pytest.fixture(scope="module")
def pcr():
    from fissure_segmentation_amd.shape_model import point_cloud_registration
    return point_cloud_registration


def _check(name, got, want, own, factor=4):
    err, allowed = to.rel_err(got, want), to.bar(own, factor)
    print(f"{name}: off by {err:.3e}, the fp32 restatement by {own:.3e} (bar {allowed:.3e})")
    assert np.isfinite(np.asarray(got)).all(), name
    assert err <= allowed, name


def _capture(fn):
    """-> (eager result, result of one replay of fn captured in a graph)"""
    eager = fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    static.zero_()
    graph.replay()
    torch.cuda.synchronize()
    return eager, static


# ------------------------------------------------------------------ the system matrix
@pytest.mark.parametrize("n", [1, 4, 5, 63, 64, 65, 257])
def test_system_matrix(device, F_hip, n):
    clouds = [to.control_points(n, 10 * n + b, duplicates=1 if n >= 4 and b == 1 else 0) for b in range(3)]
    for lambd in (0., 0.1):
        batch = F_hip.tps_system(torch.from_numpy(np.stack(clouds)).to(device), lambd)
        assert batch.shape == (3, n + 4, n + 4) and batch.dtype == torch.float64
        alone = F_hip.tps_system(torch.from_numpy(clouds[1]).to(device), lambd)          # B = 1, given 2-D
        assert alone.shape == (n + 4, n + 4) and torch.equal(alone, batch[1])
        for b, c in enumerate(clouds):
            A, want = batch[b].cpu().numpy(), to.system64(c, lambd)
            assert np.array_equal(A, A.T), "not symmetric bit for bit"
            assert np.array_equal(np.diag(A)[:n], np.full(n, lambd))
            assert np.array_equal(A[:n, n:], np.concatenate([np.ones((n, 1)), c.astype(np.float64)], 1))
            assert np.array_equal(A[n:, n:], np.zeros((4, 4)))
            err = np.abs(A - want).max()
            allowed = 64 * ULP64 * max(np.abs(want[:n, :n]).max(), np.finfo(np.float64).tiny)
            print(f"n={n} lambda={lambd} item {b}: u block off by {err:.3e} (bar {allowed:.3e})")
            assert err <= allowed
            if n >= 4 and b == 1:
                assert A[n - 1, 0] == 0 and A[0, n - 1] == 0 and not np.signbit(A[0, n - 1])   # coincident points: u(0) = +0


# ------------------------------------------------------------------ evaluation with a given theta
@pytest.mark.parametrize("n", [1, 4, 64, 65, 257, 1025])
def test_eval_given_theta(device, F_hip, n):
    c = to.control_points(n, 20 + n)
    cd = torch.from_numpy(c).to(device)
    for C in (1, 3, 4):
        theta = to.random_theta(n, C, 30 + n + C)
        td = torch.from_numpy(theta).to(device)
        for Q in (1, 63, 65, 1025):
            x = to.queries(Q, 40 + Q, c)                     # row 0 lies ON a control point: r = 0
            got = F_hip.tps_eval(torch.from_numpy(x).to(device), cd, td)
            assert got.shape == (Q, C) and got.dtype == torch.float32
            want = to.z64(x, c, theta)
            _check(f"eval n={n} Q={Q} C={C}", got.cpu().numpy(), want, to.rel_err(to.z32(x, c, theta), want))


def test_eval_far_queries_cancel(device, F_hip):
    """|x| = 50: u is about 1e4 at every control point and the weights sum to zero"""
    for n in (64, 1025):
        c, theta, x = to.control_points(n, 50 + n), to.random_theta(n, 3, 51 + n), to.far_queries()
        got = F_hip.tps_eval(*(torch.from_numpy(a).to(device) for a in (x, c, theta)))
        want = to.z64(x, c, theta)
        _check(f"far queries n={n}", got.cpu().numpy(), want, to.rel_err(to.z32(x, c, theta), want))


@pytest.mark.parametrize("lat", [(5, 7, 9), (2, 2, 2), (1, 3, 1), (3, 1, 70)])
def test_lattice_queries_equal_explicit_ones(device, F_hip, lat):
    n, B = 65, 2
    c = torch.from_numpy(np.stack([to.control_points(n, 60 + b) for b in range(B)])).to(device)
    theta = torch.from_numpy(np.stack([to.random_theta(n, 3, 61 + b) for b in range(B)])).to(device)
    nodes = torch.from_numpy(to.lattice(*lat)).to(device)
    implied = F_hip.tps_eval(lat, c, theta)
    explicit = F_hip.tps_eval(nodes[None].expand(B, -1, -1).contiguous(), c, theta)
    assert implied.shape == (B, lat[0] * lat[1] * lat[2], 3) and torch.equal(implied, explicit)
    assert torch.equal(F_hip.tps_eval(lat, c[1], theta[1]), implied[1])


# ------------------------------------------------------------------ fit plus evaluation
@functools.lru_cache(maxsize=None)
def _fit_case(n, lambd):
    c, f, x = to.control_points(n, 70 + n), to.rough_values(n, 3, 70 + n), to.queries(65, 70 + n)
    x[0] = c[0]
    want = to.z64(x, c, to.fit64(c, f, lambd))
    return c, f, x, want, to.rel_err(to.z32(x, c, to.fit32(c, f, lambd)), want)


@pytest.mark.parametrize("n,lambd", [(5, 0.1), (64, 0.1), (257, 0.1), (1024, 0.1), (5, 0.), (64, 0.)])
def test_fit_and_eval(device, F_hip, pcr, n, lambd):
    c, f, x, want, own = _fit_case(n, lambd)
    cd, fd, xd = (torch.from_numpy(a).to(device) for a in (c, f, x))
    theta = F_hip.tps_fit(cd, fd, lambd)
    assert theta.shape == (n + 4, 3) and theta.dtype == torch.float64
    _check(f"fit + eval n={n} lambda={lambd}", F_hip.tps_eval(xd, cd, theta).cpu().numpy(), want, own)
    # the class with the reference's signatures is the same two calls
    assert torch.equal(pcr.TPS.fit(cd, fd, lambd), theta) and torch.equal(pcr.TPS.z(xd, cd, theta), F_hip.tps_eval(xd, cd, theta))
    if n == 64:   # fit_batch only sets how many systems are solved at once
        batch = F_hip.tps_fit(torch.stack([cd, cd.flip(0), cd]), torch.stack([fd, fd.flip(0), fd]), lambd, fit_batch=2)
        _check("fit in chunks of 2", F_hip.tps_eval(xd, cd, batch[2]).cpu().numpy(), want, own)


@pytest.mark.parametrize("n", to.GOLDEN_FIT)
def test_fit_and_eval_against_the_reference(device, F_hip, golden, n):
    c, f, x = to.golden_fit_inputs(n)
    cd, fd, xd = (torch.from_numpy(a).to(device) for a in (c, f, x))
    own = to.rel_err(to.z32(x, c, to.fit32(c, f, to.LAMBDA)), to.z64(x, c, to.fit64(c, f, to.LAMBDA)))
    _check(f"fixture fit{n}_z", F_hip.tps_eval(xd, cd, F_hip.tps_fit(cd, fd, to.LAMBDA)).cpu().numpy(), golden[f"fit{n}_z"], own, 5)
    theta = golden[f"fit{n}_theta"].astype(np.float64)
    own = to.rel_err(to.z32(x, c, theta), to.z64(x, c, theta))
    _check(f"fixture fit{n}_z at its theta", F_hip.tps_eval(xd, cd, torch.from_numpy(theta).to(device)).cpu().numpy(),
           golden[f"fit{n}_z"], own, 5)


# ------------------------------------------------------------------ grid sampling
@functools.lru_cache(maxsize=None)
def _grid_case(size, n):
    c, f = to.control_points(n, 80 + n), to.rough_values(n, 3, 80 + n)
    grid, outside = to.sample_grid(size, 81)
    want = to.dense_route64(c, to.fit64(c, f, to.LAMBDA), grid, size)
    return c, f, grid, outside, want, to.rel_err(to.route32(c, f, grid, size), want)


@pytest.mark.parametrize("size,n", [((22, 30, 37), 40), ((8, 9, 11), 40), (to.ONE_NODE_SHAPE, 40), ((8, 9, 11), 600)])
def test_grid_sample(device, F_hip, pcr, size, n):
    c, f, grid, outside, want, own = _grid_case(size, n)
    cd, fd, gd = (torch.from_numpy(a).to(device) for a in (c, f, grid))
    theta = F_hip.tps_fit(cd, fd, to.LAMBDA)
    got = F_hip.tps_grid_sample(gd, cd, theta, size, step=to.STEP)
    assert got.shape == (len(grid), 3) and got.dtype == torch.float32
    _check(f"grid_sample {size} n={n} vs the dense-route oracle", got.cpu().numpy(), want, own)
    zero = (want == 0).all(1)
    assert zero[outside].all() and np.array_equal((got.cpu().numpy() == 0).all(1), zero), "zero padding: exactly 0 where the oracle is"
    # the same route on the device: thin_plate_dense (lattice kernel + F.interpolate), then F.grid_sample
    field = pcr.thin_plate_dense(cd[None], fd[None], size, to.STEP, to.LAMBDA)
    assert field.shape == (1, *size, 3)
    dense = torch.nn.functional.grid_sample(field.permute(0, 4, 1, 2, 3), gd.view(1, -1, 1, 1, 3), align_corners=False)
    dense = dense.reshape(3, -1).t()
    _check(f"grid_sample {size} n={n} vs thin_plate_dense + grid_sample on the device", got.cpu().numpy(), dense.cpu().numpy(), own)
    _check(f"thin_plate_dense + grid_sample {size} vs the oracle", dense.cpu().numpy(), want, own)
    # Q = 1: each sample alone gives its bits
    for s in (0, 9, len(grid) - 1):
        assert torch.equal(F_hip.tps_grid_sample(gd[s:s + 1], cd, theta, size), got[s:s + 1])


def test_thin_plate_dense_against_the_reference(device, pcr, golden):
    c, f, idx = to.golden_dense_inputs()
    size = to.GOLDEN_DENSE_SHAPE
    field = pcr.thin_plate_dense(torch.from_numpy(c).to(device)[None], torch.from_numpy(f).to(device)[None], size, to.STEP,
                                 to.LAMBDA, unroll_step_size=7)
    want = to.dense_field64(c, to.fit64(c, f, to.LAMBDA), size).reshape(3, -1).t().numpy()[idx]
    D1, H1, W1 = to.coarse_size(size)
    y2 = torch.from_numpy(to.z32(to.lattice(D1, H1, W1), c, to.fit32(c, f, to.LAMBDA))).view(1, D1, H1, W1, 3).permute(0, 4, 1, 2, 3)
    yard = torch.nn.functional.interpolate(y2, size, mode="trilinear", align_corners=True)[0].reshape(3, -1).t().numpy()[idx]
    got = field.reshape(-1, 3)[torch.from_numpy(idx).to(device)].cpu().numpy()
    _check("thin_plate_dense vs the oracle", got, want, to.rel_err(yard, want))
    _check("thin_plate_dense vs the fixture", got, golden["dense_at_voxels"], to.rel_err(yard, want), 5)


# ------------------------------------------------------------------ reproducibility
def test_same_bits_again_alone_in_a_batch_and_from_a_graph(device, F_hip):
    n, B, size = 257, 3, (22, 30, 37)
    c = torch.from_numpy(np.stack([to.control_points(n, 90 + b) for b in range(B)])).to(device)
    f = torch.from_numpy(np.stack([to.rough_values(n, 3, 90 + b) for b in range(B)])).to(device)
    x = torch.from_numpy(np.stack([to.queries(65, 91 + b) for b in range(B)])).to(device)
    g = torch.from_numpy(np.stack([to.sample_grid(size, 92 + b)[0] for b in range(B)])).to(device)
    theta = F_hip.tps_fit(c, f, to.LAMBDA)
    calls = {"system": lambda s=slice(None): F_hip.tps_system(c[s], to.LAMBDA),
             "eval": lambda s=slice(None): F_hip.tps_eval(x[s], c[s], theta[s]),
             "lattice eval": lambda s=slice(None): F_hip.tps_eval((5, 7, 9), c[s], theta[s]),
             "grid_sample": lambda s=slice(None): F_hip.tps_grid_sample(g[s], c[s], theta[s], size)}
    for name, call in calls.items():
        first = call()
        assert torch.equal(call(), first), name
        for b in range(B):
            assert torch.equal(call(slice(b, b + 1))[0], first[b]), (name, b)
    for name in ("eval", "lattice eval", "grid_sample"):
        eager, replayed = _capture(calls[name])
        assert torch.equal(eager, replayed), name


# ------------------------------------------------------------------ the entry points
@pytest.mark.parametrize("shape", to.GOLDEN_IMG_SHAPES)
def test_interpolate_displacements_tps(device, pcr, golden, shape):
    e, v, q = to.golden_voxel_inputs(shape)
    ed, vd, qd = (torch.from_numpy(a).to(device) for a in (e, v, q))
    want = to.interpolate64(e, v, q, shape)
    own = to.rel_err(to.interpolate32(e, v, q, shape), want)
    got = pcr.interpolate_displacements_tps(ed, vd, qd, shape)
    assert got.is_cuda and got.shape == q.shape and got.dtype == torch.float32
    _check(f"interpolate_displacements_tps {shape} vs the oracle", got.cpu().numpy(), want, own)
    _check(f"interpolate_displacements_tps {shape} vs the fixture", got.cpu().numpy(), golden["interp_" + "_".join(map(str, shape))], own, 5)
    batch = pcr.interpolate_displacements_tps(torch.stack([ed, ed.flip(0)]), torch.stack([vd, vd.flip(0)]), torch.stack([qd, qd]), shape)
    assert torch.equal(batch[0], got)
    one = pcr.interpolate_displacements_tps(ed, vd, qd[3:4], shape)            # Q = 1
    assert one.shape == (1, 3) and torch.equal(one, got[3:4])
    if shape != to.GOLDEN_IMG_SHAPES[0]:
        return
    # inverse_transformation_at_sampled_points: numpy in, numpy out; tensors in, tensor out
    e64, v64, q64 = (a.astype(np.float64) for a in (e, v, q))
    with torch.cuda.device(device):
        out = pcr.inverse_transformation_at_sampled_points(e64, v64, q64, shape, 'tps')
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == q.shape
    _check("inverse_transformation_at_sampled_points (numpy) vs the fixture", q64 - out, q64 - golden["inverse"], own, 5)
    out_t = pcr.inverse_transformation_at_sampled_points(ed.double(), vd.double(), qd.double(), shape, 'tps')
    assert out_t.is_cuda and out_t.dtype == torch.float64 and np.array_equal(out_t.cpu().numpy(), out)
    # 'knn' does not look at the shape, and is what it was: the sample minus the kNN interpolation
    knn = pcr.inverse_transformation_at_sampled_points(ed, vd, qd, shape, 'knn')
    assert torch.equal(knn, pcr.inverse_transformation_at_sampled_points(ed, vd, qd))
    assert torch.equal(knn, qd - pcr.interpolate_displacements_weighted_knn(ed, vd, qd))


def test_data_set_correspondences_tps(device, golden, monkeypatch):
    """the points pair by pair at 5 x the fp32 restatement's own error on that pair; the four statistics at the bars of
    tests/test_correspondences_gpu.py with the interpolation bar replaced by the largest of those"""
    import test_correspondences_gpu as tc
    from fissure_segmentation_amd.shape_model.generate_corresponding_points import data_set_correspondences
    inp = ko.correspondence_inputs()
    I, O, P = ko.CORR_INSTANCES, ko.CORR_OBJECTS, ko.CORR_POINTS
    shape = to.GOLDEN_CORR_SHAPE

    def call(as_numpy, mode):
        arrays = [inp["fixed_pcs"], inp["moving_pcs"], inp["moved_pcs"], inp["displacements"]]
        if not as_numpy:
            arrays = [torch.from_numpy(a).to(device) for a in arrays]
        with torch.cuda.device(device):
            return data_set_correspondences(arrays[0], inp["meshes"], arrays[1], copy.deepcopy(inp["transforms"]), arrays[2], arrays[3],
                                            shape, None, mode="simple", undo_affine_reg=True, show=False, interpolation_mode=mode)

    got = call(True, "tps")
    max_disp = float(np.abs(inp["displacements"]).max())
    fwd_got, fwd_ref = tc._forward(got[0], inp["transforms"]), tc._forward(golden["corr_pcs"], inp["transforms"])
    worst = 0.
    for i in range(I):
        for o in range(O):
            args = (inp["moved_pcs"][i, o], inp["displacements"][i, o], inp["fixed_pcs"][o], shape)
            want = to.interpolate64(*args, sparse=True)
            own = to.rel_err(to.interpolate32(*args), want)
            sl = slice(o * P, (o + 1) * P)
            _check(f"pair ({i},{o}) vs the oracle", inp["fixed_pcs"][o] - fwd_got[i, sl], want, own)
            _check(f"pair ({i},{o}) vs the fixture", inp["fixed_pcs"][o] - fwd_got[i, sl], inp["fixed_pcs"][o] - fwd_ref[i, sl], own, 5)
            worst = max(worst, to.bar(own, 5) * np.abs(want).max() / max_disp)
    monkeypatch.setattr(tc, "INTERP_BAR", worst)
    ref = {k.replace("corr_", "tps_"): golden[k] for k in golden.files if k.startswith("corr_")}
    ref["tps_is_applied"] = np.zeros(I, bool)
    tc._compare(got, ref, "tps", inp, inp["fixed_pcs"], True)
    # GPU tensors in, GPU tensors out, the same bits; 'knn' is not touched by the shape or the new argument
    on_gpu = call(False, "tps")
    assert on_gpu[0].is_cuda and np.array_equal(on_gpu[0].cpu().numpy(), got[0])
    for k in ("mean", "std", "hd", "cf"):
        assert torch.equal(on_gpu[4][k].cpu(), got[4][k])
    monkeypatch.undo()
    knn = call(True, "knn")
    tc._compare(knn, np.load(os.path.join(GOLDEN_DIR, "correspondences_ref.npz")), "simple_undo", inp, inp["fixed_pcs"], True)
