"""CPU tests of the Poisson-disk sampler: the two checkers of tests/poisson_disk_oracle.py against each other (the bit-exact
restatement of csrc/poisson_disk.hip and the heap / KD-tree implementation), the pair weight against its fp64 formula, the
blue-noise property the elimination exists for, the inputs of the register_all GPU test, and every refusal before a launch."""
import numpy as np
import pytest
import torch

import poisson_disk_oracle as po

SQUARES = {"64_of_320": (64, 320), "256_of_1280": (256, 1280)}
SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def square_runs():
    """(name, seed) -> (points, R, r_min, keep, order) of oracle (a) on the unit square (area 1) at init_factor 5"""
    out = {}
    for name, (n, m) in SQUARES.items():
        R, r_min = po.radii(1.0, n, m)
        for seed in SEEDS:
            p = po.unit_square(seed, m)
            out[name, seed] = (p, R, r_min, *po.eliminate(p, n, R, r_min))
    return out


@pytest.mark.parametrize("name", list(SQUARES))
def test_restatement_equals_heap_implementation_on_the_unit_square(square_runs, name):
    n = SQUARES[name][0]
    for seed in SEEDS:
        p, R, r_min, keep, order = square_runs[name, seed]
        kb, ob = po.eliminate_heap(p, n, R, r_min)
        assert np.array_equal(order, ob) and np.array_equal(keep, kb)
        assert len(keep) == n and np.all(np.diff(keep) > 0) and len(set(order.tolist()) | set(keep.tolist())) == len(p)


def test_restatement_equals_heap_implementation_on_the_edge_cases():
    dup, R, r_min = po.duplicates_cloud()
    M = len(dup)
    d2 = po.sq_dist(dup[:, None], dup[None])
    off = ~np.eye(M, dtype=bool)
    assert (d2[off] == 0).sum() >= 8 and ((d2[off] > 0) & (np.sqrt(d2[off]) < r_min)).sum() >= 4   # duplicates, pairs below r_min
    for n_keep in (1, 7, M // 2, M - 1, M):
        a, b = po.eliminate(dup, n_keep, R, r_min), po.eliminate_heap(dup, n_keep, R, r_min)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) == n_keep and len(a[1]) == M - n_keep
    assert np.array_equal(po.eliminate(dup, M, R, r_min)[0], np.arange(M))
    # coincident rows have equal weights as long as they live: the rows 3, 10, 11 leave in index order (at most one stays)
    left = [i for i in po.eliminate(dup, 1, R, r_min)[1].tolist() if i in (3, 10, 11)]
    assert len(left) >= 2 and left == sorted(left)
    # a lattice: nearly every round is a tie of many samples
    lat, R, r_min = po.lattice()
    a, b = po.eliminate(lat, 60, R, r_min), po.eliminate_heap(lat, 60, R, r_min)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    w0 = po.initial_weights(lat, R, r_min)
    assert a[1][0] == np.flatnonzero(w0 == w0.max())[0] and (w0 == w0.max()).sum() > 100
    # an R so small that nobody has a neighbour, R = 0 and a negative R: all weights 0, removal in index order
    p = po.unit_square(4, 80)
    for R0 in (np.float32(1e-6), np.float32(0), np.float32(-1)):
        assert not po.initial_weights(p, R0, np.float32(0)).any()
        a, b = po.eliminate(p, 30, R0, np.float32(0)), po.eliminate_heap(p, 30, R0, np.float32(0))
        assert np.array_equal(a[1], np.arange(50)) and np.array_equal(a[0], np.arange(50, 80))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = po.eliminate(p[:1], 1, np.float32(1), np.float32(0))
    assert one[0].tolist() == [0] and len(one[1]) == 0


def test_pair_weight_equals_the_fp64_formula_to_fp32_rounding():
    """w = (1 - max(d, r_min) / R)^8.  fp32: the root and the quotient x = d / R <= 1 are each rounded once (2^-24 together),
    t = 1 - x once more (2^-25), so t is off by at most 1.5 * 2^-24; the eighth power multiplies that by 8 t^7 <= 8, and the
    three squarings add 2^-25 each, amplified 4, 2 and 1 times: at most (12 + 3.5) * 2^-24 in all."""
    rng = np.random.default_rng(0)
    R, r_min = np.float32(0.137), np.float32(0.021)
    d2 = (rng.random(20000).astype(np.float32) * R * R).astype(np.float32)
    d2[:4] = [0, np.float32(r_min) ** 2, np.nextafter(R * R, np.float32(0)), np.float32(1e-30)]
    w32 = po.pair_weight(d2, R, r_min)
    w64 = (1 - np.maximum(np.sqrt(d2.astype(np.float64)), float(r_min)) / float(R)) ** 8
    err = np.abs(w32.astype(np.float64) - w64).max()
    print("largest difference of the fp32 pair weight from fp64:", err, "=", err * 2 ** 24, "* 2^-24")
    assert w32.dtype == np.float32 and err <= 15.5 * 2.0 ** -24
    assert w32[0] == w32[1] == po.pair_weight(np.float32(1e-8), R, r_min) and w32.max() <= 1     # below r_min: the weight at r_min
    q = po.pair_q(d2, R, r_min)
    assert q.dtype == np.int64 and q.min() >= 0 and q.max() <= 2 ** 24 and np.array_equal(q, np.rint(w32.astype(np.float64) * 2 ** 24))
    assert po.pair_weight(np.float32(1), np.float32(0.5), np.float32(2)) == 0                     # r_min > R: clamped, not 3^8
    a, b = po.unit_square(1, 50), po.unit_square(2, 50)
    assert np.array_equal(po.sq_dist(a, b), po.sq_dist(b, a))                                     # q(i, j) = q(j, i)


@pytest.mark.parametrize("name", list(SQUARES))
def test_kept_set_is_blue_noise(square_runs, name):
    """the smallest nearest-neighbour distance of the kept set is at least 0.5 R (a plain fp64 implementation of the rule gives
    0.67 .. 0.71 R on these inputs); the first n uniform samples, what one has without the elimination, give 0.03 .. 0.2 R"""
    n = SQUARES[name][0]
    for seed in SEEDS:
        p, R, _, keep, _ = square_runs[name, seed]
        kept, raw = po.min_nn_distance(p[keep]) / R, po.min_nn_distance(p[:n]) / R
        print(name, "seed", seed, "min nearest-neighbour distance / R: kept", kept, "first n uniform samples", raw)
        assert kept >= 0.5 > raw


def test_radii_are_open3d_constants():
    R, r_min = po.radii(np.array([1.0, 4.0]), 64, 320)
    assert R.dtype == r_min.dtype == np.float32
    np.testing.assert_allclose(R, [2 * np.sqrt(1 / 64 / (2 * np.sqrt(3))), 4 * np.sqrt(1 / 64 / (2 * np.sqrt(3)))], rtol=1e-7)
    np.testing.assert_allclose(r_min / R, 0.5 * (1 - 0.2 ** 1.5), rtol=1e-6)
    assert po.radii(1.0, 10, 10)[1] == 0


# ------------------------------------------------------------------ the inputs of the register_all GPU test
def test_register_all_inputs_register_within_half_the_heuristic_distance_on_the_cpu():
    """the pipeline of register_all from the oracles alone (poisson_disk_oracle + cpd_oracle): on these inputs every registered
    point ends within half of correspondence_distance_heuristic of a fixed point, so the expected portion of correspondences
    is exactly 1 and no point sits near the threshold"""
    fixed, meshes = po.fixed_clouds(), po.moving_surfaces()
    assert fixed.shape == (po.REG_OBJECTS, po.REG_POINTS, 3) and len(meshes) == po.REG_INSTANCES
    rng = np.random.default_rng(5)
    u = [rng.random((po.REG_INSTANCES, po.REG_INIT_FACTOR * po.REG_POINTS, 3), np.float32) for _ in range(po.REG_OBJECTS)]
    r = po.register_all_cpu(fixed, meshes, u)
    print("heuristic distances", r["heuristic"], "largest distance of a registered point to its fixed cloud", r["nn"].max(2))
    assert (r["nn"] <= 0.5 * r["heuristic"][None, :, None]).all()
    # the first and the last instance are really moved: before the registration more than half of their points are farther
    # than that from the fixed cloud
    before = np.sqrt(((r["moving"][:, :, :, None] - fixed[None, :, None]) ** 2).sum(-1)).min(-1)
    far = (before > 0.5 * r["heuristic"][None, :, None]).mean((1, 2))
    print("portion of points farther than half the heuristic distance before the registration, per instance", far)
    assert far[0] > 0.5 and far[2] > 0.5


# ------------------------------------------------------------------ refusals before any launch
def test_host_side_checks_of_the_entry_point():
    from fissure_segmentation_amd import _lib
    q = _lib.lib.fsg_sample_elimination_workspace_bytes
    assert q(1, 320) == 320 * 8 and q(3, 16384) == 3 * 16384 * 8 and q(0, 5) == 0 and q(2, 0) == 0 and q(-1, 5) == 0
    run = lambda *a: _lib.call("fsg_sample_elimination_f32", *a)   # noqa: E731
    for B, M, n_keep in ((1, 0, 0), (1, 5, 0), (1, 5, 6), (-1, 5, 2), (65536, 5, 2), (1, -3, 1)):
        with pytest.raises(RuntimeError, match=r"code 1\).*bad shape"):
            run(8, 8, B, M, n_keep, 8, 8, 8, 1 << 30, None)
    with pytest.raises(RuntimeError, match=r"code 3\).*at most 16384"):
        run(8, 8, 1, 16385, 100, 8, 8, 8, 1 << 30, None)
    for args in ((None, 8, 1, 5, 2, 8), (8, None, 1, 5, 2, 8), (8, 8, 1, 5, 2, None)):
        with pytest.raises(RuntimeError, match="NULL pointer"):
            run(*args, None, 8, 1 << 30, None)
    with pytest.raises(RuntimeError, match="workspace of 39 bytes, 40 needed"):
        run(8, 8, 1, 5, 2, 8, None, 8, 39, None)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        run(8, 8, 1, 5, 2, 8, None, 4, 1 << 30, None)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        run(8, 8, 1, 5, 2, 8, None, None, 1 << 30, None)
    run(None, None, 0, 5, 2, None, None, None, 0, None)   # an empty batch is no error and launches nothing
    assert _lib.SAMPLE_ELIMINATION_MAX_POINTS == po.MAX_POINTS == 16384


def test_python_refusals():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd import mesh as M_hip
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    pts = torch.zeros(2, 10, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.sample_elimination(pts, 4, 0.1, 0.01)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.sample_elimination(pts[0], 4, 0.1, 0.01, return_order=True)
    with pytest.raises(TypeError):
        F_hip.sample_elimination(pts.numpy(), 4, 0.1, 0.01)
    for bad in (dict(points=pts[..., :2]), dict(points=pts[None]), dict(points=pts.long()), dict(points=pts[:0]), dict(n_keep=0),
                dict(n_keep=11), dict(n_keep=2.0), dict(n_keep=True), dict(points=torch.zeros(1, 16385, 3))):
        with pytest.raises(ValueError):
            F_hip.sample_elimination(**{**dict(points=pts, n_keep=4, r_max=0.1, r_min=0.01), **bad})
    square = M_hip.Meshes(torch.tensor([[[0., 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]]), torch.tensor([[0, 1, 2], [0, 2, 3]]))
    for bad in (dict(number_of_points=0), dict(number_of_points=2.5), dict(init_factor=0.5), dict(init_factor=0),
                dict(number_of_points=4000), dict(number_of_points=16385, init_factor=1)):
        with pytest.raises(ValueError):
            square.sample_points_poisson_disk(**{**dict(number_of_points=8), **bad})
    with pytest.raises(RuntimeError, match="GPU only"):
        square.sample_points_poisson_disk(8)
    with pytest.raises(RuntimeError, match="GPU only"):
        M_hip.sample_points_poisson_disk(square, 8, init_factor=2, return_indices=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        pcr.evaluate_registration(torch.zeros(5, 3), torch.zeros(6, 3), 1.0)
    with pytest.raises(TypeError):
        pcr.evaluate_registration(np.zeros((5, 3)), torch.zeros(6, 3), 1.0)
    with pytest.raises(ValueError):
        pcr.evaluate_registration(torch.zeros(2, 5, 3), torch.zeros(6, 3), 1.0)


def test_correspondence_distance_heuristic():
    from fissure_segmentation_amd.shape_model.point_cloud_registration import correspondence_distance_heuristic as h
    pc = np.array([[0., 0, 0], [3, 4, 12], [1, 1, 1]])
    assert h(pc) == pytest.approx(0.05 * 13) and isinstance(h(pc), float)
    both = np.stack([pc, 2 * pc])
    np.testing.assert_allclose(h(both), [0.65, 1.3], rtol=1e-15)
    t = h(torch.from_numpy(both))
    assert t.dtype == torch.float64 and torch.allclose(t, torch.tensor([0.65, 1.3], dtype=torch.float64), rtol=1e-15, atol=0)
    assert h(torch.from_numpy(pc)).dim() == 0
    with pytest.raises(ValueError):
        h(np.zeros((3, 2)))


def test_register_all_refuses_ragged_objects_and_bad_arguments():
    from fissure_segmentation_amd.shape_model.point_cloud_registration import register_all
    mesh = (np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match=r"\[4, 5\] points"):
        register_all([np.zeros((4, 3)), np.zeros((5, 3))], [[mesh, mesh]])
    with pytest.raises(ValueError, match=r"\[4, 5\] points"):
        register_all([torch.zeros(4, 3), torch.zeros(5, 3)], [[mesh, mesh]])
    with pytest.raises(ValueError, match="no fixed point clouds"):
        register_all([], [[mesh]])
    with pytest.raises(ValueError, match=r"must be \(points, 3\)"):
        register_all([np.zeros((4, 2))], [[mesh]])
    with pytest.raises(ValueError, match="a mesh for each of the 2 objects"):
        register_all(np.zeros((2, 4, 3)), [[mesh, mesh], [mesh]])
    with pytest.raises(ValueError, match="1 ids for 2 instances"):
        register_all(np.zeros((2, 4, 3)), [[mesh, mesh]] * 2, ids=["a"])
    with pytest.raises(ValueError, match="pair_batch"):
        register_all(np.zeros((2, 4, 3)), [[mesh, mesh]], pair_batch=0)
    with pytest.raises(RuntimeError, match="GPU only"):
        register_all(torch.zeros(2, 4, 3), [[mesh, mesh]])
