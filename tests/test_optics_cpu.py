"""CPU tests of the OPTICS port: the checkers themselves (tests/optics_oracle.py -- the two restatements of csrc/optics.hip's
rule against each other and against sklearn's compute_optics_graph), the host xi extraction (shape_model/optics.py) against
sklearn's cluster_optics_xi, hand cases of the ordering, and every refusal that happens before a launch."""
import numpy as np
import pytest
import torch

import optics_oracle as oo


@pytest.fixture(scope="module")
def cases():
    """name -> (points, min_samples, eps, graph by the heap restatement, graph by the matrix restatement)"""
    return {name: (X, k, eps, oo.graph(X, k, eps), oo.graph_brute(X, k, eps)) for name, X, k, eps in oo.cpu_cases()}


CASE_NAMES = [c[0] for c in oo.cpu_cases()]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_two_restatements_agree_bit_for_bit(cases, name):
    _, _, _, g, gb = cases[name]
    assert oo.same_graph(g, gb)
    n = len(g["ordering"])
    assert sorted(g["ordering"].tolist()) == list(range(n)) and np.isfinite(g["reach2"]).sum() > n // 2


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_sklearn_graph(cases, name):
    """same ordering and predecessors; sklearn rounds its distances to 15 decimals and takes roots before it compares, so the
    values agree to rounding, not to the bit"""
    cluster = pytest.importorskip("sklearn.cluster")
    X, k, eps, g, _ = cases[name]
    order, core, reach, pred = cluster.compute_optics_graph(X.astype(np.float64), min_samples=k, max_eps=eps, metric="minkowski",
                                                            p=2, metric_params=None, algorithm="auto", leaf_size=30, n_jobs=None)
    assert np.array_equal(order, g["ordering"]) and np.array_equal(pred, g["pred"])
    for ours, theirs in ((np.sqrt(g["core2"]), core), (np.sqrt(g["reach2"]), reach)):
        assert np.array_equal(np.isinf(ours), np.isinf(theirs))
        fin = np.isfinite(theirs)
        err = np.abs(ours[fin] - theirs[fin]) / np.maximum(theirs[fin], 1e-300)
        print(name, "largest relative difference", err.max() if fin.any() else 0.0)
        assert (err <= 1e-12).all()


def _sk_labels(g, k, **kw):
    cluster = pytest.importorskip("sklearn.cluster")
    return cluster.cluster_optics_xi(reachability=np.sqrt(g["reach2"]), predecessor=g["pred"], ordering=g["ordering"],
                                     min_samples=k, **kw)[0]


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("correction", [True, False])
def test_xi_labels_equal_sklearn_on_the_case_graphs(cases, name, correction):
    from fissure_segmentation_amd.shape_model.optics import optics_xi_labels
    _, k, _, g, _ = cases[name]
    for xi, mcs in ((0.05, None), (0.02, None), (0.2, 12), (0.05, 0.05)):
        kw = dict(xi=xi, predecessor_correction=correction, min_cluster_size=mcs)
        got = optics_xi_labels(np.sqrt(g["reach2"]), g["pred"], g["ordering"], k, **kw)
        assert got.dtype == np.int64 and np.array_equal(got, _sk_labels(g, k, **kw)), (xi, mcs)


@pytest.mark.parametrize("seed", range(24))
def test_xi_labels_equal_sklearn_on_further_seeds(seed):
    """small graphs of every kind: sheets and blobs, tight and infinite radii, with and without outliers"""
    from fissure_segmentation_amd.shape_model.optics import optics_xi_labels
    rng = np.random.default_rng(100 + seed)
    n, k = int(rng.integers(150, 500)), int(rng.integers(2, 9))
    X = oo.sheet(n, seed, noise=float(rng.uniform(0.1, 3)), outliers=int(rng.integers(0, 30))) if seed % 2 \
        else oo.blobs(n, seed, centres=int(rng.integers(1, 6)), outliers=int(rng.integers(0, 30)))
    eps = [np.inf, 4.0, 9.0, 20.0][seed % 4]
    g = oo.graph(X, k, eps)
    for correction in (True, False):
        for xi in (0.05, 0.15):
            got = optics_xi_labels(torch.from_numpy(np.sqrt(g["reach2"])), torch.from_numpy(g["pred"]), g["ordering"], k, xi=xi,
                                   predecessor_correction=correction)
            assert np.array_equal(got, _sk_labels(g, k, xi=xi, predecessor_correction=correction)), (seed, correction, xi)


def test_xi_labels_on_plots_with_inf_runs_one_cluster_and_none():
    from fissure_segmentation_amd.shape_model.optics import optics_xi_labels
    # runs of inf: two far blobs and isolated points under a small radius
    rng = np.random.default_rng(3)
    X = np.concatenate([rng.normal(0, 1, (80, 3)), rng.normal(50, 1, (80, 3)), rng.uniform(100, 400, (15, 3))]).astype(np.float32)
    g = oo.graph(X, 5, 3.0)
    assert np.isinf(g["reach2"]).sum() > 10
    got = optics_xi_labels(np.sqrt(g["reach2"]), g["pred"], g["ordering"], 5)
    assert np.array_equal(got, _sk_labels(g, 5)) and got.max() >= 1 and (got[160:] == -1).all()
    # one cluster: a single tight blob
    X = rng.normal(0, 1, (200, 3)).astype(np.float32)
    g = oo.graph(X, 5, np.inf)
    got = optics_xi_labels(np.sqrt(g["reach2"]), g["pred"], g["ordering"], 5, min_cluster_size=150)
    assert np.array_equal(got, _sk_labels(g, 5, min_cluster_size=150)) and got.max() <= 0
    # no cluster: every reachability inf
    g = oo.graph(oo.lattice(40, spacing=10.0), 3, 1.0)
    assert np.isinf(g["reach2"]).all()
    got = optics_xi_labels(np.sqrt(g["reach2"]), g["pred"], g["ordering"], 3)
    assert np.array_equal(got, _sk_labels(g, 3)) and (got == -1).all()
    for bad in (dict(min_samples=1), dict(min_samples=41), dict(xi=1.5), dict(min_cluster_size=1), dict(min_cluster_size=2.0),
                dict(ordering=np.zeros(40, np.int64)), dict(predecessor=g["pred"][:5])):
        kw = {**dict(reachability=np.sqrt(g["reach2"]), predecessor=g["pred"], ordering=g["ordering"], min_samples=3), **bad}
        with pytest.raises(ValueError):
            optics_xi_labels(**kw)


def test_hand_cases_of_the_ordering():
    # two far blobs: the walk through the first one ends, and it restarts with inf at the lowest unprocessed index
    a = np.array([[0, 0, 0], [100, 0, 0], [1, 0, 0], [101, 0, 0], [2, 0, 0], [102, 0, 0]], np.float32)
    for g in (oo.graph(a, 2, 5.0), oo.graph_brute(a, 2, 5.0)):
        assert g["ordering"].tolist() == [0, 2, 4, 1, 3, 5] and g["pred"].tolist() == [-1, -1, 0, 1, 2, 3]
        assert g["reach2"].tolist() == [np.inf, np.inf, 1.0, 1.0, 1.0, 1.0] and g["core2"].tolist() == [1.0] * 6
    # all duplicates: every distance 0, the order is the index order, everybody's predecessor is point 0
    d = np.full((7, 3), 2.5, np.float32)
    for g in (oo.graph(d, 3, 1.0), oo.graph_brute(d, 3, np.inf)):
        assert g["ordering"].tolist() == list(range(7)) and g["pred"].tolist() == [-1] + [0] * 6
        assert g["reach2"].tolist() == [np.inf] + [0.0] * 6 and g["core2"].tolist() == [0.0] * 7
    # a 1-D lattice, eps exactly one spacing: the edge is inclusive (d2 = e2 = 1 is a neighbour); with k = 3 the end points have
    # two neighbours only (core inf): point 0 starts the walk and updates nobody, the walk restarts at 1 and runs up the line
    lat = oo.lattice(6)
    for g in (oo.graph(lat, 3, 1.0), oo.graph_brute(lat, 3, 1.0)):
        assert g["core2"].tolist() == [np.inf, 1.0, 1.0, 1.0, 1.0, np.inf]
        assert g["ordering"].tolist() == [0, 1, 2, 3, 4, 5] and g["pred"].tolist() == [-1, -1, 1, 2, 3, 4]
        assert g["reach2"].tolist() == [np.inf, np.inf, 1.0, 1.0, 1.0, 1.0]
    g = oo.graph_brute(lat[[2, 0, 1, 3]], 2, 1.0)   # points 2, 0, 1, 3: start at row 0 (x = 2); rows 2 and 3 tie at reach 1
    assert g["ordering"].tolist() == [0, 2, 1, 3] and g["pred"].tolist() == [-1, 2, 0, 0]
    # just below one spacing nobody has a neighbour
    g = oo.graph(lat, 2, np.nextafter(1.0, 0.0))
    assert np.isinf(g["core2"]).all() and g["ordering"].tolist() == list(range(6)) and (g["pred"] == -1).all()
    for bad in ((lat[:, :2], 2, 1.0), (lat.astype(np.float64), 2, 1.0), (lat, 1, 1.0), (lat, 7, 1.0), (lat, 2, 0.0), (lat, 2, -1.0)):
        with pytest.raises(ValueError):
            oo.graph(*bad)


def test_centroid_helpers_agree():
    from fissure_segmentation_amd.shape_model.optics import cluster_means
    X = oo.sheet(300, 9)
    labels = np.random.default_rng(0).integers(-1, 4, 300)
    assert np.array_equal(cluster_means(X, labels), oo.centroids_sequential(X, labels))
    assert cluster_means(X, np.full(300, -1)).shape == (0, 3)


# ------------------------------------------------------------------ refusals before any launch
def test_python_refusals():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd import _lib
    from fissure_segmentation_amd.shape_model.optics import optics_cluster_centroids
    pts = torch.zeros(2, 10, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.optics(pts, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.optics(pts[0], 3, 2.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.optics(pts, 3, torch.ones(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU only"):
        optics_cluster_centroids(pts[0], 3, 2.0)
    with pytest.raises(TypeError):
        F_hip.optics(pts.numpy(), 3)
    with pytest.raises(TypeError):
        optics_cluster_centroids(pts[0].numpy(), 3)
    big = torch.zeros(1, 70, 3)
    for bad in (dict(points=pts[..., :2]), dict(points=pts[None]), dict(points=pts.long()), dict(points=pts[:0]),
                dict(min_samples=1), dict(min_samples=11), dict(min_samples=3.0), dict(min_samples=True),
                dict(points=big, min_samples=_lib.OPTICS_MAX_MIN_SAMPLES + 1), dict(points=pts[:, :1], min_samples=2),
                dict(max_eps=0.0), dict(max_eps=-1.0), dict(max_eps=float("nan")), dict(max_eps="1"),
                dict(max_eps=torch.ones(3)), dict(max_eps=torch.ones(2, 1)), dict(max_eps=torch.ones(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            F_hip.optics(**{**dict(points=pts, min_samples=3), **bad})
    with pytest.raises(ValueError):
        optics_cluster_centroids(pts, 3)
    assert _lib.OPTICS_MAX_POINTS >= 131072 and _lib.OPTICS_MAX_MIN_SAMPLES == 64


def test_cluster_mode_reaches_the_device_path():
    """fails without the feature: with a positive divisor the 'cluster' mode is served, so CPU tensors are refused as such"""
    from fissure_segmentation_amd.shape_model import generate_corresponding_points as gcp
    a4, a3 = np.zeros((32, 1, 6, 3)), np.zeros((1, 6, 3))
    t3, t4 = torch.from_numpy(a3), torch.from_numpy(a4)
    with pytest.raises(RuntimeError, match="GPU only"):
        gcp.data_set_correspondences(t3, [[None]] * 32, t4, [{}] * 32, t4, t4, None, None, mode="cluster",
                                     optics_minsamples_divisor=16)
    # a divisor that gives sklearn no valid min_samples keeps the refusal, before anything else is looked at
    for divisor in (-1, 0, 2.0, None):
        with pytest.raises(NotImplementedError, match="OPTICS.*positive divisor"):
            gcp.data_set_correspondences(a3, [[None]] * 32, a4, [{}] * 32, a4, a4, None, None, mode="cluster",
                                         optics_minsamples_divisor=divisor)
    with pytest.raises(NotImplementedError, match="Parzen mode is unfinished"):
        gcp.data_set_correspondences(a3, [[None]] * 32, a4, [{}] * 32, a4, a4, None, None, mode="parzen",
                                     optics_minsamples_divisor=16)


def test_host_side_checks_of_the_entry_point():
    from fissure_segmentation_amd import _lib
    q = _lib.lib.fsg_optics_workspace_bytes
    assert q(1, 100, 5) == 64 + 9264 * 4 + 4400 and q(3, 1000, 2) == 3 * (37120 + 44000) and q(0, 5, 2) == 0 and q(1, 0, 2) == 0
    assert q(2, 65, 2) % 16 == 0 and q(2, 65, 2) == 2 * (37120 + 2864)
    call = lambda *a: _lib.call("fsg_optics_f32", *a)   # noqa: E731
    for B, n, k in ((1, 1, 2), (1, 5, 1), (1, 5, 6), (1, 500, 65), (-1, 5, 2), (1, _lib.OPTICS_MAX_POINTS + 1, 2), (65536, 5, 2)):
        with pytest.raises(RuntimeError, match="bad shape"):
            call(16, 16, B, n, k, 16, 16, 16, 16, 16, 1 << 40, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        call(None, 16, 1, 5, 2, 16, 16, 16, 16, 16, 1 << 40, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        call(16, 16, 1, 5, 2, 16, 16, None, 16, 16, 1 << 40, None)
    with pytest.raises(RuntimeError, match="workspace of 63 bytes"):
        call(16, 16, 1, 5, 2, 16, 16, 16, 16, 16, 63, None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(16, 16, 1, 5, 2, 16, 16, 16, 16, 8, 1 << 40, None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(16, 16, 1, 5, 2, 16, 16, 16, 16, None, 1 << 40, None)
    call(None, None, 0, 5, 2, None, None, None, None, None, 0, None)   # an empty batch is no error and launches nothing


def test_new_symbols_are_in_the_library_and_the_header():
    from fissure_segmentation_amd import _lib
    for name in ("fsg_optics_workspace_bytes", "fsg_optics_f32"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["fsg_optics_f32"][0]) == 12
    assert _lib.DEFINES["FSG_OPTICS_MAX_POINTS"] == 262144 and _lib.DEFINES["FSG_OPTICS_MAX_MIN_SAMPLES"] == 64
