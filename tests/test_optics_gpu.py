"""GPU tests of the OPTICS port (csrc/optics.hip, functional.optics, shape_model/optics.py, the 'cluster' mode of
data_set_correspondences).  Everything is compared bit for bit with tests/optics_oracle.py's `graph`: the squares core2 and
reach2, the ordering and the predecessors."""
import copy

import numpy as np
import pytest
import torch

import kmeans_oracle as ko
import optics_oracle as oo

pytestmark = pytest.mark.gpu
CAP = 64   # FSG_OPTICS_MAX_MIN_SAMPLES


def _run(device, X, k, eps):
    from fissure_segmentation_amd import functional as F_hip
    t = torch.from_numpy(np.ascontiguousarray(X)).to(device)
    return F_hip.optics(t, k, eps, return_squared=True)


def _equal(got, g, item=None):
    o, c, r, p = [(t if item is None else t[item]).cpu().numpy() for t in got]
    assert o.dtype == np.int64 and p.dtype == np.int64 and c.dtype == np.float64 and r.dtype == np.float64
    first = int(np.argmax(o != g["ordering"])) if not np.array_equal(o, g["ordering"]) else -1
    assert first < 0, f"ordering differs first at step {first}: {o[first]} for {g['ordering'][first]}"
    assert np.array_equal(c.view(np.int64), g["core2"].view(np.int64)), "core2"
    assert np.array_equal(r.view(np.int64), g["reach2"].view(np.int64)), "reach2"
    assert np.array_equal(p, g["pred"]), "pred"


def _dense_sheet(n, seed, outliers=0):
    """a sheet with about 0.44 points per unit area whatever n is"""
    return oo.sheet(n, seed, noise=0.3, outliers=outliers, size=1.5 * np.sqrt(n))


def _eps_for(k):
    """a radius with about 1.5 k points in it on _dense_sheet: cores both finite and inf occur"""
    return float(np.sqrt(1.5 * k / (0.44 * np.pi)))


SIZES = [(n, min(k, n)) for n in (2, 63, 64, 65, 1025, 4097) for k in (2, 5, CAP)]
SIZES = sorted(set(SIZES))


@pytest.mark.parametrize("n,k", SIZES)
def test_sizes_and_min_samples(device, n, k):
    X = _dense_sheet(n, 10 + n, outliers=n // 20)
    eps = _eps_for(k) if 4 * k <= n else np.inf   # (a cloud of about k points: everybody within reach, all cores finite)
    g = oo.graph(X, k, eps)
    if n > 100:
        assert np.isfinite(g["core2"]).any() and np.isinf(g["core2"]).any()
    _equal(_run(device, X, k, eps), g)


def test_more_than_1024_blocks(device):
    """n = 66 000 is 1 032 blocks of 64 slots: a thread of the ordering kernel holds more than one block minimum"""
    n, k, eps = 66000, 5, 3.0
    X = _dense_sheet(n, 77, outliers=500)
    g = oo.graph(X, k, eps)
    assert 0.5 < np.isfinite(g["reach2"]).mean() < 1.0
    _equal(_run(device, X, k, eps), g)


def test_eps_edges(device):
    X = _dense_sheet(1025, 5)
    extent = float((X.max(0) - X.min(0)).max())
    # tiny: nobody has a neighbour, every core is inf, the order is the index order
    got = _run(device, X, 3, 1e-6)
    assert got[0].tolist() == list(range(1025)) and torch.isinf(got[1]).all() and torch.isinf(got[2]).all() and (got[3] == -1).all()
    _equal(got, oo.graph(X, 3, 1e-6))
    # inf: one cell, everybody is everybody's neighbour
    g = oo.graph(X, 5, np.inf)
    assert np.isfinite(g["core2"]).all() and np.isinf(g["reach2"]).sum() == 1
    _equal(_run(device, X, 5, np.inf), g)
    # finite: the grid at its cap of 21 cells per axis (extent / eps = 40), below it (7 cells), and two cells
    for eps in (extent / 40, extent / 6.5, extent / 1.5):
        _equal(_run(device, X, 4, eps), oo.graph(X, 4, eps))


def test_ties_and_cells(device):
    rng = np.random.default_rng(8)
    # duplicates: every point three or more times, and a pile of forty copies of one point
    base = _dense_sheet(200, 3)
    dup = np.concatenate([base, base, base[::-1], np.repeat(base[:1], 40, 0)])
    dup = dup[rng.permutation(len(dup))]
    for k, eps in ((2, 0.5), (7, 2.0), (45, 4.0)):
        _equal(_run(device, dup, k, eps), oo.graph(dup, k, eps))
    # an integer lattice with eps exactly on a spacing (inclusive edge, ties everywhere), on the diagonal, and on two spacings
    lat = oo.lattice(12, 11, 5)
    for k, eps in ((2, 1.0), (7, 1.0), (8, float(np.sqrt(2.0))), (20, 2.0)):
        g = oo.graph(lat, k, eps)
        assert np.isfinite(g["core2"]).any()
        _equal(_run(device, lat, k, eps), g)
    shuffled = lat[rng.permutation(len(lat))]
    _equal(_run(device, shuffled, 7, 1.0), oo.graph(shuffled, 7, 1.0))
    # points on cell borders: coordinates are multiples of the cell side (eps = side here: spacing 0.5, eps 1 and 0.5)
    fine = oo.lattice(21, 9, 3, spacing=0.5)
    for k, eps in ((5, 1.0), (3, 0.5)):
        _equal(_run(device, fine, k, eps), oo.graph(fine, k, eps))
    # an offset cloud: coordinates near 1e4, where fp32 leaves a grid of 1e-3
    off = (_dense_sheet(700, 12).astype(np.float64) * 0.05 + 1e4).astype(np.float32)
    for k, eps in ((4, 0.2), (4, np.inf)):
        _equal(_run(device, off, k, eps), oo.graph(off, k, eps))


def test_batch_reproducibility_and_graph_replay(device):
    from fissure_segmentation_amd import functional as F_hip
    n, k = 1500, 5
    X = np.stack([_dense_sheet(n, 20), oo.blobs(n, 21, outliers=60), _dense_sheet(n, 22, outliers=100)])
    eps = [2.5, 6.0, np.inf]
    t = torch.from_numpy(X).to(device)
    e = torch.tensor(eps, dtype=torch.float64, device=device)
    batch = F_hip.optics(t, k, e, return_squared=True)
    graphs = [oo.graph(X[b], k, eps[b]) for b in range(3)]
    for b in range(3):
        _equal(batch, graphs[b], item=b)
        alone = F_hip.optics(t[b], k, eps[b], return_squared=True)
        assert all(torch.equal(a, c[b]) for a, c in zip(alone, batch))
    again = F_hip.optics(t, k, e, return_squared=True)
    assert all(torch.equal(a, c) for a, c in zip(again, batch))
    # the roots are torch's of the squares
    rooted = F_hip.optics(t, k, e)
    assert torch.equal(rooted[1], torch.sqrt(batch[1])) and torch.equal(rooted[2], torch.sqrt(batch[2]))
    assert torch.equal(rooted[0], batch[0]) and torch.equal(rooted[3], batch[3])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph):
            cap = F_hip.optics(t, k, e, return_squared=True)
    torch.cuda.current_stream().wait_stream(side)
    for c in cap:
        c.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(cap, batch))


def test_cluster_centroids_equal_the_oracle_pipeline_and_sklearn(device):
    cluster = pytest.importorskip("sklearn.cluster")
    from fissure_segmentation_amd.shape_model.optics import optics_cluster_centroids
    X = oo.blobs(1200, 31, centres=5, outliers=80)
    k, eps = 6, oo.heuristic_eps(X)
    want_c, want_l = oo.pipeline(X, k, eps)
    cen, lab = optics_cluster_centroids(torch.from_numpy(X).to(device), k, eps)
    assert cen.is_cuda and lab.is_cuda and cen.dtype == torch.float64 and lab.dtype == torch.int64
    assert want_l.max() >= 1 and np.array_equal(lab.cpu().numpy(), want_l)
    assert np.array_equal(cen.cpu().numpy().view(np.int64), want_c.view(np.int64))
    sk = cluster.OPTICS(min_samples=k, max_eps=eps).fit(X.astype(np.float64))
    assert np.array_equal(sk.labels_, want_l)


# ------------------------------------------------------------------ data_set_correspondences(mode='cluster')
I, O, P, DIVISOR = 16, 2, 64, 4


@pytest.fixture(scope="module")
def inputs():
    return ko.correspondence_inputs(seed=11, instances=I, objects=O, P=P)


def _call(inp, device, as_numpy=True, fixed=None, **kw):
    from fissure_segmentation_amd.shape_model.generate_corresponding_points import data_set_correspondences
    transforms = copy.deepcopy(inp["transforms"])
    arrays = [inp["fixed_pcs"] if fixed is None else fixed, inp["moving_pcs"], inp["moved_pcs"], inp["displacements"]]
    if not as_numpy:
        arrays = [torch.from_numpy(a).to(device) for a in arrays]
    with torch.cuda.device(device):
        return data_set_correspondences(arrays[0], inp["meshes"], arrays[1], transforms, arrays[2], arrays[3], None, None,
                                        show=False, **kw)


def test_cluster_mode_is_its_public_pieces(device, inputs):
    from fissure_segmentation_amd.shape_model import generate_corresponding_points as gcp
    got = _call(inputs, device, mode="cluster", optics_minsamples_divisor=DIVISOR)
    assert all(isinstance(a, np.ndarray) for a in (got[0], got[2], got[3])) and not any(v.is_cuda for v in got[4].values())
    # the centroids are the oracle pipeline's on every object's pool, with the reference's radius
    pools = inputs["moved_pcs"].transpose(1, 0, 2, 3).reshape(O, I * P, 3).astype(np.float32)
    cents = []
    for o in range(O):
        eps = (inputs["moved_pcs"][:, o].max() - inputs["moved_pcs"][:, o].min()) * 0.05   # of the fp64 coordinates as given
        cents.append(oo.pipeline(pools[o], I // DIVISOR, eps)[0])
    counts = [len(c) for c in cents]
    assert min(counts) >= 1 and counts[0] != counts[1], counts   # ragged: the objects differ in their cluster counts
    assert np.array_equal(got[2].view(np.int64), np.concatenate(cents).view(np.int64))
    assert got[3].tolist() == [1] * counts[0] + [2] * counts[1] and got[0].shape == (I, sum(counts), 3)
    assert [t["is_applied"] for t in got[1]] == [False] * I
    # the rest is object_correspondences called by hand with those centroids
    t = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
    s, R, tr = gcp._transforms(inputs["transforms"], I, device)
    at = 0
    for o in range(O):
        one = gcp.object_correspondences(t(cents[o]), t(inputs["moved_pcs"][:, o]), t(inputs["displacements"][:, o]),
                                         t(inputs["moving_pcs"][:, o]), [inputs["meshes"][i][o] for i in range(I)], s, R, tr, True)
        assert np.array_equal(one[0].cpu().numpy(), got[0][:, at:at + counts[o]])
        for j, key in enumerate(("mean", "std", "hd", "cf")):
            assert torch.equal(one[1 + j].cpu(), got[4][key][:, o]), (key, o)
        at += counts[o]
    # GPU tensors in, GPU tensors out, the same bits
    on_gpu = _call(inputs, device, as_numpy=False, mode="cluster", optics_minsamples_divisor=DIVISOR)
    assert all(a.is_cuda for a in (on_gpu[0], on_gpu[2], on_gpu[3])) and all(v.is_cuda for v in on_gpu[4].values())
    for a, b in zip((got[0], got[2], got[3]), (on_gpu[0], on_gpu[2], on_gpu[3])):
        assert np.array_equal(a, b.cpu().numpy())
    for key in ("mean", "std", "hd", "cf"):
        assert torch.equal(got[4][key], on_gpu[4][key].cpu())
    # a divisor that leaves min_samples below 2 is sklearn's ValueError
    with pytest.raises(ValueError, match="min_samples"):
        _call(inputs, device, mode="cluster", optics_minsamples_divisor=16)
