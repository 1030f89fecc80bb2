"""GPU tests of csrc/edt.hip against tests/edt_oracle.py (scipy.ndimage.distance_transform_edt in fp64): the squared
distance transform in its int32 and fp32 modes, the feature transform (as a property: its tie rule is not scipy's),
determinism, `nearest_label`, `labelmap_distances` and the lung split of data_processing/process_lung_mask.py."""
import functools
import warnings

import numpy as np
import pytest
import torch

import edt_oracle as eo
from fissure_segmentation_amd import functional as F
from fissure_segmentation_amd.data_processing import process_lung_mask as plm

pytestmark = pytest.mark.gpu

BASE = (2, 19, 21, 70)      # W crosses one 64-bit word with a remainder of 6; no axis is a multiple of the wave; H != D
DENSITIES = (0.5, 0.02, 0.001)
REL = 4.8e-7                # four fp32 ulps: one rounding each in the product, the square and the two sums
INT_INF = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def _mask(density, shape=BASE):
    return eo.random_sites(shape, density, int(density * 1000) + sum(shape))      # (only ever read)


@functools.lru_cache(maxsize=None)
def _oracle(density, sampling=None, shape=BASE):
    o = np.stack([eo.edt_sq(x, sampling) for x in _mask(density, shape)])
    o.setflags(write=False)
    return o


def _within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    return np.all((got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf))))


@pytest.mark.parametrize("density", DENSITIES)
def test_unit_spacing_is_exact(device, density):
    m, want = _mask(density), _oracle(density)
    t = torch.from_numpy(m).to(device)
    d2 = F.distance_transform_edt(t, squared=True)
    assert d2.dtype == torch.int32 and d2.shape == t.shape
    assert np.array_equal(d2.cpu().numpy(), np.rint(want).astype(np.int32))
    d = F.distance_transform_edt(t)
    assert d.dtype == torch.float32 and _within_one_ulp(d.cpu().numpy(), np.sqrt(want))
    for dt in (torch.uint8, torch.int32, torch.int64):          # integer volumes: nonzero = set
        assert torch.equal(F.distance_transform_edt(t.to(dt) * 3, squared=True), d2)


@pytest.mark.parametrize("density", DENSITIES)
def test_spacing_exact_in_fp32(device, density):
    s = (2.5, 1.0, 0.75)
    want = _oracle(density, s)
    t = torch.from_numpy(_mask(density)).to(device)
    d2 = F.distance_transform_edt(t, sampling=s, squared=True)
    assert d2.dtype == torch.float32
    got = d2.cpu().numpy().astype(np.float64)
    print("max relative error", float(np.max(np.abs(got - want)[want > 0] / want[want > 0])))
    assert np.array_equal(got == 0, want == 0)
    assert np.all(np.abs(got - want) <= REL * want)
    d = F.distance_transform_edt(t, sampling=s).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(d - np.sqrt(want)) <= REL * np.sqrt(want))


def test_spacing_rounded_to_fp32(device):
    s = (0.7, 1.1, 2.3)
    s32 = tuple(float(np.float32(v)) for v in s)
    for density in DENSITIES:
        want = _oracle(density, s32)
        d2 = F.distance_transform_edt(torch.from_numpy(_mask(density)).to(device), sampling=s, squared=True)
        got = d2.cpu().numpy().astype(np.float64)
        print("density", density, "max relative error", float(np.max(np.abs(got - want)[want > 0] / want[want > 0])))
        assert np.array_equal(got == 0, want == 0)
        assert np.all(np.abs(got - want) <= REL * want)
        # and bit for bit what the restatement of the passes gives
        assert np.array_equal(d2[0].cpu().numpy(), eo.passes(_mask(density)[0], s)[0])


def test_edge_cases(device):
    z = torch.zeros(BASE, dtype=torch.bool, device=device)
    d, idx = F.distance_transform_edt(z, return_indices=True)
    assert float(d.abs().max()) == 0.0
    grid = torch.stack(torch.meshgrid(*(torch.arange(n, device=device, dtype=torch.int32) for n in BASE[1:]), indexing="ij"))
    assert torch.equal(idx, grid[None].expand(2, -1, -1, -1, -1))           # every voxel is its own site
    ones = torch.ones(BASE, dtype=torch.bool, device=device)
    for s in (None, (2.5, 1.0, 0.75)):
        d, idx = F.distance_transform_edt(ones, sampling=s, return_indices=True)
        assert bool(torch.isinf(d).all()) and bool((d > 0).all()) and bool((idx == -1).all())
    d2 = F.distance_transform_edt(ones, squared=True)
    assert d2.dtype == torch.int32 and bool((d2 == INT_INF).all())
    one_empty = ones.clone()
    one_empty[1, 3, 4, 5] = False                                            # item 0 has no site, item 1 has one
    d, idx = F.distance_transform_edt(one_empty, return_indices=True)
    assert bool(torch.isinf(d[0]).all()) and bool((idx[0] == -1).all()) and bool(torch.isfinite(d[1]).all())
    assert bool((idx[1] == torch.tensor([3, 4, 5], device=device, dtype=torch.int32)[:, None, None, None]).all())
    # one site in each of two opposite corners: the full-length outward walk, +inf rows and planes through passes 2 and 3
    corners = np.ones(BASE, bool)
    corners[0, 0, 0, 0] = corners[1, -1, -1, -1] = False
    t = torch.from_numpy(corners).to(device)
    for s in (None, (2.5, 1.0, 0.75)):
        d2 = F.distance_transform_edt(t, sampling=s, squared=True).cpu().numpy().astype(np.float64)
        want = np.stack([eo.edt_sq(x, s) for x in corners])
        assert np.array_equal(d2, np.rint(want)) if s is None else np.all(np.abs(d2 - want) <= REL * want)
    for shape, density in (((7, 9, 1), 0.1), ((1, 9, 70), 0.05), ((1, 3, 70, 130), 0.002), ((1, 3, 70, 130), 0.3),
                           ((3, 1, 1), 0.4), ((2, 5, 64), 0.05), ((2, 5, 128), 0.02)):
        m = eo.random_sites((1,) + shape, density, sum(shape))[0] if len(shape) == 3 else eo.random_sites(shape, density, sum(shape))
        want = eo.edt_sq(m) if m.ndim == 3 else np.stack([eo.edt_sq(x) for x in m])
        d2 = F.distance_transform_edt(torch.from_numpy(m).to(device), squared=True)
        assert d2.shape == m.shape and np.array_equal(d2.cpu().numpy(), np.rint(want).astype(np.int32)), shape


@pytest.mark.parametrize("sampling", [None, (2.5, 1.0, 0.75)], ids=str)
@pytest.mark.parametrize("density", DENSITIES)
def test_indices_name_a_site_at_the_returned_distance(device, density, sampling):
    m = _mask(density)
    t = torch.from_numpy(m).to(device)
    d2, idx = F.distance_transform_edt(t, sampling=sampling, return_indices=True, squared=True)
    assert idx.dtype == torch.int32 and idx.shape == (BASE[0], 3) + BASE[1:]
    only = F.distance_transform_edt(t, sampling=sampling, return_distances=False, return_indices=True)
    assert torch.equal(only, idx)
    assert torch.equal(d2, F.distance_transform_edt(t, sampling=sampling, squared=True))     # the same values without indices
    idx, d2 = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()
    g = np.indices(BASE[1:])
    for b in range(BASE[0]):
        z, y, x = idx[b]
        for a, n in zip((z, y, x), BASE[1:]):
            assert a.min() >= 0 and a.max() < n
        assert not m[b][z, y, x].any()
        if sampling is None:
            assert np.array_equal((g[0] - z) ** 2 + (g[1] - y) ** 2 + (g[2] - x) ** 2, d2[b])
        else:                                            # the same three roundings per term and sum, W then H then D
            s = [np.float32(v) for v in sampling]
            t0, t1, t2 = ((s[i] * np.abs(g[i] - a).astype(np.float32)) ** 2 for i, a in ((2, x), (1, y), (0, z)))
            assert np.array_equal((t0 + t1) + t2, d2[b])
        # the tie rule: the restatement of the passes picks the same site
        assert np.array_equal(np.ravel_multi_index((z, y, x), BASE[1:]), eo.passes(m[b], sampling)[1])


def test_determinism_batch_independence_and_graph_replay(device):
    t = torch.from_numpy(_mask(0.02)).to(device)
    for s in (None, (2.5, 1.0, 0.75)):
        d2, idx = F.distance_transform_edt(t, sampling=s, return_indices=True, squared=True)
        again = F.distance_transform_edt(t, sampling=s, return_indices=True, squared=True)
        assert torch.equal(d2, again[0]) and torch.equal(idx, again[1])
        for b in range(BASE[0]):
            alone = F.distance_transform_edt(t[b], sampling=s, return_indices=True, squared=True)
            assert torch.equal(alone[0], d2[b]) and torch.equal(alone[1], idx[b])
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph):
                cap = F.distance_transform_edt(t, sampling=s, return_indices=True, squared=True)
        torch.cuda.current_stream().wait_stream(side)
        cap[0].zero_()
        cap[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap[0], d2) and torch.equal(cap[1], idx)


def test_nearest_label(device):
    lab = eo.label_scene()
    t = torch.from_numpy(lab).to(device)
    got = F.nearest_label(t, (1, 2))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), eo.nearest_label(lab, (1, 2)))
    assert torch.equal(F.nearest_label(t.long(), [2, 1]), got)                        # the order given does not matter
    keep = torch.from_numpy(lab != 0).to(device)
    assert torch.equal(F.nearest_label(t, (1, 2), keep=keep), got * keep)
    s = (2.5, 1.0, 0.75)
    want = eo.nearest_label(lab, (1, 2, 7), s)
    assert np.array_equal(F.nearest_label(t, (1, 2, 7), sampling=s).cpu().numpy(), want)
    assert bool((F.nearest_label(t, (1, 9)) == 1).all())                              # a candidate without voxels is infinitely far
    sym = eo.label_scene_symmetric()
    got = F.nearest_label(torch.from_numpy(sym).to(device), (1, 2)).cpu().numpy()
    assert np.array_equal(got, eo.nearest_label(sym, (1, 2)))
    assert (got[:, :, 32] == 1).all() and (got[:, :, 33] == 2).all()                   # the equidistant plane goes to label 1


def test_lung_split_bridged(device, capsys):
    m = eo.lungs_bridged()
    t = torch.from_numpy(m).to(device)
    assert F.connected_components(t)[1] == 1
    comps, n, opened = plm.maybe_detach_mask(t)
    assert n == 2 and opened and comps.dtype == torch.int32 and "Opening with radius 3" in capsys.readouterr().out
    want, radii, warn = eo.lung_split(m)
    assert radii == [3] and not warn
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="Found .* connected components")    # two components: no warning
        got = plm.binary_lung_mask_to_left_right(t)
    assert got.dtype == torch.uint8 and got.shape == t.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got != 0, m)                                 # every voxel of the mask is labelled, nothing outside it
    assert np.argwhere(got == 2)[:, 2].mean() < np.argwhere(got == 1)[:, 2].mean()     # the right lung (smaller x) is 2
    other = plm.binary_lung_mask_to_left_right(t.to(torch.uint8), left_label=7, right_label=5).cpu().numpy()
    assert np.array_equal(other, eo.lung_split(m, 7, 5)[0]) and np.array_equal(other == 7, got == 1)


def test_lung_split_speck_and_single_ball(device, capsys):
    m = eo.lungs_speck()
    t = torch.from_numpy(m).to(device)
    with pytest.warns(UserWarning, match="Found 3 connected components"):
        got = plm.binary_lung_mask_to_left_right(t)
    assert "Opening" not in capsys.readouterr().out
    want, radii, warn = eo.lung_split(m)
    assert radii == [] and warn and np.array_equal(got.cpu().numpy(), want)
    assert int(got[2, 3, 30:35].max()) == 0 and int((torch.from_numpy(m).to(device) & (got == 0)).sum()) == 5
    with pytest.raises(ValueError, match="could not be detached"):
        plm.binary_lung_mask_to_left_right(torch.from_numpy(eo.one_ball()).to(device))
    out = capsys.readouterr().out
    assert all(f"Opening with radius {r} " in out for r in (3, 5, 7)) and "radius 9" not in out


def test_labelmap_distances(device):
    a, b = eo.slabs()
    ta, tb = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
    spacing = (1.5, 1.0, 2.0)
    want = eo.labelmap_distances(a, b, spacing)
    got = F.labelmap_distances(ta, tb, spacing)
    print("labelmap_distances", [float(g) for g in got], want)
    for g, w in zip(got, want):
        assert abs(float(g) - w) <= REL * want[2]
    swapped = F.labelmap_distances(tb, ta, spacing)
    assert all(float(g) == float(s) for g, s in zip(got, swapped))
    assert all(abs(float(g) - w) <= REL * w for g, w in zip(F.labelmap_distances(ta.to(torch.uint8) * 2, tb), eo.labelmap_distances(a, b)))
    for x, y in ((ta, torch.zeros_like(tb)), (torch.zeros_like(ta), tb)):
        assert all(bool(torch.isnan(v)) for v in F.labelmap_distances(x, y, spacing))
    big = torch.arange(20_000_000, device=device, dtype=torch.float64)[torch.randperm(20_000_000, device=device)]
    assert float(F._quantile_linear(big, 0.95)) == pytest.approx(0.95 * (20_000_000 - 1), rel=1e-12)   # above torch.quantile's limit
    small = torch.rand(1001, device=device, dtype=torch.float64)
    assert float(F._quantile_linear(small, 0.95)) == pytest.approx(eo.quantile_linear(small.cpu().numpy(), 0.95), rel=1e-12)
