"""GPU tests of csrc/morphology.hip against tests/morphology_oracle.py (scipy.ndimage): ball dilation / erosion / closing /
opening on bit planes, connected components with their statistics, and the two callers (find_lobes,
multiple_objects_morphology).  Every comparison is exact equality."""
import functools

import numpy as np
import pytest
import torch

import morphology_oracle as mo
from fissure_segmentation_amd import functional as F
from fissure_segmentation_amd.data_processing import find_lobes as fl
from fissure_segmentation_amd.utils import image_ops

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 70), (9, 33, 130), (3, 4, 64), (12, 10, 1), (2, 33, 30, 37)]   # the last one: B = 2, different contents
RADII = [1, 2, 4, (1, 2, 3), (0, 0, 5)]


def _contents(shape):
    """density 0.3 and 0.7, all-zero, all-one; a batch shape draws every item on its own"""
    seed = sum(shape)
    return [mo.random_mask(shape, 0.3, seed), mo.random_mask(shape, 0.7, seed + 1), np.zeros(shape, bool), np.ones(shape, bool)]


def _each_item(fn, a):
    return fn(a) if a.ndim == 3 else np.stack([fn(x) for x in a])


def _popcount(bits):
    return int(np.unpackbits(bits.cpu().numpy().view(np.uint8)).sum())


@pytest.mark.parametrize("radius", RADII, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_morphology_equals_scipy(device, shape, radius):
    for a in _contents(shape):
        t = torch.from_numpy(a).to(device)
        for border in (0, 1):
            got = F.binary_dilate(t, radius, border=border)
            assert got.dtype == torch.bool and got.shape == t.shape
            assert np.array_equal(got.cpu().numpy(), _each_item(lambda x: mo.dilate(x, radius, border), a)), ("dilate", border)
            got = F.binary_erode(t, radius, border=border)
            assert np.array_equal(got.cpu().numpy(), _each_item(lambda x: mo.erode(x, radius, border), a)), ("erode", border)
        assert np.array_equal(F.binary_closing(t, radius).cpu().numpy(), _each_item(lambda x: mo.closing(x, radius), a)), "closing"
        assert np.array_equal(F.binary_opening(t, radius).cpu().numpy(), _each_item(lambda x: mo.opening(x, radius), a)), "opening"
        if a.ndim == 4:   # an item's result does not depend on the rest of the batch
            assert torch.equal(F.binary_closing(t[0], radius), F.binary_closing(t, radius)[0])
            assert torch.equal(F.binary_dilate(t[0], radius, border=1), F.binary_dilate(t, radius, border=1)[0])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_tail_bits_stay_clear(device, shape):
    """the words of a plane hold no bit past W after any launch: the set bits of the plane are the oracle's voxels"""
    a = _contents(shape)[0]
    t = torch.from_numpy(a).to(device)
    t4 = t if t.dim() == 4 else t[None]
    W, r = shape[-1], (2, 2, 2)
    bits = F._pack_bits(t4)
    assert bits.dtype == torch.int64 and bits.shape[-1] == (W + 63) // 64 and _popcount(bits) == int(a.sum())
    for border in (0, 1):
        assert _popcount(F._bits_dilate(bits, W, r, border=border)) == int(_each_item(lambda x: mo.dilate(x, r, border), a).sum())
        assert _popcount(F._bits_erode(bits, W, r, border=border)) == int(_each_item(lambda x: mo.erode(x, r, border), a).sum())
    assert _popcount(F._bits_dilate(bits, W, r, inv_in=True)) == int(_each_item(lambda x: mo.dilate(~x, r, 0), a).sum())
    assert _popcount(F._bits_closing(bits, W, r)) == int(_each_item(lambda x: mo.closing(x, r), a).sum())
    assert _popcount(F._bits_opening(bits, W, r)) == int(_each_item(lambda x: mo.opening(x, r), a).sum())
    assert torch.equal(F._unpack_bits(bits, W), t4)


def _slabs():
    """two slabs that touch only across the z face between two tiles of the local pass (z = 3 | 4), at one voxel"""
    m = np.zeros((8, 6, 70), bool)
    m[1:4, 1:5, 2:60] = True
    m[4:7, 1:5, 2:60] = True
    m[3] = False
    m[3, 2, 40] = True
    return m


def _single():
    m = np.zeros((5, 6, 70), bool)
    m[3, 4, 65] = True
    return m


CC_CASES = {
    "random6": (lambda: mo.random_mask((17, 19, 70), 0.45, 0), 6, 458),
    "random18": (lambda: mo.random_mask((17, 19, 70), 0.45, 0), 18, 3),
    "random26": (lambda: mo.random_mask((17, 19, 70), 0.45, 0), 26, 2),
    "serpentine6": (mo.serpentine, 6, 1),
    "serpentine26": (mo.serpentine, 26, 1),
    "checker6": (mo.checkerboard, 6, 8 * 8 * 64 // 2),
    "checker18": (mo.checkerboard, 18, 1),
    "empty": (lambda: np.zeros((5, 6, 70), bool), 6, 0),
    "full": (lambda: np.ones((5, 6, 70), bool), 6, 1),
    "single": (_single, 26, 1),
    "slabs": (_slabs, 6, 1),
    "batch": (lambda: np.stack([mo.random_mask((9, 10, 67), 0.45, 5), mo.random_mask((9, 10, 67), 0.2, 6)]), 6, None),
}


@pytest.mark.parametrize("case", list(CC_CASES), ids=str)
def test_components_equal_scipy(device, case):
    make, conn, want_n = CC_CASES[case]
    m = make()
    t = torch.from_numpy(m).to(device)
    labels, n = F.connected_components(t, conn)
    assert labels.dtype == torch.int32 and labels.shape == t.shape
    items = [m] if m.ndim == 3 else list(m)
    ns = [n] if m.ndim == 3 else n
    got = labels.cpu().numpy() if m.ndim == 4 else labels.cpu().numpy()[None]
    for i, item in enumerate(items):
        ref, ref_n = mo.label(item, conn)
        assert ns[i] == ref_n and (want_n is None or ref_n == want_n)
        assert np.array_equal(got[i], ref)
    again, n2 = F.connected_components(t, conn)
    assert n2 == n and torch.equal(again, labels)                          # two runs give equal bits
    n_max = max(ns)
    sizes, sums = F.component_stats(labels, n)
    assert sizes.dtype == torch.int64 and sums.dtype == torch.int64
    sizes, sums = sizes.cpu().numpy().reshape(len(items), n_max), sums.cpu().numpy().reshape(len(items), n_max, 3)
    relabelled = F.relabel_by_size(labels, n).cpu().numpy().reshape(got.shape)
    for i, item in enumerate(items):
        ref_sizes, ref_sums = mo.stats(got[i], ns[i])
        assert np.array_equal(sizes[i, :ns[i]], ref_sizes) and np.array_equal(sums[i, :ns[i]], ref_sums)
        assert not sizes[i, ns[i]:].any() and not sums[i, ns[i]:].any()
        assert np.array_equal(relabelled[i], mo.relabel_by_size(got[i], ns[i]))
    if m.ndim == 4:   # an item's labels do not depend on the rest of the batch
        alone, n_alone = F.connected_components(t[1], conn)
        assert n_alone == n[1] and torch.equal(alone, labels[1])


@functools.lru_cache(maxsize=None)
def _lung():
    return mo.lung_volume()


@pytest.mark.parametrize("exclude_rhf", [False, True])
def test_find_lobes_equals_the_oracle(device, exclude_rhf):
    lung, fis = _lung()
    want, ok = mo.find_lobes(fis, lung, exclude_rhf)
    assert ok
    lobes, meshes, success = fl.find_lobes(torch.from_numpy(fis).to(device), torch.from_numpy(lung).to(device), exclude_rhf)
    assert success is True and meshes == [] and lobes.dtype == torch.int64
    assert np.array_equal(lobes.cpu().numpy(), want)
    assert mo.lobe_numbering_holds(lobes.cpu().numpy(), exclude_rhf)        # from the voxels alone, not through the oracle
    assert sorted(np.bincount(want.ravel())[1:].tolist()) == (sorted([6923, 18425, 30895, 18425]) if exclude_rhf else
                                                               sorted([6923, 18425, 19638, 18425, 4192]))


@pytest.mark.parametrize("exclude_rhf", [False, True])
def test_find_lobes_drops_the_smallest_of_six_components(device, exclude_rhf):
    """one component more than lobes: the largest are picked on the device"""
    lung, fis = mo.lung_volume_six()
    want, ok = mo.find_lobes(fis, lung, exclude_rhf)
    assert ok
    lobes, _, success = fl.find_lobes(torch.from_numpy(fis).to(device), torch.from_numpy(lung).to(device), exclude_rhf)
    assert success is True and np.array_equal(lobes.cpu().numpy(), want)
    assert mo.lobe_numbering_holds(lobes.cpu().numpy(), exclude_rhf)


def test_permuted_integer_volumes(device):
    """a dense but non-contiguous int64 volume (a permuted view) gives what its logical array gives"""
    a = mo.random_mask((70, 9, 11), 0.3, 3)
    t = torch.from_numpy(a.astype(np.int64) * 7).to(device).permute(2, 1, 0)
    a = a.transpose(2, 1, 0)
    assert not t.is_contiguous() and tuple(t.shape) == a.shape == (11, 9, 70)
    assert np.array_equal(F.binary_dilate(t, 2).cpu().numpy(), mo.dilate(a, 2, 0))
    labels, n = F.connected_components(t, 6)
    ref, ref_n = mo.label(a, 6)
    assert n == ref_n and np.array_equal(labels.cpu().numpy(), ref)
    lung, fis = _lung()
    for exclude_rhf in (False, True):   # (the comparison with 3 and the where keep the permuted strides)
        want, ok = mo.find_lobes(fis, lung, exclude_rhf)
        f = torch.from_numpy(np.ascontiguousarray(fis.transpose(2, 1, 0)).astype(np.int64)).to(device).permute(2, 1, 0)
        m = torch.from_numpy(np.ascontiguousarray(lung.transpose(1, 0, 2)).astype(np.int64)).to(device).permute(1, 0, 2)
        assert not f.is_contiguous() and not m.is_contiguous()
        lobes, _, success = fl.find_lobes(f, m, exclude_rhf)
        assert ok and success is True and np.array_equal(lobes.cpu().numpy(), want)


def test_find_lobes_without_fissures_returns_the_components(device):
    lung, fis = _lung()
    want, ok = mo.find_lobes(np.zeros_like(fis), lung)
    assert not ok
    comp, meshes, success = fl.find_lobes(torch.zeros_like(torch.from_numpy(fis)).to(device), torch.from_numpy(lung).to(device))
    assert success is False and meshes == [] and comp.dtype == torch.int32
    assert np.array_equal(comp.cpu().numpy(), want)


@pytest.mark.parametrize("mode", ["dilate", "erode"])
def test_multiple_objects_morphology_equals_the_sequential_loop(device, mode):
    m = mo.three_label_map()
    got = image_ops.multiple_objects_morphology(torch.from_numpy(m).to(device), 2, mode)
    assert got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), mo.multiple_objects_morphology(m, 2, mode))
    again = image_ops.multiple_objects_morphology(torch.from_numpy(m.astype(np.int64)).to(device), (2, 2, 2), mode)
    assert torch.equal(again, got)
