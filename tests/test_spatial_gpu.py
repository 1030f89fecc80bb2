"""GPU tests of csrc/spatial.hip through functional.bspline_prefilter / elastic_field / spatial_transform,
augmentations.image_augmentation and utils.image_ops.resample_equal_spacing, against tests/spatial_oracle.py (scipy in fp64).
Numbers are held to the oracle's bar (4 x the fp32 restatement's own error, floor 4.8e-7 of the largest magnitude); labels are
compared voxel for voxel, a voxel excused only where its fp64 coordinate lies within 1e-3 of a decision boundary.  Every case is
tiny: volume (2, 1, 20, 24, 70), patch (12, 14, 66)."""
import functools

import numpy as np
import pytest
import torch

import spatial_oracle as so
from fissure_segmentation_amd import augmentations as aug
from fissure_segmentation_amd import functional as F
from fissure_segmentation_amd.utils import image_ops

pytestmark = pytest.mark.gpu

SETS = (0, 1, 2, 3)
START = (3, 4, 2)                # the crop of the identity test


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # (a copy: the oracle's arrays are read-only)


def _params(k, dev, keys=("matrix", "centre", "elastic")):
    p = so.parameter_set(k)
    return {key: _t(p[key], dev) for key in keys}


@functools.lru_cache(maxsize=None)
def _coords(k):
    p = so.parameter_set(k)
    c = so.coordinates(p["matrix"], p["centre"], p["elastic"], so.PATCH)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _image_refs(k, order):
    p = so.parameter_set(k)
    want = so.sample_image(so.volume(), _coords(k), order)
    r32 = so.restate_image(so.volume(), p["matrix"], p["centre"], p["elastic"], so.PATCH, order, np.float32)
    want.setflags(write=False)
    return want, r32


@functools.lru_cache(maxsize=None)
def _label_refs(k, order):
    want = so.sample_labels(so.labels(), _coords(k), order)
    ex = so.excused(so.labels(), _coords(k), order)
    want.setflags(write=False)
    return want, ex


def _vol(dev):
    return _t(so.volume().astype(np.float32), dev)


def _seg(dev, dtype=torch.int64):
    return _t(so.labels(), dev).to(dtype)


# ------------------------------------------------------------------------------------------------ numerical parity
def test_prefilter_matches_the_restatement(device):
    coef = F.bspline_prefilter(_vol(device))
    assert coef.dtype == torch.float32 and coef.shape == (2, 1, 44, 48, 94)
    ok, msg = so.bar("prefilter", coef.cpu().numpy(), so.prefilter(so.volume()), so.prefilter(so.volume(), dtype=np.float32))
    assert ok, msg


@pytest.mark.parametrize("order", [3, 1])
@pytest.mark.parametrize("k", SETS)
def test_image_matches_map_coordinates(device, k, order):
    want, r32 = _image_refs(k, order)
    img, seg = F.spatial_transform(_vol(device), None, so.PATCH, order_data=order, **_params(k, device))
    assert seg is None and img.dtype == torch.float32 and img.shape == (2, 1) + so.PATCH
    ok, msg = so.bar(f"order {order} set {k}", img.cpu().numpy(), want, r32)
    assert ok, msg
    if order == 3:          # cached coefficients give the same bits
        again, _ = F.spatial_transform(F.bspline_prefilter(_vol(device)), None, so.PATCH, prefiltered=True, **_params(k, device))
        assert torch.equal(again, img)


@pytest.mark.parametrize("k", SETS)
def test_elastic_field_matches_gaussian_filter(device, k):
    p = so.parameter_set(k)
    got = F.elastic_field(_t(p["noise"], device), _t(p["sigma"], device), _t(p["alpha"], device))
    assert got.dtype == torch.float32 and got.shape == (2, 3) + so.PATCH
    want = np.stack([float(p["alpha"][b]) * so.gaussian(p["noise"][b], float(p["sigma"][b])) for b in range(2)])
    r32 = np.stack([so.restate_gaussian(p["noise"][b], p["sigma"][b], p["alpha"][b], np.float32) for b in range(2)])
    ok, msg = so.bar(f"elastic set {k}", got.cpu().numpy(), want, r32)
    assert ok, msg


def test_elastic_field_radius_beyond_the_axes(device):
    """sigma 11 on the 12 x 14 x 66 field: the radius (44) exceeds every axis but W; numbers as sigma / alpha; a sigma outside
    (0, 255] in a TENSOR gives NaN for that item alone"""
    noise = so.parameter_set(0)["noise"]
    got = F.elastic_field(_t(noise, device), 11.0, 250.0)
    want = np.stack([250.0 * so.gaussian(noise[b], 11.0) for b in range(2)])
    r32 = np.stack([so.restate_gaussian(noise[b], 11.0, 250.0, np.float32) for b in range(2)])
    ok, msg = so.bar("elastic sigma 11", got.cpu().numpy(), want, r32)
    assert ok, msg
    mixed = F.elastic_field(_t(noise, device), torch.tensor([11.0, 300.0], device=device), 250.0)
    assert torch.equal(mixed[0], got[0]) and bool(torch.isnan(mixed[1]).all())


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("order,limit", [(0, 0.015), (1, 0.005)])
@pytest.mark.parametrize("k", SETS)
def test_labels_match_scipy_voxel_for_voxel(device, k, order, limit):
    want, ex = _label_refs(k, order)
    img, seg = F.spatial_transform(None, _seg(device), so.PATCH, order_seg=order, **_params(k, device))
    assert img is None and seg.dtype == torch.int64 and seg.shape == (2, 1) + so.PATCH
    got = seg.cpu().numpy()
    share = float(ex.mean())
    wrong = (got != want)[:, 0] & ~ex
    so.record(f"SPATIAL_PARITY labels order {order} set {k}: excused share {share:.4f}, differing inside the excuses "
              f"{int(((got != want)[:, 0] & ex).sum())}, outside {int(wrong.sum())}")
    assert share <= limit and not wrong.any()
    assert (want != 0).mean() > 0.05                                  # the scene is not empty
    for dt in (torch.uint8, torch.int32, torch.int16):                # every label type reads the same
        assert torch.equal(F.spatial_transform(None, _seg(device, dt), so.PATCH, order_seg=order, **_params(k, device))[1], seg)


# ------------------------------------------------------------------------------------------------ exact properties
def test_identity_returns_the_crop(device):
    vol, seg = _vol(device), _seg(device)
    matrix = torch.eye(3, device=device)[None].repeat(2, 1, 1)
    centre = torch.tensor([[s + (p - 1) / 2 for s, p in zip(START, so.PATCH)]] * 2, device=device)
    sl = (slice(None), slice(None)) + tuple(slice(s, s + p) for s, p in zip(START, so.PATCH))
    for order_seg in (0, 1):
        img, lab = F.spatial_transform(vol, seg, so.PATCH, matrix, centre, order_data=1, order_seg=order_seg)
        assert torch.equal(img, vol[sl]) and torch.equal(lab, seg[sl])
    img3, _ = F.spatial_transform(vol, None, so.PATCH, matrix, centre, order_data=3)
    r32 = so.restate_image(so.volume(), matrix.cpu().numpy(), centre.cpu().numpy(), None, so.PATCH, 3, np.float32)
    ok, msg = so.bar("order 3 identity", img3.cpu().numpy(), so.volume()[sl], r32)
    assert ok, msg
    img0, _ = F.spatial_transform(vol, None, so.PATCH, matrix, centre, order_data=0)
    assert torch.equal(img0, vol[sl])


def test_mirror_is_a_flip_of_the_output(device):
    vol, seg = _vol(device), _seg(device)
    p = _params(2, device)
    mirror = torch.tensor([[True, False, True], [False, True, False]], device=device)
    for order_data, order_seg in ((3, 0), (1, 1)):
        img, lab = F.spatial_transform(vol, seg, so.PATCH, order_data=order_data, order_seg=order_seg, **p)
        mi, ml = F.spatial_transform(vol, seg, so.PATCH, order_data=order_data, order_seg=order_seg, mirror=mirror, **p)
        for got, plain in ((mi, img), (ml, lab)):
            assert torch.equal(got[0], plain[0].flip(1, 3)) and torch.equal(got[1], plain[1].flip(2))
        none, _ = F.spatial_transform(vol, None, so.PATCH, order_data=order_data, mirror=torch.zeros_like(mirror), **p)
        assert torch.equal(none, img)


def test_intensity_map_is_folded_into_the_store(device):
    vol = _vol(device)
    a, b = 2.0 / 1624.0, 0.37
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    for order in (3, 1):
        plain, _ = F.spatial_transform(vol, None, so.PATCH, order_data=order, **_params(1, device))
        mapped, _ = F.spatial_transform(vol, None, so.PATCH, order_data=order, intensity=(a, b), **_params(1, device))
        x = plain.double().cpu().numpy()
        want = a32 * x + b32
        err = np.abs(mapped.double().cpu().numpy() - want)
        assert np.all(err <= 2.0 ** -23 * np.maximum(np.abs(a32 * x), np.abs(want)))        # two half-ulp roundings


def test_resample_equal_spacing(device):
    vol = so.volume()[0, 0]
    lab = so.labels()[0, 0]
    spacing, target = (0.75, 1.25, 3.0), 1.5
    size, _ = so.resample_coords(vol.shape, spacing, target)
    assert size == [10, 20, 140]
    got, new = image_ops.resample_equal_spacing(_t(vol.astype(np.float32), device), spacing, target)
    assert new == (1.5, 1.5, 1.5) and got.dtype == torch.float32 and list(got.shape) == size
    matrix = np.diag([np.float32(target / s) for s in spacing]).astype(np.float32)[None]
    centre = (matrix[0].astype(np.float64) @ np.array([(o - 1) / 2 for o in size])).astype(np.float32)[None]
    c32 = so.coordinates(matrix, centre, None, size, np.float32)[0]
    ok, msg = so.bar("resample linear", got.cpu().numpy(), so.resample(vol, spacing, target, False),
                     so.trilinear(vol.astype(np.float32), c32))
    assert ok, msg
    near, _ = image_ops.resample_equal_spacing(_t(lab, device), spacing, target, use_nearest_neighbor=True)
    assert near.dtype == torch.int64 and np.array_equal(near.cpu().numpy(), so.resample(lab, spacing, target, True).astype(np.int64))
    same = _t(lab, device)
    out, sp = image_ops.resample_equal_spacing(same, (1.5, 1.5, 1.5), 1.5)
    assert out is same and sp == (1.5, 1.5, 1.5)
    out, _ = image_ops.resample_equal_spacing(same, (1.5, 1.5, 1.51), 1.5)      # round(70 * 1.00667) = 70: still unchanged
    assert out is same


# ------------------------------------------------------------------------------------------------ reproducibility
def _pipeline(vol, seg, noise, sigma, alpha, matrix, centre, mirror):
    elastic = F.elastic_field(noise, sigma, alpha)
    coef = F.bspline_prefilter(vol)
    img, lab = F.spatial_transform(coef, seg, so.PATCH, matrix, centre, elastic=elastic, mirror=mirror, order_data=3, order_seg=1,
                                   prefiltered=True, intensity=(0.5, -0.1))
    return elastic, coef, img, lab


def test_same_bits_twice_alone_and_from_a_graph(device):
    p = _params(3, device, ("noise", "sigma", "alpha", "matrix", "centre"))
    mirror = torch.tensor([[False, True, True], [True, False, False]], device=device)
    args = (_vol(device), _seg(device), p["noise"], p["sigma"], p["alpha"], p["matrix"], p["centre"], mirror)
    first = _pipeline(*args)
    again = _pipeline(*args)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    for b in range(2):
        alone = _pipeline(*(a[b:b + 1] for a in args))
        assert all(torch.equal(x[0], y[b]) for x, y in zip(alone, first))
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph):
            cap = _pipeline(*args)
    torch.cuda.current_stream().wait_stream(side)
    for c in cap:
        c.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(cap, first))


# ------------------------------------------------------------------------------------------------ image_augmentation
def test_image_augmentation_end_to_end(device):
    vol, seg = _vol(device), _seg(device)
    patch = (8, 10, 34)
    gen = torch.Generator(device=device)
    gen.manual_seed(11)
    img, lab, params = aug.image_augmentation(vol, seg, patch, generator=gen, return_params=True)
    assert img.dtype == torch.float32 and img.shape == (2, 1) + patch and lab.dtype == torch.int64 and lab.shape == (2, 1) + patch
    assert bool(torch.isfinite(img).all()) and set(torch.unique(lab).tolist()) <= set(np.unique(so.labels()).tolist())
    gen.manual_seed(11)
    img2, lab2 = aug.image_augmentation(vol, seg, patch, generator=gen)
    assert torch.equal(img, img2) and torch.equal(lab, lab2)
    gen.manual_seed(12)
    assert not torch.equal(aug.image_augmentation(vol, seg, patch, generator=gen)[0], img)
    img3, lab3 = F.spatial_transform(vol, seg, patch, **params)
    assert torch.equal(img, img3) and torch.equal(lab, lab3)
    gen.manual_seed(11)                  # a data set keeps the coefficients: the same patch from them
    img4, lab4 = aug.image_augmentation(F.bspline_prefilter(vol), seg, patch, generator=gen, prefiltered=True)
    assert torch.equal(img, img4) and torch.equal(lab, lab4)
    gen.manual_seed(11)                  # normalize_img folded in
    img5, _ = aug.image_augmentation(vol, seg, patch, generator=gen, intensity=(0.25, -1.0))
    assert torch.allclose(img5, img * 0.25 - 1.0, rtol=0, atol=1e-6)
    # the draws: centres at least half a patch from every border, parameters inside their ranges, both mirror states seen
    gen.manual_seed(5)
    p = aug.random_spatial_parameters(512, so.VOLUME[2:], patch, generator=gen)
    lo = torch.tensor([q // 2 for q in patch], device=device)
    hi = torch.tensor([n - q // 2 for n, q in zip(so.VOLUME[2:], patch)], device=device)
    assert bool((p["centre"] >= lo).all()) and bool((p["centre"] <= hi).all())
    assert p["matrix"].shape == (512, 3, 3) and p["mirror"].dtype == torch.bool and p["mirror"].shape == (512, 3)
    scale = torch.linalg.det(p["matrix"].double()).abs() ** (1 / 3)
    assert 0.8 - 1e-6 <= float(scale.min()) and float(scale.max()) <= 1.2 + 1e-6
    rot = p["matrix"].double() / scale[:, None, None]
    assert float((rot @ rot.transpose(1, 2) - torch.eye(3, device=device, dtype=torch.float64)).abs().max()) < 1e-5
    assert 10 <= float(p["sigma"].min()) and float(p["sigma"].max()) <= 13 and 0 <= float(p["alpha"].min()) <= float(p["alpha"].max()) <= 1000
    frac = float(p["mirror"].any(1).double().mean())
    assert 0.5 < frac < 0.72                     # 0.7 * (1 - 0.5^3) = 0.61
