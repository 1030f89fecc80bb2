"""CPU tests of the voxel patch augmentation port (csrc/spatial.hip): the oracle's own claims (tests/spatial_oracle.py), the
scenes the GPU tests use, the declarations of the new entry points, the host-side helpers and the argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import spatial_oracle as so
from fissure_segmentation_amd import _lib, augmentations as aug
from fissure_segmentation_amd import functional as F
from fissure_segmentation_amd.utils import image_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsg_bspline_prefilter_axis_f32", "fsg_gauss_axis_f32", "fsg_spatial_resample_f32")


def _probe_coords(shape, seed, margin):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(-margin, n - 1 + margin, 4000) for n in shape])


def test_padding_12_reproduces_scipy_and_4_does_not():
    vol = so.volume()[0, 0]
    inside, around = _probe_coords(vol.shape, 1, 0.0), _probe_coords(vol.shape, 2, 3.0)
    c12 = so.prefilter(vol)
    for coords, bound in ((inside, 1e-13), (around, 1e-12)):
        want = ndi.map_coordinates(vol, coords, order=3, mode="nearest")
        err = np.abs(so.cubic(c12, coords) - want).max()
        print("padding 12, fp64 restatement against scipy:", err)
        assert err <= bound
    want = ndi.map_coordinates(vol, inside, order=3, mode="nearest")
    err4 = np.abs(so.cubic(so.prefilter(vol, pad=4), inside, pad=4) - want).max()
    print("padding 4:", err4)
    assert 1e-8 < err4 < 1e-3
    # clamping an outside coordinate onto the image instead of evaluating in the padding is a different function
    out = around[:, (around < 0).any(0) | (around > np.array(vol.shape)[:, None] - 1).any(0)]
    clamped = np.stack([np.clip(out[i], 0, n - 1) for i, n in enumerate(vol.shape)])
    assert np.abs(so.cubic(c12, clamped) - ndi.map_coordinates(vol, out, order=3, mode="nearest")).max() > 0.05


def test_coordinates_beyond_the_padding_run_into_the_edge_coefficient():
    vol = so.volume()[0, 0]
    far = np.array([[-40.0, 5.0, 30.0], [3.0, 60.0, 9.0], [200.0, -13.5, 81.2]]).T
    want = ndi.map_coordinates(vol, far, order=3, mode="nearest")
    assert np.abs(so.cubic(so.prefilter(vol), far) - want).max() <= 1e-12


def test_per_label_rule_on_a_hand_made_case():
    seg = np.zeros((2, 2, 2), np.int64)
    seg[0, 0, 0], seg[0, 0, 1], seg[1, 1, 1] = 1, 3, 2
    pts = np.array([[0, 0, .5], [0, 0, .4], [0, 0, .6], [.5, .5, .5], [0, .4, 0], [0, 0, 1.2], [-.1, 0, 0], [1, 1, 1]]).T
    got = so.labels_order1(seg, pts)
    # 1|3 tie at 0.5 each -> the larger; 0.6 of label 1; 0.6 of label 3; eight corners, 0 holds 5/8; 0.6 of label 1 against 0;
    # outside on W and on D -> 0; the corner itself
    assert got.tolist() == [3, 1, 3, 0, 1, 0, 0, 2]
    assert so.sample_labels(seg[None, None], pts[None], 0)[0, 0].tolist() == [3, 1, 3, 2, 1, 0, 0, 2]   # scipy rounds .5 up


def test_fp32_restatement_is_close_and_scenes_are_as_described():
    vol, lab = so.volume(), so.labels()
    assert set(np.unique(lab)) == {0, 1, 2, 3, 4} and lab.shape == so.VOLUME
    outside, shares0, shares1 = [], [], []
    for k in range(4):
        p = so.parameter_set(k)
        assert 2.4 < np.abs(p["elastic"]).max() < 3.3
        coords = so.coordinates(p["matrix"], p["centre"], p["elastic"], so.PATCH)
        n = np.array(so.VOLUME[2:]).reshape(1, 3, 1, 1, 1)
        outside.append(((coords < 0) | (coords > n - 1)).any(1).mean())
        shares0.append(so.excused(lab, coords, 0).mean())
        shares1.append(so.excused(lab, coords, 1).mean())
        for order in (3, 1):
            want = so.sample_image(vol, coords, order)
            r32 = so.restate_image(vol, p["matrix"], p["centre"], p["elastic"], so.PATCH, order, np.float32)
            r64 = so.restate_image(vol, p["matrix"], p["centre"], p["elastic"], so.PATCH, order, np.float64)
            assert np.abs(r64 - want).max() <= 1e-11 and np.abs(r32 - want).max() <= 2e-4 * np.abs(want).max()
        g64 = p["alpha"].astype(np.float64)[:, None, None, None, None] * np.stack(
            [so.gaussian(p["noise"][b], float(p["sigma"][b])) for b in range(2)])
        for b in range(2):
            r = so.restate_gaussian(p["noise"][b], p["sigma"][b], p["alpha"][b], np.float64)
            assert np.abs(r - g64[b]).max() <= 1e-12 * np.abs(g64).max()
    print("outside", outside, "excused order 0", shares0, "order 1", shares1)
    assert 0.05 < np.mean(outside) < 0.3 and max(shares0) <= 0.015 and max(shares1) <= 0.005
    # the sigma-11 case: the radius (44) exceeds every axis of the field but W
    noise = so.parameter_set(0)["noise"][0]
    r = so.restate_gaussian(noise, np.float32(11), np.float32(1), np.float64)
    assert so.gauss_taps(11.0, np.float64)[1] == 44 and np.abs(r - so.gaussian(noise, 11.0)).max() <= 1e-13


def test_header_and_binding_declare_the_same_entry_points():
    with open(os.path.join(ROOT, "include", "fsg_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/fsg_hip.h"
        args, res = _lib.SIGNATURES[name]
        assert len(m.group(1).split(",")) == len(args) and res is ctypes.c_int
        assert hasattr(_lib.lib, name)
    assert re.search(r"#define FSG_BSPLINE_PAD (\d+)", header).group(1) == str(_lib.BSPLINE_PAD) == str(so.PAD)
    kinds = [int(re.search(rf"#define FSG_LABEL_{k} (\d+)", header).group(1)) for k in ("U8", "I32", "I64")]
    assert kinds == [_lib.LABEL_U8, _lib.LABEL_I32, _lib.LABEL_I64]
    with open(os.path.join(ROOT, "fissure-segmentation_amd", "csrc", "Makefile")) as f:
        assert " spatial.hip" in f.read()


def test_resample_factors_and_matrix():
    assert image_ops.get_resample_factors((0.75, 0.75, 3.0), 1.5) == [0.5, 0.5, 2.0]
    assert image_ops.get_resample_factors((2.0, 1.0, 0.5)) == [2.0, 1.0, 0.5]
    mat, size = aug.spacing_resampling_matrix((101, 200, 33), (0.75, 0.75, 3.0), 1.5)
    assert size == [50, 100, 66] and mat.shape == (1, 3, 4)         # round(50.5) = 50: Python's round
    assert torch.equal(mat[0, :, :3], torch.diag(torch.tensor([0.5, 0.5, 2.0]))) and not mat[0, :, 3].any()
    size, axes = so.resample_coords((10, 11, 12), (1.0, 1.25, 0.5), 1.0)
    assert size == [10, 14, 6] and axes[1][5] == 4.0 and axes[2][3] == 6.0


def test_cpu_tensors_are_refused():
    img, seg = torch.zeros(1, 1, 6, 7, 8), torch.zeros(1, 1, 6, 7, 8, dtype=torch.int64)
    m, c = torch.eye(3)[None], torch.zeros(1, 3)
    for call in (lambda: F.bspline_prefilter(img), lambda: F.elastic_field(torch.zeros(1, 3, 4, 5, 6), 2.0, 1.0),
                 lambda: F.spatial_transform(img, seg, (4, 4, 4), m, c), lambda: F.spatial_transform(None, seg, (4, 4, 4), m, c),
                 lambda: aug.image_augmentation(img, seg, (4, 4, 4)), lambda: image_ops.resample_equal_spacing(img[0, 0], (1, 2, 1)),
                 lambda: aug.random_spatial_parameters(1, (6, 7, 8), (4, 4, 4), device="cpu")):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_argument_checks():
    img, seg = torch.zeros(2, 1, 6, 7, 8), torch.zeros(2, 1, 6, 7, 8, dtype=torch.int64)
    m, c = torch.eye(3)[None].repeat(2, 1, 1), torch.zeros(2, 3)
    with pytest.raises(ValueError, match=r"\(B, C, D, H, W\)"):
        F.bspline_prefilter(img[0])
    with pytest.raises(ValueError, match="floating-point"):
        F.bspline_prefilter(seg)
    with pytest.raises(ValueError, match="2\\^31"):
        F.bspline_prefilter(torch.zeros(1).expand(1, 1, 2048, 1024, 1024))
    with pytest.raises(ValueError, match=r"\(B, 3, pd, ph, pw\)"):
        F.elastic_field(torch.zeros(1, 2, 4, 5, 6), 2.0, 1.0)
    for bad in (0.0, -1.0, 256.0, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            F.elastic_field(torch.zeros(1, 3, 4, 5, 6), bad, 1.0)
    with pytest.raises(ValueError, match="alpha"):
        F.elastic_field(torch.zeros(2, 3, 4, 5, 6), 2.0, torch.zeros(3))
    for patch in ((4, 4), (4, 0, 4), 4):
        with pytest.raises(ValueError, match="patch_size"):
            F.spatial_transform(img, seg, patch, m, c)
    with pytest.raises(ValueError, match="neither"):
        F.spatial_transform(None, None, (4, 4, 4), m, c)
    for kw in ({"order_data": 2}, {"order_seg": 3}):
        with pytest.raises(ValueError, match="order_data must be"):
            F.spatial_transform(img, seg, (4, 4, 4), m, c, **kw)
    with pytest.raises(ValueError, match="prefiltered"):
        F.spatial_transform(img, seg, (4, 4, 4), m, c, order_data=1, prefiltered=True)
    with pytest.raises(ValueError, match="smaller than their padding"):
        F.spatial_transform(img, None, (4, 4, 4), m, c, prefiltered=True)
    with pytest.raises(ValueError, match="do not match"):
        F.spatial_transform(img, seg[:, :, :5], (4, 4, 4), m, c)
    with pytest.raises(ValueError, match="integer"):
        F.spatial_transform(img, img, (4, 4, 4), m, c)
    with pytest.raises(ValueError, match="matrix"):
        F.spatial_transform(img, seg, (4, 4, 4), m[:1], c)
    with pytest.raises(ValueError, match="matrix"):
        F.spatial_transform(img, seg, (4, 4, 4), m, c[:, :2])
    with pytest.raises(ValueError, match="elastic"):
        F.spatial_transform(img, seg, (4, 4, 4), m, c, elastic=torch.zeros(2, 3, 4, 4, 5))
    with pytest.raises(ValueError, match="mirror"):
        F.spatial_transform(img, seg, (4, 4, 4), m, c, mirror=torch.zeros(2, 3))
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        image_ops.resample_equal_spacing(img[0], (1, 1, 1))
    with pytest.raises(ValueError, match="positive"):
        image_ops.resample_equal_spacing(img[0, 0], (1, 0, 1))
    with pytest.raises(ValueError, match=r"\(B, C, D, H, W\)"):
        aug.image_augmentation(img[0], seg[0], (4, 4, 4))


def test_host_side_error_codes():
    """every argument check runs before anything is launched: the pointers are never followed"""
    lib, one = _lib.lib, 8
    assert lib.fsg_bspline_prefilter_axis_f32(one, 4, 0, 1, 16, None) == 1 and b"bad shape" in lib.fsg_last_error()
    assert lib.fsg_bspline_prefilter_axis_f32(one, 4, 5, 1, one, None) == 1 and b"in == out" in lib.fsg_last_error()
    assert lib.fsg_bspline_prefilter_axis_f32(None, 4, 5, 1, one, None) == 1 and b"NULL" in lib.fsg_last_error()
    assert lib.fsg_gauss_axis_f32(one, 0, 4, 5, 1, one, None, 16, None) == 1 and b"bad shape" in lib.fsg_last_error()
    assert lib.fsg_gauss_axis_f32(one, 1, 1 << 20, 1 << 10, 2, one, None, 16, None) == 1 and b"2^31" in lib.fsg_last_error()
    assert lib.fsg_gauss_axis_f32(one, 1, 4, 5, 1, None, None, 16, None) == 1 and b"NULL" in lib.fsg_last_error()
    ok = dict(src=one, C=1, od=3, seg=one, kind=2, Cs=1, os=0, B=1, D=6, H=7, W=8, pd=4, ph=4, pw=4, m=one, c=one)

    def resample(**kw):
        a = dict(ok, **kw)
        return lib.fsg_spatial_resample_f32(a["src"], a["C"], a["od"], a["seg"], a["kind"], a["Cs"], a["os"], a["B"], a["D"], a["H"],
                                            a["W"], a["pd"], a["ph"], a["pw"], a["m"], a["c"], None, None, 1.0, 0.0, one, one, None)
    for kw, text in (({"B": 0}, b"bad shape"), ({"pw": 0}, b"bad shape"), ({"D": 2048, "H": 1024, "W": 1024}, b"2^31"),
                     ({"src": None, "seg": None}, b"neither"), ({"m": None}, b"NULL"), ({"od": 2}, b"order_data"),
                     ({"os": 2}, b"order_seg"), ({"kind": 5}, b"seg_kind"), ({"C": 0}, b"C=0"), ({"Cs": 0}, b"Cs=0")):
        assert resample(**kw) == 1 and text in lib.fsg_last_error(), kw
