"""CPU tests of the Hessian fissure enhancement: the oracle (tests/hessian_oracle.py) against what the real reference
returned (tests/golden/hessian_enhance.npz), the tap helpers, the selection rule, argument validation and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy.ndimage._filters import _gaussian_kernel1d

import hessian_oracle as ho
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fsg_fissure_enhance_f32", "fsg_smooth_threshold_f32")


def test_oracle_fp32_equals_reference():
    g = load("hessian_enhance")
    assert float(g["mu"]) == ho.MU and float(g["sigma_hu"]) == ho.SIGMA_HU
    Fv, P, hw = ho.enhance(ho.volume("golden")[0])
    for name, got, want in (("F", Fv, g["F_plain"]), ("P", P, g["P_plain"]), ("hu", hw, g["hu_plain"]),
                            ("F block", ho.enhance(ho.volume("golden", ho.BLOCK_VALUE)[0])[0], g["F_block"])):
        diff = float(np.abs(got.numpy() - want).max())
        print(f"PARITY oracle32 vs reference {name}: max abs {diff:.3g}")
        assert got.shape == want.shape and diff <= 1e-6, name
    assert 0.01 < float((g["F_plain"] > ho.THRESHOLD).mean()) < 0.9   # the fixture exercises both sides of the threshold


def test_tap_helpers():
    from fissure_segmentation_amd import functional as F_hip
    for sigma in (1.0, 0.5, 0.8):
        for order in (0, 1, 2):
            want = torch.from_numpy(_gaussian_kernel1d(sigma, order, int(4.0 * sigma + 0.5))).float()
            assert torch.equal(F_hip.gaussian_derivative_taps(sigma, order), want), (sigma, order)
            assert torch.equal(ho.derivative_taps(sigma, order), want)
    k1, k2 = F_hip.gaussian_derivative_taps(1.0, 1), F_hip.gaussian_derivative_taps(1.0, 2)
    assert k1.numel() == 9 and torch.equal(k1, -k1.flip(0)) and torch.equal(k2, k2.flip(0))   # what the kernel requires
    tz, ty, tx = F_hip.discrete_gaussian_taps(1.0)
    for t in (tz, ty, tx, ho.discrete_gaussian_taps(1.0)):
        assert t.dtype == torch.float32 and t.numel() == 7
        np.testing.assert_allclose(t.numpy(), ho.DISCRETE_GAUSSIAN_VAR1, rtol=0, atol=1e-6)
    assert torch.equal(tz, ho.discrete_gaussian_taps(1.0)) and abs(float(tz.double().sum()) - 1) < 1e-6
    tz, ty, tx = F_hip.discrete_gaussian_taps(1.0, spacing=(2.0, 1.0, 1.25))   # physical variance 1 -> voxel variances 1/4, 1, 0.64
    assert torch.equal(tz, ho.discrete_gaussian_taps(0.25)) and torch.equal(ty, ho.discrete_gaussian_taps(1.0))
    assert torch.equal(tx, ho.discrete_gaussian_taps(0.64)) and tz.numel() < ty.numel()
    assert F_hip.discrete_gaussian_taps((0.0, 1.0, 1.0))[0].tolist() == [1.0]


def test_selection_order_and_ties():
    """the package's selection (plain torch over the compacted candidates, any device) on a hand-made volume"""
    from fissure_segmentation_amd.data_processing.keypoint_extraction import select_candidates
    v = torch.zeros(3, 4, 5)
    v[2, 3, 4] = 0.9
    v[0, 1, 2] = v[1, 0, 0] = v[0, 0, 3] = 0.5                        # a tie: linear index ascending
    v[1, 1, 1] = 0.7
    v[2, 0, 0] = 0.2                                                  # not ABOVE the threshold
    v[0, 0, 0] = 0.1
    flags = v > 0.2
    assert select_candidates(v, flags, 20000).tolist() == [[2, 3, 4], [1, 1, 1], [0, 0, 3], [0, 1, 2], [1, 0, 0]]
    assert select_candidates(v, flags, 3).tolist() == [[2, 3, 4], [1, 1, 1], [0, 0, 3]]      # K cuts inside the tie
    assert select_candidates(v, flags, 4).tolist() == [[2, 3, 4], [1, 1, 1], [0, 0, 3], [0, 1, 2]]
    assert select_candidates(v, v > 0.95, 3).shape == (0, 3) and select_candidates(v, flags, 3).dtype == torch.int64
    for K in (20000, 4, 3, 1):                                        # the oracle's dense sort states the same rule
        assert torch.equal(select_candidates(v, flags, K), ho.select(v[None, None], 0.2, K)), K


def test_new_symbols_exported_and_bound():
    from fissure_segmentation_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    declared = set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name


def test_library_validates_before_it_launches():
    """the entry points check the host-side arguments first and the device pointers last, so with NULL volumes every argument
    error below is reported and a lost check ends in the NULL error, never in a launch"""
    from fissure_segmentation_amd import _lib
    f9 = (ctypes.c_float * 9)

    def enhance(k1, k2, n, shape=(1, 8, 8, 8), sigma_hu=250.0):
        return _lib.call("fsg_fissure_enhance_f32", None, None, *shape, k1, k2, n, -400.0, sigma_hu, None, None, None, None)
    k1 = f9(*[float(v) for v in ho.derivative_taps(1.0, 1)])
    k2 = f9(*[float(v) for v in ho.derivative_taps(1.0, 2)])
    wide = (ctypes.c_float * 11)(*([0.0] * 11))
    for args, word in (((wide, wide, 11), "derivative taps"), ((k1, k2, 4), "derivative taps"),
                       ((k2, k2, 9), "first-derivative taps must be antisymmetric"),
                       ((k1, k1, 9), "second-derivative taps must be symmetric"), ((k1, k2, 9, (1, 0, 8, 8)), "bad shape"),
                       ((k1, k2, 9, (1, 8, 8, 8), 0.0), "sigma_hu"), ((None, k2, 9), "NULL tap pointer"),
                       ((k1, k2, 9), "NULL pointer")):
        with pytest.raises(RuntimeError, match=word):
            enhance(*args)
    w7 = (ctypes.c_float * 7)(*[float(v) for v in ho.discrete_gaussian_taps(1.0)])

    def smooth(*taps, shape=(1, 8, 8, 8)):
        return _lib.call("fsg_smooth_threshold_f32", None, *shape, *taps, 0.2, None, None, None)
    for args, word in (((w7, 7, wide, 11, w7, 7), "smoothing taps"), ((w7, 7, w7, 6, w7, 7), "smoothing taps"),
                       ((w7, 7, None, 7, w7, 7), "NULL tap pointer"), ((w7, 7, w7, 7, w7, 7), "NULL pointer")):
        with pytest.raises(RuntimeError, match=word):
            smooth(*args)
    with pytest.raises(RuntimeError, match="bad shape"):
        smooth(w7, 7, w7, 7, w7, 7, shape=(1, 8, -1, 8))


def test_python_layer_validates():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.data_processing import fissure_enhancement as fe
    from fissure_segmentation_amd.data_processing import keypoint_extraction as ke
    img, mask = ho.volume("golden")
    with pytest.raises(ValueError, match="sigma"):
        fe.HessianEnhancementFilter(ho.MU, ho.SIGMA_HU, gaussian_derivation_sigma=1.5)        # radius 6
    with pytest.raises(ValueError, match="sigma"):
        F_hip.fissure_enhance(img, ho.MU, ho.SIGMA_HU, derivation_sigma=0.1)                    # radius 0
    with pytest.raises(ValueError, match="positive"):
        F_hip.fissure_enhance(img, ho.MU, 0.0)
    with pytest.raises(ValueError, match="taps"):
        F_hip.smooth_threshold(img, [torch.ones(11) / 11] * 3, 0.2)
    with pytest.raises(ValueError, match="taps"):
        F_hip.smooth_threshold(img, [torch.ones(4) / 4] * 3, 0.2)
    with pytest.raises(ValueError, match="three"):
        F_hip.smooth_threshold(img, [torch.ones(3) / 3] * 2, 0.2)
    with pytest.raises(ValueError, match="feature_mode"):
        ke.enhancement_point_cloud(img, mask, ho.MU, ho.SIGMA_HU, feature_mode="cnn")
    filt = fe.HessianEnhancementFilter(ho.MU, ho.SIGMA_HU)
    for call in (lambda: filt(img), lambda: fe.get_enhanced_fissure_image(img, mask, ho.MU, ho.SIGMA_HU),
                 lambda: fe.hessian_based_enhancement_torch(img, ho.MU, ho.SIGMA_HU),
                 lambda: ke.hessian_enhancement_kpts(img), lambda: ke.enhancement_point_cloud(img, mask, ho.MU, ho.SIGMA_HU)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    assert ke.FEATURE_MODES == (None, 'mind', 'mind_ssc', 'image') and ke.ENHANCEMENT_FEATURE_MODES[-1] == 'enhancement'


def test_plain_torch_helpers_match_oracle():
    from fissure_segmentation_amd.data_processing import fissure_enhancement as fe
    img, _ = ho.volume("golden")
    H = fe.hessian_matrix(img, 1.0)
    assert torch.equal(H, ho.hessian(img, 1.0))
    ev = torch.linalg.eigvalsh(H)
    ev = torch.gather(ev, -1, torch.argsort(ev.abs(), dim=-1, descending=True))
    got = fe.fissure_filter(img[0, 0], ev[..., 0], ev[..., 1], ho.MU, ho.SIGMA_HU, return_intermediate=True)
    for a, b in zip(got, ho.enhance(img)):
        assert torch.equal(a, b)


def test_reference_import_name_resolves_to_the_package():
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from data_processing.fissure_enhancement import HessianEnhancementFilter, fissure_filter, hessian_matrix  # noqa: F401
        from data_processing.keypoint_extraction import enhancement_point_cloud, hessian_enhancement_kpts  # noqa: F401
        assert HessianEnhancementFilter.__module__.startswith("fissure_segmentation_amd.")
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
