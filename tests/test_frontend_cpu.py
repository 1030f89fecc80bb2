"""CPU tests of the image front end: the oracle (tests/frontend_oracle.py, fp32) against what the real reference returned
(tests/golden/frontend_*.npz), the plain-torch helpers of the package against the same, the pair table of MIND-SSC, and the
host-side contract (symbols, CPU tensors refused, reference import names)."""
import os
import re

import numpy as np
import pytest
import torch

import frontend_oracle as fo
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5
NEW_SYMBOLS = ("fsg_foerstner_dist_f32", "fsg_nms_keypoints", "fsg_mind_stats_workspace_bytes", "fsg_mind_stats_f32",
               "fsg_mind_eval_f32", "fsg_mind_eval_kp_f32")


def _close(got, want, rtol=RTOL, atol=0.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=atol)


def _inputs():
    g = load("frontend_foerstner")
    assert int(g["seed"]) == fo.GOLDEN_SEED and tuple(g["shape"]) == fo.GOLDEN_SHAPE
    return g, fo.ct_volume(fo.GOLDEN_SEED), fo.ct_volume(fo.GOLDEN_SEED, constant_block=True), fo.box_mask()


@pytest.mark.parametrize("sigma", fo.DIST_SIGMAS)
def test_oracle_distinctiveness_matches_reference(sigma):
    g, img, img_const, _ = _inputs()
    for key, vol in ((f"dist_s{sigma}", img), (f"dist_const_s{sigma}", img_const)):
        mx, p999, same_nan = fo.rel_err(fo.distinctiveness(vol, sigma), torch.from_numpy(g[key]))
        print(f"PARITY oracle32 vs reference {key}: max {mx:.3g} p99.9 {p999:.3g}")
        assert same_nan and mx <= RTOL
    assert np.isnan(g[f"dist_const_s{sigma}"]).any() and not np.isnan(g[f"dist_s{sigma}"]).any()


@pytest.mark.parametrize("sigma,d", fo.KPT_CONFIGS)
def test_oracle_keypoints_equal_reference(sigma, d):
    g, img, img_const, mask = _inputs()
    for key, vol in ((f"kpts_s{sigma}_d{d}", img), (f"kpts_const_s{sigma}_d{d}", img_const)):
        got = fo.foerstner_kpts(vol, mask, sigma=sigma, d=d)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), g[key]), key
        assert len(g[key]) > 5


def test_oracle_smooth_and_nms_match_reference():
    g, img, _, _ = _inputs()
    _close(fo.smooth(img, 0.8).numpy(), g["smooth_s0.8"])
    dist = torch.from_numpy(g["dist_s0.5"])
    for d in (5, 4):
        assert np.array_equal(fo.nms(dist, d).numpy(), g[f"nms_d{d}"])


@pytest.mark.parametrize("ssc,dil", fo.MIND_CONFIGS)
def test_oracle_mind_matches_reference(ssc, dil):
    g = load(f"frontend_mind_{'ssc' if ssc else 'plain'}_d{dil}")
    got = fo.mind(fo.ct_volume(fo.GOLDEN_SEED), dilation=dil, sigma=0.8, ssc=ssc).numpy()
    assert got.shape == (1, 12 if ssc else 6, *fo.GOLDEN_SHAPE)
    assert tuple(g["planes"]) == fo.MIND_GOLDEN_PLANES
    _close(got[:, :, list(fo.MIND_GOLDEN_PLANES)], g["mind"], rtol=RTOL, atol=1e-7)   # values in [0, 1]; the smallest ones underflow


def test_ssc_table_and_permutation_match_golden_channel_order():
    """the package derives its pair table from the six-neighbourhood; each output channel, recomputed on its own from the
    pair the table assigns to it, must be the reference's channel at that position"""
    from fissure_segmentation_amd.data_processing.point_features import SSC_ORDER, mind_shift_tables
    shifts, outch, box = mind_shift_tables(True)
    assert len(shifts) == 12 and sorted(outch) == list(range(12)) and not box
    assert [tuple(tuple(v + 1 for v in p) for p in pair) for pair in shifts] == [tuple(pq) for pq in fo.ssc_pairs()]
    assert tuple(SSC_ORDER) == fo.SSC_PERMUTATION and [outch[c] for c in SSC_ORDER] == list(range(12))
    for a, b in shifts:
        assert sum((x - y) ** 2 for x, y in zip(a, b)) == 2 and sum(abs(x) for x in a) == 1 and sum(abs(x) for x in b) == 1
    img = fo.ct_volume(fo.GOLDEN_SEED)
    p = torch.nn.functional.pad(img, (1,) * 6, mode="replicate")[0, 0]
    D, H, W = fo.GOLDEN_SHAPE

    def at(s):
        return p[1 + s[0]: 1 + s[0] + D, 1 + s[1]: 1 + s[1] + H, 1 + s[2]: 1 + s[2] + W]
    ssd = torch.stack([fo.smooth(((at(a) - at(b)) ** 2)[None, None], 0.8)[0, 0] for a, b in shifts])
    ssd = ssd - ssd.min(0).values
    var = ssd.mean(0)
    var = var.clamp(var.mean() * 0.001, var.mean() * 1000)
    want, planes = load("frontend_mind_ssc_d1")["mind"][0], list(fo.MIND_GOLDEN_PLANES)
    for c in range(12):
        _close(torch.exp(-ssd[c] / var).numpy()[planes], want[outch[c]], rtol=1e-4, atol=1e-6)
    plain, order, box = mind_shift_tables(False)
    assert box and order == list(range(6)) and all(a == 2 ** 27 - 1 for a, _ in plain)
    assert [b for _, b in plain] == [0b111 << 12, (0b111 << 3) | (0b111 << 9) | (0b111 << 15) | (0b111 << 21), 0b111 << 12, 0, 0, 0]


def test_package_torch_helpers_match_reference():
    from fissure_segmentation_amd.data_processing.foerstner import invert_structure_tensor_only_trace, structure_tensor
    from fissure_segmentation_amd.data_processing.point_features import image_patch_features
    from fissure_segmentation_amd.utils import general_utils as gu
    from fissure_segmentation_amd.utils import image_utils as iu
    g, img, _, _ = _inputs()
    gp = load("frontend_points")
    _close(iu.smooth(img, 0.8).numpy(), g["smooth_s0.8"])
    filt = torch.tensor([1.0 / 12.0, -8.0 / 12.0, 0.0, 8.0 / 12.0, -1.0 / 12.0])
    for key, vol, sigma in (("dist_s1.4", img, 1.4), ("dist_s0.5", img, 0.5), ("dist_const_s0.5", fo.ct_volume(fo.GOLDEN_SEED, constant_block=True), 0.5)):
        grad = torch.cat([iu.filter_1d(vol, filt, k) for k in range(3)], dim=1)
        dist = 1. / invert_structure_tensor_only_trace(structure_tensor(grad, sigma)).sum(dim=1, keepdim=True)
        mx, _, same_nan = fo.rel_err(dist, torch.from_numpy(g[key]))
        assert same_nan and mx <= RTOL, (key, mx)
    pts, shape = fo.patch_points(fo.GOLDEN_SEED + 1, 40), torch.tensor(fo.GOLDEN_SHAPE)
    assert gu.ALIGN_CORNERS is False
    grid = gu.kpts_to_grid(pts, shape, align_corners=gu.ALIGN_CORNERS)
    np.testing.assert_allclose(grid.numpy(), gp["grid"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(fo.kpts_to_grid(pts, shape).numpy(), gp["grid"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gu.kpts_to_world(grid, shape, align_corners=gu.ALIGN_CORNERS).numpy(), gp["world"], rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(fo.kpts_to_world(grid, shape).numpy(), gp["world"], rtol=1e-6, atol=1e-5)
    assert grid.min() >= -1 and grid.max() <= 1
    for ps in fo.PATCH_SIZES:
        got = gu.sample_patches_at_kpts(img, grid, ps)
        assert got.shape == (1, 40, ps, ps, ps)
        np.testing.assert_allclose(got.numpy(), gp[f"patches_p{ps}"], rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(fo.sample_patches_at_kpts(img, grid, ps).numpy(), gp[f"patches_p{ps}"], rtol=1e-5, atol=1e-3)
    feat = image_patch_features(img, grid, 5)
    assert feat.shape == (125, 40) and torch.equal(feat[:, 3], gu.sample_patches_at_kpts(img, grid, 5)[0, 3].flatten())
    with pytest.raises(NotImplementedError):
        gu.kpts_to_grid(pts, shape, return_transform=True)
    with pytest.raises(ValueError):
        gu.sample_patches_at_kpts(img, grid * 3, 5)


def test_new_symbols_exported_and_bound():
    from fissure_segmentation_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    declared = set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    ws = _lib.lib.fsg_mind_stats_workspace_bytes
    assert ws(0, 8, 8, 8) == 0 and ws(1, 8, 8, 32) == 4 and ws(2, 9, 8, 33) == 2 * 2 * 1 * 2 * 4
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_foerstner_dist_f32", None, 1, 8, 8, 8, None, 3, None, None)
    with pytest.raises(RuntimeError, match="window"):
        _lib.call("fsg_nms_keypoints", 1, None, 1, 8, 8, 8, 99, 0.0, 1, None, None)


def test_cpu_tensors_are_refused():
    from fissure_segmentation_amd.data_processing import foerstner, keypoint_extraction, point_features
    from fissure_segmentation_amd.utils import image_utils
    img, mask = fo.ct_volume(1, (8, 8, 8)), torch.ones(1, 1, 8, 8, 8, dtype=torch.bool)
    kp = torch.zeros(2, 3, dtype=torch.int64)
    for call in (lambda: foerstner.distinctiveness(img, 0.5), lambda: foerstner.foerstner_kpts(img, mask),
                 lambda: image_utils.nms(img, 5), lambda: point_features.mind(img),
                 lambda: point_features.mind_at_keypoints(img, kp),
                 lambda: keypoint_extraction.foerstner_point_cloud(img, mask)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    assert keypoint_extraction.MAX_KPTS == 20000
    kp2, perm = keypoint_extraction.limit_keypoints(torch.arange(30).view(10, 3), 4)
    assert kp2.shape == (4, 3) and len(perm) == 4
    kp3, perm = keypoint_extraction.limit_keypoints(kp)
    assert kp3 is kp and perm.tolist() == [0, 1]


def test_reference_import_names_resolve_to_the_package():
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from data_processing.foerstner import foerstner_kpts
        from data_processing.keypoint_extraction import foerstner_point_cloud
        from data_processing.point_features import mind
        from utils.general_utils import kpts_to_grid
        from utils.image_utils import smooth
        for fn in (foerstner_kpts, foerstner_point_cloud, mind, kpts_to_grid, smooth):
            assert fn.__module__.startswith("fissure_segmentation_amd."), fn
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
