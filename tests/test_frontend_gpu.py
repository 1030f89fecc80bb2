"""GPU tests of the image front end (csrc/volume.hip) through the C ABI: fields against the fp64 oracle with a bar computed
from the oracle's own fp32 error, keypoints as sets outside a computed ambiguity zone, the reference's quirks, the path from
a volume to class scores, and determinism.

Bars.  A field may differ from the fp64 oracle by at most max(FLOOR, 10 x e_cpu32) in the maximum and in the 99.9th
percentile of the relative error, e_cpu32 being the same statistic of the oracle's fp32 run on the same input.  FLOOR =
16 x 2^-24 ~ 1e-6: a handful of fp32 roundings, for inputs on which the fp32 oracle happens to be exact.  MIND is bounded by
1 and its small values underflow in fp32, so its error is taken relative to max(|value|, 1e-3)."""
import numpy as np
import pytest
import torch

import frontend_oracle as fo
from golden_util import fill_state_dict, load

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -24
AMBIGUOUS_CAP = 0.02


def _check_field(name, got, want64, want32, denom_floor=1e-300):
    g = fo.rel_err(got.cpu(), want64, denom_floor)
    c = fo.rel_err(want32, want64, denom_floor)
    print(f"PARITY {name}: kernel max {g[0]:.3g} p99.9 {g[1]:.3g} | cpu32 max {c[0]:.3g} p99.9 {c[1]:.3g}")
    assert g[2], f"{name}: NaN positions differ from the fp64 oracle"
    assert g[0] <= max(FLOOR, 10 * c[0]) and g[1] <= max(FLOOR, 10 * c[1]), name


def _volumes():
    return [("golden", fo.ct_volume(fo.GOLDEN_SEED)), ("golden_const", fo.ct_volume(fo.GOLDEN_SEED, constant_block=True)),
            ("large", fo.ct_volume(fo.LARGE_SEED, fo.LARGE_SHAPE))]


@pytest.mark.parametrize("sigma", fo.DIST_SIGMAS)
def test_distinctiveness(device, sigma):
    from fissure_segmentation_amd.data_processing.foerstner import distinctiveness
    for name, img in _volumes():
        got = distinctiveness(img.to(device), sigma)
        assert got.shape == img.shape and got.dtype == torch.float32
        _check_field(f"distinctiveness sigma={sigma} {name}", got, fo.distinctiveness(img.double(), sigma), fo.distinctiveness(img, sigma))
    g = load("frontend_foerstner")
    got = distinctiveness(fo.ct_volume(fo.GOLDEN_SEED, constant_block=True).to(device), sigma).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(g[f"dist_const_s{sigma}"])) and np.isnan(got).any()


def test_smooth_and_nms(device):
    from fissure_segmentation_amd.utils.image_utils import nms, smooth
    g = load("frontend_foerstner")
    for name, img in _volumes():
        _check_field(f"smooth {name}", smooth(img.to(device), 0.8), fo.smooth(img.double(), 0.8), fo.smooth(img, 0.8))
    for key in ("dist_s0.5", "dist_const_s0.5"):
        dist = torch.from_numpy(g[key])
        for d in (5, 4, 9, 1):
            got, want = nms(dist.to(device), d).cpu(), fo.nms(dist, d)
            assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(-1), want.nan_to_num(-1)), (key, d)
    assert np.array_equal(nms(torch.from_numpy(g["dist_s0.5"]).to(device), 4).cpu().numpy(), g["nms_d4"])
    big = fo.distinctiveness(fo.ct_volume(fo.LARGE_SEED, fo.LARGE_SHAPE), 0.5)
    assert torch.equal(nms(big.to(device), 5).cpu(), fo.nms(big, 5))


@pytest.mark.parametrize("ssc,dil", fo.MIND_CONFIGS)
def test_mind_and_mind_at_keypoints(device, ssc, dil):
    from fissure_segmentation_amd.data_processing.point_features import mind, mind_at_keypoints
    for name, img in _volumes():
        if name == "golden_const":
            continue
        got = mind(img.to(device), dilation=dil, sigma=0.8, ssc=ssc)
        assert got.shape == (1, 12 if ssc else 6, *img.shape[2:])
        _check_field(f"mind ssc={ssc} dilation={dil} {name}", got, fo.mind(img.double(), dil, 0.8, ssc), fo.mind(img, dil, 0.8, ssc), 1e-3)
        rng = np.random.default_rng(5)
        D, H, W = img.shape[2:]
        kp = torch.from_numpy(np.stack([rng.integers(0, D, 300), rng.integers(0, H, 300), rng.integers(0, W, 300)], 1))
        kp[0], kp[1] = torch.tensor([0, 0, 0]), torch.tensor([D - 1, H - 1, W - 1])
        at = mind_at_keypoints(img.to(device), kp.to(device), dilation=dil, sigma=0.8, ssc=ssc)
        assert at.shape == (got.shape[1], 300)
        assert torch.equal(at, got[0][:, kp[:, 0], kp[:, 1], kp[:, 2]]), "mind_at_keypoints is not mind at the keypoints, bitwise"
    if True:
        want = load(f"frontend_mind_{'ssc' if ssc else 'plain'}_d{dil}")["mind"]
        got = mind(fo.ct_volume(fo.GOLDEN_SEED).to(device), dilation=dil, sigma=0.8, ssc=ssc).cpu().numpy()
        np.testing.assert_allclose(got[:, :, list(fo.MIND_GOLDEN_PLANES)], want, rtol=1e-4, atol=1e-6)   # channel order against the real reference


@pytest.mark.parametrize("sigma,d", fo.KPT_CONFIGS)
def test_keypoints_golden_equal_reference(device, sigma, d):
    from fissure_segmentation_amd.data_processing.foerstner import foerstner_kpts
    g, mask = load("frontend_foerstner"), fo.box_mask()
    for key, img in ((f"kpts_s{sigma}_d{d}", fo.ct_volume(fo.GOLDEN_SEED)),
                     (f"kpts_const_s{sigma}_d{d}", fo.ct_volume(fo.GOLDEN_SEED, constant_block=True))):
        got = foerstner_kpts(img.to(device), mask.to(device), sigma=sigma, d=d)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), g[key]), key


@pytest.mark.parametrize("sigma,d", ((0.5, 5), (1.4, 9)))
def test_keypoints_large_volume_outside_ambiguity_zone(device, sigma, d):
    from fissure_segmentation_amd.data_processing.foerstner import foerstner_kpts
    img, mask = fo.ct_volume(fo.LARGE_SEED, fo.LARGE_SHAPE), fo.box_mask(fo.LARGE_SHAPE)
    d64, d32 = fo.distinctiveness(img.double(), sigma), fo.distinctiveness(img, sigma)
    flags64 = fo.keypoint_flags(d64, mask, d, 1e-8)[0, 0]
    k64 = torch.nonzero(flags64)
    cand = fo.nms(d64, d) == d64
    tau = 10 * float(((d32.double() - d64).abs() / d64.abs())[cand].max())
    ambiguous = (fo.decision_margins(d64, d, 1e-8) <= tau) & fo.erode_mask(mask)[0, 0]
    n_amb = int(ambiguous.sum())
    print(f"PARITY keypoints sigma={sigma} d={d}: {len(k64)} oracle keypoints, tau {tau:.3g}, {n_amb} ambiguous voxels")
    assert n_amb <= AMBIGUOUS_CAP * len(k64), "the seeded input is too ambiguous for this tau: change the input"
    got = foerstner_kpts(img.to(device), mask.to(device), sigma=sigma, d=d).cpu()
    flags = torch.zeros_like(flags64)
    flags[got[:, 0], got[:, 1], got[:, 2]] = True
    assert torch.equal(flags & ~ambiguous, flags64 & ~ambiguous)
    assert torch.equal(got, torch.nonzero(flags)), "not in torch.nonzero's order"


def test_quirks(device):
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.data_processing.foerstner import foerstner_kpts
    # centre-free erosion on a flat field where every voxel is a window maximum
    dist = torch.ones(1, 1, 6, 7, 8)
    mask = torch.ones(1, 1, 6, 7, 8, dtype=torch.bool)
    mask[0, 0, 3, 3, 3] = False          # not in the mask, six mask neighbours: kept; its six neighbours: dropped
    flags = F_hip.nms_keypoint_flags(dist.to(device), mask.to(device), 3, 1e-8).cpu()
    want = fo.keypoint_flags(dist, mask, 3, 1e-8)
    assert torch.equal(flags, want) and bool(flags[0, 0, 3, 3, 3]) and not bool(flags[0, 0, 3, 3, 4]) and not bool(flags[0, 0, 2, 3, 3])
    assert bool(flags[0, 0, 0, 0, 0]) and bool(flags[0, 0, 5, 6, 7])      # border voxels: outside counts as inside the mask
    assert int(flags.sum()) == 6 * 7 * 8 - 6
    # even window: reaches one voxel further forward than backward
    dist = torch.zeros(1, 1, 9, 9, 40)
    dist[0, 0, 4, 4, 20], dist[0, 0, 4, 4, 18], dist[0, 0, 4, 4, 22], dist[0, 0, 4, 4, 35] = 3.0, 2.0, 2.5, 1.0
    for d in (4, 5, 2):
        got = F_hip.nms_keypoint_flags(dist.to(device), None, d, 0.5).cpu()
        assert torch.equal(got, fo.keypoint_flags(dist, torch.ones_like(dist, dtype=torch.bool), d, 0.5)), d
    # d = 4 is the window [i - 1, i + 2]: 18 sees the 3.0 at 20 and is dropped, 22 does not and stays; d = 5 drops both
    assert torch.nonzero(F_hip.nms_keypoint_flags(dist.to(device), None, 4, 0.5))[:, 2:].tolist() == [[4, 4, 20], [4, 4, 22], [4, 4, 35]]
    assert torch.nonzero(F_hip.nms_keypoint_flags(dist.to(device), None, 5, 0.5))[:, 2:].tolist() == [[4, 4, 20], [4, 4, 35]]
    # a NaN suppresses every keypoint whose window holds it, across tile borders too
    img, mask = fo.ct_volume(fo.GOLDEN_SEED, constant_block=True), torch.ones(1, 1, *fo.GOLDEN_SHAPE, dtype=torch.bool)
    d32 = fo.distinctiveness(img, 0.5)
    got = foerstner_kpts(img.to(device), mask.to(device), sigma=0.5, d=5).cpu()
    near_nan = torch.isnan(fo.nms(d32, 5))[0, 0]
    assert near_nan.any() and not near_nan[got[:, 0], got[:, 1], got[:, 2]].any() and len(got) > 10
    spike = torch.rand(1, 1, 12, 12, 40, generator=torch.Generator().manual_seed(1)) + 1
    spike[0, 0, 6, 6, 31] = float("nan")
    got = F_hip.nms_keypoint_flags(spike.to(device), None, 5, 1e-8).cpu()
    assert torch.equal(got, fo.keypoint_flags(spike, torch.ones_like(spike, dtype=torch.bool), 5, 1e-8)) and not got[0, 0, 4:9, 4:9, 29:34].any()


def test_volume_to_class_scores(device):
    from fissure_segmentation_amd.data_processing.keypoint_extraction import foerstner_point_cloud
    from fissure_segmentation_amd.data_processing.point_features import mind
    from fissure_segmentation_amd.models.dgcnn import DGCNNSeg
    from fissure_segmentation_amd.data_processing.foerstner import foerstner_kpts
    from fissure_segmentation_amd.utils.general_utils import kpts_to_grid
    shape = fo.E2E_SHAPE   # the seed is reject-sampled for a keypoint margin of 1e-3: the list equals the oracle's exactly
    img, mask = fo.ct_volume(fo.E2E_SEED, shape), fo.box_mask(shape)
    spacing = (1.5, 1.0, 1.0)
    cloud = foerstner_point_cloud(img.to(device), mask.to(device), spacing=spacing, feature_mode="mind_ssc")
    kp = fo.foerstner_kpts(img.double(), mask, sigma=0.5, d=5)
    K = len(kp)
    assert K > 100 and cloud.shape == (15, K) and cloud.dtype == torch.float32
    assert float(cloud[:3].min()) >= -1 and float(cloud[:3].max()) <= 1
    sp = torch.tensor(spacing)
    want = fo.kpts_to_grid((kp * sp).flip(-1), torch.tensor(shape) * sp).T
    torch.testing.assert_close(cloud[:3].cpu(), want, rtol=1e-6, atol=1e-6)        # the oracle's coordinates, same order
    own = foerstner_kpts(img.to(device), mask.to(device), sigma=0.5, d=5)
    assert torch.equal(own.cpu(), kp)
    assert torch.equal(cloud[:3], kpts_to_grid((own * sp.to(device)).flip(-1), torch.tensor(shape, device=device) * sp.to(device)).T)
    feat = mind(img.to(device))[0][:, own[:, 0], own[:, 1], own[:, 2]]
    assert torch.equal(cloud[3:], feat)
    assert foerstner_point_cloud(img.to(device), mask.to(device), feature_mode=None).shape == (3, K)
    assert foerstner_point_cloud(img.to(device), mask.to(device), feature_mode="mind").shape == (9, K)
    patches = foerstner_point_cloud(img.to(device), mask.to(device), feature_mode="image")
    assert patches.shape == (128, K)
    centre = img[0, 0][kp[:, 0], kp[:, 1], kp[:, 2]]          # the centre voxel of a 5^3 patch, -1000 HU -> -1, 0 HU -> +1
    torch.testing.assert_close(patches[3 + 62].cpu(), (centre + 1000) / 1000 * 2 - 1, rtol=1e-5, atol=1e-5)
    net = fill_state_dict(DGCNNSeg(k=20, in_features=15, num_classes=4), 11).to(device).eval()
    with torch.no_grad():
        scores = net.predict_full_pointcloud(cloud[None], sample_points=128, n_runs_min=10)
    assert tuple(scores.shape) == (1, 4, K) and torch.isfinite(scores).all()
    torch.testing.assert_close(scores.sum(1), torch.ones(1, K, device=device), rtol=1e-5, atol=1e-5)


def test_two_runs_are_bitwise_equal(device):
    from fissure_segmentation_amd.data_processing import foerstner, keypoint_extraction, point_features
    from fissure_segmentation_amd.utils import image_utils
    img, mask = fo.ct_volume(fo.LARGE_SEED + 2, (40, 44, 72)).to(device), fo.box_mask((40, 44, 72)).to(device)
    kp = foerstner.foerstner_kpts(img, mask, 0.5, 5)
    calls = [lambda: foerstner.distinctiveness(img, 0.5), lambda: foerstner.distinctiveness(img, 1.4),
             lambda: foerstner.foerstner_kpts(img, mask, 0.5, 5), lambda: image_utils.nms(img, 4),
             lambda: point_features.mind(img), lambda: point_features.mind(img, 2, 0.8, False),
             lambda: point_features.mind_at_keypoints(img, kp),
             lambda: keypoint_extraction.foerstner_point_cloud(img, mask, feature_mode="mind_ssc")]
    for i, call in enumerate(calls):
        a, b = call(), call()
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), i
