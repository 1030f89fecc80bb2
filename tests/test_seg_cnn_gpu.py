"""Voxel CNN (MobileNetASPP) on the GPU against the fp64 oracle (tests/seg_cnn_oracle.py).  The bar everywhere: the error against
fp64 is at most 4 x the error of the oracle's own fp32 run on the same inputs, at least 4.8e-7 of the output's largest magnitude;
it is computed here, nothing is fixed in advance.  Every figure is printed before it is asserted (profiles/seg_cnn_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import seg_cnn_cases as cases
import seg_cnn_oracle as so
from golden_util import load

pytestmark = pytest.mark.gpu


def _check(what, got, ref64, err32):
    err, bar = float((got.detach().double().cpu() - ref64).abs().max()), cases.bar(err32, ref64)
    print(f"{what}: error {err:.3e}, oracle's fp32 error {err32:.3e}, bar {bar:.3e}, largest magnitude {float(ref64.abs().max()):.3e}")
    assert tuple(got.shape) == tuple(ref64.shape) and err <= bar


@functools.lru_cache(maxsize=None)
def _net(device, patch=(16, 16, 16)):
    from fissure_segmentation_amd.models.seg_cnn import MobileNetASPP
    net = MobileNetASPP(cases.NUM_CLASSES, patch_size=patch)
    net.load_state_dict(cases.state())
    return net.to(device).eval()


# ------------------------------------------------------------------------------------------------ kernel (a)
@pytest.mark.parametrize("name", [c[0] for c in cases.BLOCK_CASES])
def test_block_kernel_against_fp64(device, name):
    from fissure_segmentation_amd import functional as F_hip
    x64, tensors, kw, y64, err32, _ = cases.block_case(name)
    x = x64.float().to(device).contiguous(memory_format=torch.channels_last_3d)
    args = [t.float().to(device) for t in tensors]
    y = F_hip.mbconv3d(x, *args, **kw)
    _check(name, y, y64, err32)
    assert y.permute(0, 2, 3, 4, 1).is_contiguous()                       # channels-last memory
    assert torch.equal(F_hip.mbconv3d(x, *args, **kw), y)                 # the same bits on every run
    assert torch.equal(F_hip.mbconv3d(x64.float().to(device), *args, **kw), y)      # whatever the layout it arrives in
    if x.shape[0] > 1:                                                    # item 0 alone = item 0 inside the batch
        assert torch.equal(F_hip.mbconv3d(x[:1], *args, **kw), y[:1])


# ------------------------------------------------------------------------------------------------ the network
@functools.lru_cache(maxsize=None)
def _forward_case(name, training=False):
    fx = load("seg_cnn_net")
    key = "train" if training else name
    x = so.volume(int(fx[key + "_seed"]), tuple(fx[key + "_shape"]), float(fx["input_scale"]))
    y64 = so.forward(x.double(), cases.state64(), training=training)
    err32 = float((so.forward(x, cases.state(), training=training).double() - y64).abs().max())
    return x, y64, err32, torch.from_numpy(fx[key])


@pytest.mark.parametrize("name", ["fwd16", "fwd8x12x16"])
def test_eval_forward_against_fp64(device, name):
    x, y64, err32, fixture = _forward_case(name)
    net = _net(device)
    with torch.no_grad():
        y = net(x.to(device))
        _check("forward " + name, y, y64, err32)
        assert torch.equal(net(x.to(device)), y)
        if x.shape[0] > 1:
            assert torch.equal(net(x[:1].to(device)), y[:1])
    print(f"forward {name}: against the reference's fp32 fixture {float((y.cpu() - fixture).abs().max()):.3e}")


def test_eval_forward_replays_from_a_graph(device):
    x = _forward_case("fwd16")[0].to(device)
    net = _net(device)
    with torch.no_grad():
        eager = net(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(x)
        torch.cuda.current_stream().wait_stream(side)
        static = x.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(static)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        static.copy_(x.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, net(x.flip(0)))


def test_training_forward_against_fp64(device):
    from fissure_segmentation_amd.models.seg_cnn import MobileNetASPP
    x, y64, err32, fixture = _forward_case("train", training=True)
    net = MobileNetASPP(cases.NUM_CLASSES, patch_size=(16, 16, 16))
    net.load_state_dict(cases.state())
    net = net.to(device).train()
    net.aspp.project[3].p = 0.0            # as in the fixture: the dropout mask of a CPU stream cannot be replayed here
    xg = x.to(device).requires_grad_(True)
    y = net(xg)
    _check("training-mode forward", y, y64, err32)
    print(f"training-mode forward: against the reference's fp32 fixture {float((y.detach().cpu() - fixture).abs().max()):.3e}")
    y.square().mean().backward()           # gradients come from autograd
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    assert all(p.grad is not None for p in net.parameters())


# ------------------------------------------------------------------------------------------------ patch inference
@functools.lru_cache(maxsize=None)
def _patch_case(use_gaussian):
    fx = load("seg_cnn_patch")
    x = so.volume(int(fx["seed"]), tuple(fx["shape"]), float(fx["input_scale"]))
    patch, ov = tuple(int(p) for p in fx["patch"]), float(fx["min_overlap"])
    y64 = so.predict_all_patches(x.double(), cases.state64(), patch, ov, use_gaussian)
    err32 = float((so.predict_all_patches(x, cases.state(), patch, ov, use_gaussian).double() - y64).abs().max())
    return x, patch, ov, y64, err32, torch.from_numpy(fx["gaussian" if use_gaussian else "uniform"])


@pytest.mark.parametrize("use_gaussian", [True, False])
def test_predict_all_patches_against_fp64(device, use_gaussian):
    x, patch, ov, y64, err32, fixture = _patch_case(use_gaussian)
    net = _net(device, patch)
    y = net.predict_all_patches(x.to(device), min_overlap=ov, use_gaussian=use_gaussian)
    what = "predict_all_patches " + ("gaussian" if use_gaussian else "uniform")
    _check(what, y, y64, err32)
    print(f"{what}: against the reference's fp32 fixture {float((y.cpu() - fixture).abs().max()):.3e}")
    assert torch.equal(net.predict_all_patches(x.to(device), min_overlap=ov, use_gaussian=use_gaussian), y)


def test_predict_all_patches_does_not_depend_on_patch_batch(device):
    x = so.volume(41, (1, 1, 24, 16, 16), 3.0).to(device)
    net = _net(device)
    one = net.predict_all_patches(x, patch_batch=1)
    three = net.predict_all_patches(x, patch_batch=3)
    assert tuple(one.shape) == (1, cases.NUM_CLASSES, 24, 16, 16) and torch.equal(one, three)
    two_items = net.predict_all_patches(torch.cat([x, x.flip(2)]), patch_batch=3)       # an item alone = the item in a batch
    assert torch.equal(two_items[:1], one)


def test_patch_kernels_against_fp64(device):
    """kernels (b) alone: random logits, three patches of 8x12x8 on a 10x12x13 volume of two items -- one overhanging with an odd
    padding, two overlapping"""
    from fissure_segmentation_amd import functional as F_hip
    g = torch.Generator().manual_seed(7)
    patch, (D, H, W), K = (8, 12, 8), (10, 12, 13), 3
    logits = 3 * torch.randn((3, K, 4, 6, 4), generator=g)
    entries = [(0, 0, 0, 0), (0, 2, 0, 5), (1, 5, 0, 3)]        # the last: 5 of 8 cells inside, padding 2 in front, 1 behind
    wmap = so.gaussian_map(patch)

    def oracle(dtype):
        out, norm = torch.zeros(2, K, D, H, W, dtype=dtype), torch.zeros(2, 1, D, H, W, dtype=dtype)
        for lg, (b, z, y, x) in zip(logits.to(dtype), entries):
            up = torch.nn.functional.interpolate(lg[None], scale_factor=2, mode="trilinear", align_corners=False)
            prob = torch.softmax(up, dim=1) * wmap.to(dtype)
            n = [min(p, s - o) for p, s, o in zip(patch, (D, H, W), (z, y, x))]
            f = [so.front_back(p - m)[0] for p, m in zip(patch, n)]
            crop = (slice(None), slice(None)) + tuple(slice(a, a + m) for a, m in zip(f, n))
            out[b:b + 1, :, z:z + n[0], y:y + n[1], x:x + n[2]] += prob[crop]
            norm[b:b + 1, :, z:z + n[0], y:y + n[1], x:x + n[2]] += wmap.to(dtype)[None, None][crop]
        return out, norm

    (s64, n64), (s32, n32) = oracle(torch.float64), oracle(torch.float32)
    out_sum, out_w = torch.zeros(2, K, D, H, W, device=device), torch.zeros(2, 1, D, H, W, device=device)
    F_hip.patch_accumulate(logits.to(device), entries, patch, out_sum, out_w, wmap.float().to(device))
    _check("patch_accumulate sum", out_sum, s64, float((s32.double() - s64).abs().max()))
    _check("patch_accumulate weight", out_w, n64, float((n32.double() - n64).abs().max()))
    covered = (n64 > 0).expand_as(s64)
    f64, f32 = torch.softmax(s64 / n64, dim=1), torch.softmax(s32 / n32, dim=1)
    got = F_hip.patch_finalize(out_sum, out_w)
    err = float((got.double().cpu() - f64)[covered].abs().max())
    bar = cases.bar(float((f32.double() - f64)[covered].abs().max()), f64[covered])
    print(f"patch_finalize: error {err:.3e}, bar {bar:.3e}")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ keypoints
def test_cnn_point_cloud_against_fp64(device):
    from fissure_segmentation_amd.data_processing.keypoint_extraction import cnn_point_cloud
    from fissure_segmentation_amd.utils.general_utils import ALIGN_CORNERS, kpts_to_grid, sample_patches_at_kpts
    img, mask, p64, p32 = cases.keypoint_case()
    e = cases.bar(float((p32.double() - p64).abs().max()), p64)
    amb = cases.ambiguous(p64, e) & mask
    net = _net(device, cases.KP_PATCH)
    kp, feat = cnn_point_cloud(net, img.to(device), mask[None, None].to(device), spacing=(1, 1, 1), feat_patch=5)
    assert kp.dtype == torch.int64 and kp.shape[1] == 3 and tuple(feat.shape) == (125, kp.shape[0])
    got = torch.zeros(cases.KP_SHAPE, dtype=torch.bool)
    got[tuple(kp.cpu().t())] = True
    want = so.cnn_keypoint_mask(p64, mask)
    print(f"cnn_point_cloud: {kp.shape[0]} keypoints, oracle {int(want.sum())}, differing {int((got != want).sum())}, "
          f"ambiguous {int(amb.sum())} of {int(mask.sum())} masked voxels (error bar {e:.3e})")
    assert int(amb.sum()) <= 0.01 * int(mask.sum())
    assert not bool(((got != want) & ~amb).any())
    assert torch.equal(kp.cpu(), torch.nonzero(got))            # in scan order, as torch.nonzero lists them
    # the features: 5^3 patches of the summed foreground scores around every keypoint
    grid = kpts_to_grid(kp.cpu().float().flip(-1), torch.tensor(cases.KP_SHAPE).float(), align_corners=ALIGN_CORNERS)
    want_feat = sample_patches_at_kpts(p64[:, 1:].sum(1, keepdim=True).float(), grid, 5).reshape(kp.shape[0], -1).t()
    ferr = float((feat.cpu() - want_feat).abs().max())
    print(f"cnn_point_cloud: features differ by {ferr:.3e} (two scores each within {e:.3e}, read in fp32)")
    assert ferr <= 2 * e + 2 * 6e-8
    # several fold models: two lists; a spacing scales the coordinates
    kps, feats = cnn_point_cloud([net, net], img.to(device), mask.to(device), spacing=(2, 1, 1))
    assert len(kps) == len(feats) == 2 and torch.equal(kps[0], kps[1]) and torch.equal(feats[0], feats[1])
    assert torch.equal(kps[0], kp * torch.tensor([2, 1, 1], device=kp.device))
