"""Voxel CNN (MobileNetASPP), the part that needs no GPU: the fp64 oracle against the real reference's fixtures, the helpers and
the Gaussian map, key / shape parity and the checkpoint round trip, the bindings, every host-side refusal, and that the inputs of
the kernel tests make both ReLU6 clamps count."""
import json
import os
import re

import numpy as np
import pytest
import torch

import seg_cnn_cases as cases
import seg_cnn_oracle as so
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net_fx():
    return load("seg_cnn_net")


@pytest.fixture(scope="module")
def patch_fx():
    return load("seg_cnn_patch")


def _assert_fixture(got64, got32, want, what):
    """the fixture is the reference's fp32 run: it may sit as far from the fp64 oracle as 4 x the oracle's own fp32 run does"""
    want = torch.from_numpy(np.asarray(want)).double()
    err = float((want - got64).abs().max())
    bar = cases.bar(float((got32.double() - got64).abs().max()), got64)
    print(f"{what}: fixture vs fp64 oracle {err:.3e}, bar {bar:.3e}, largest magnitude {float(got64.abs().max()):.3e}")
    assert want.shape == got64.shape and err <= bar


@pytest.mark.parametrize("name", ["fwd16", "fwd8x12x16"])
def test_oracle_forward_equals_reference(net_fx, name):
    assert int(net_fx["weight_seed"]) == cases.WEIGHT_SEED and int(net_fx["num_classes"]) == cases.NUM_CLASSES
    x = so.volume(int(net_fx[name + "_seed"]), tuple(net_fx[name + "_shape"]), float(net_fx["input_scale"]))
    _assert_fixture(so.forward(x.double(), cases.state64()), so.forward(x, cases.state()), net_fx[name], name)


def test_oracle_training_forward_equals_reference(net_fx):
    x = so.volume(int(net_fx["train_seed"]), tuple(net_fx["train_shape"]), float(net_fx["input_scale"]))
    _assert_fixture(so.forward(x.double(), cases.state64(), training=True), so.forward(x, cases.state(), training=True),
                    net_fx["train"], "training-mode forward")


@pytest.mark.parametrize("key, use_gaussian", [("gaussian", True), ("uniform", False)])
def test_oracle_patch_loop_equals_reference(patch_fx, key, use_gaussian):
    x = so.volume(int(patch_fx["seed"]), tuple(patch_fx["shape"]), float(patch_fx["input_scale"]))
    patch, ov = tuple(int(p) for p in patch_fx["patch"]), float(patch_fx["min_overlap"])
    _assert_fixture(so.predict_all_patches(x.double(), cases.state64(), patch, ov, use_gaussian),
                    so.predict_all_patches(x, cases.state(), patch, ov, use_gaussian), patch_fx[key], "predict_all_patches " + key)


def test_helpers_equal_reference(net_fx):
    from fissure_segmentation_amd.models import seg_cnn
    helpers = json.loads(str(net_fx["helpers_json"]))
    assert len(helpers["patch_starts"]) >= 5 and any(min(c["size"]) < min(c["patch"]) for c in helpers["patch_starts"])
    for c in helpers["patch_starts"]:
        assert seg_cnn.get_patch_starts(c["size"], c["min_overlap"], c["patch"]) == c["starts"], c
        assert so.patch_starts(c["size"], c["min_overlap"], c["patch"]) == c["starts"], c
    for c in helpers["padding"]:
        assert seg_cnn.get_necessary_padding(c["size"], c["patch"]) == c["pad"], c
        assert list(seg_cnn.maybe_pad_img_patch(torch.zeros(1, 1, *c["size"]), c["patch"]).shape[2:]) == c["padded"]
    assert any(p and any(a != b for a, b in zip(p[::2], p[1::2])) for p in (c["pad"] for c in helpers["padding"]))   # an odd split
    x = torch.arange(11 * 13 * 16, dtype=torch.float32).view(1, 1, 11, 13, 16)
    padded = seg_cnn.maybe_pad_img_patch(x, (16, 16, 16))
    assert np.array_equal(padded[0, 0].numpy(), net_fx["padded_11x13x16"])
    assert torch.equal(seg_cnn.maybe_crop_after_padding(padded, (11, 13, 16)), x)
    assert seg_cnn.maybe_crop_after_padding(x, (11, 13, 16)) is x and seg_cnn.maybe_pad_img_patch(x, (8, 13, 16)) is x


@pytest.mark.parametrize("patch", [(9, 8, 12), (16, 16, 16)])
def test_gaussian_map_equals_reference_and_scipy(net_fx, patch):
    from scipy.ndimage import gaussian_filter
    from fissure_segmentation_amd.models.seg_cnn import gaussian_weight_map
    got = gaussian_weight_map(patch)
    assert got.dtype == torch.float64 and tuple(got.shape) == patch and float(got.min()) > 0
    impulse = np.zeros(patch)
    impulse[tuple(p // 2 for p in patch)] = 1
    want = gaussian_filter(impulse, sigma=[p / 4. for p in patch], order=0, mode="constant", cval=0)
    want[want == 0] = want[want != 0].min()
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got.numpy(), net_fx["gauss_" + "x".join(map(str, patch))], rtol=1e-13, atol=0)
    np.testing.assert_allclose(so.gaussian_map(patch).numpy(), want, rtol=1e-13, atol=0)


def test_state_dict_keys_and_shapes_equal_reference(net_fx):
    from fissure_segmentation_amd.models.seg_cnn import MobileNetASPP
    keys = [str(k) for k in net_fx["keys"]]
    shapes = [tuple(json.loads(str(s))) for s in net_fx["shapes"]]
    assert len(keys) == 200
    sd = MobileNetASPP(cases.NUM_CLASSES, patch_size=(16, 16, 16)).state_dict()
    assert list(sd.keys()) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    assert list(so.state_shapes(cases.NUM_CLASSES).items()) == list(zip(keys, shapes))


def test_reference_checkpoint_round_trip(tmp_path):
    from fissure_segmentation_amd.models.seg_cnn import MobileNetASPP
    path = str(tmp_path / "model.pth")
    # what the reference's LoadableModel.save writes
    torch.save({"config": {"num_classes": cases.NUM_CLASSES, "patch_size": (16, 16, 16)}, "model_state": dict(cases.state())}, path)
    net = MobileNetASPP.load(path, "cpu")
    assert net.config == {"num_classes": cases.NUM_CLASSES, "patch_size": (16, 16, 16)} and tuple(net.patch_size) == (16, 16, 16)
    sd = net.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in cases.state().items()) and len(sd) == 200
    net.save(path)
    again = MobileNetASPP.load(path, "cpu")
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), sd.values()))
    assert MobileNetASPP(2).config == {"num_classes": 2, "patch_size": (128, 128, 128)}


def test_fold_is_invalidated_by_train_and_load_state_dict():
    from fissure_segmentation_amd.models.seg_cnn import MobileNetASPP
    net = MobileNetASPP(cases.NUM_CLASSES, patch_size=(16, 16, 16)).eval()
    net.load_state_dict(cases.state())
    first = net.folded()
    assert net.folded() is first                      # kept between calls
    scale, shift = first["backbone"][1][0][1:3]       # block 1, first BatchNorm
    s64, b64 = so.fold(cases.state64(), "backbone.layers.2.1")
    torch.testing.assert_close(scale.double(), s64, rtol=1e-6, atol=0)
    torch.testing.assert_close(shift.double(), b64, rtol=1e-5, atol=1e-7)
    net.train()
    assert net._folded is None
    net.eval()
    second = net.folded()
    assert second is not first
    net.load_state_dict(cases.state())
    assert net._folded is None


def test_symbols_declared_exported_and_bound():
    from fissure_segmentation_amd import _lib, functional
    header = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    for name in ("fsg_mbconv3d_fwd_f32", "fsg_patch_accumulate_f32", "fsg_patch_finalize_f32"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][0]
    for name in ("mbconv3d", "patch_accumulate", "patch_finalize"):
        assert callable(getattr(functional, name))
    assert "seg_cnn.hip" in open(os.path.join(ROOT, "fissure-segmentation_amd", "csrc", "Makefile")).read()
    from fissure_segmentation_amd.data_processing.keypoint_extraction import cnn_point_cloud
    assert callable(cnn_point_cloud)
    import fissure_segmentation_amd as fsg
    import sys
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        for alias in ("models.seg_cnn", "models.mobilenet", "models.aspp_3d"):
            assert sys.modules[alias].__name__ == "fissure_segmentation_amd." + alias
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)


def _block_tensors(cin=16, cmid=96, cout=24, first=False):
    z = torch.zeros
    return (z(2, cin, 4, 4, 4), z(cmid, 27 if first else cin), z(cmid), z(cmid), z(cmid, 27), z(cmid), z(cmid), z(cout, cmid), z(cout), z(cout))


def test_functional_refuses_on_the_host():
    from fissure_segmentation_amd import functional as F_hip
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.mbconv3d(*_block_tensors())
    for kw, match in ((dict(cin=65), "limits"), (dict(cout=65), "limits"), (dict(cmid=400), "limits"), (dict(cmid=100), "limits")):
        with pytest.raises(ValueError, match=match):
            F_hip.mbconv3d(*_block_tensors(**kw))
    with pytest.raises(ValueError, match="stride"):
        F_hip.mbconv3d(*_block_tensors(), stride=3)
    with pytest.raises(ValueError, match="one input channel"):
        F_hip.mbconv3d(*_block_tensors(cin=2, first=True), first=True)
    with pytest.raises(ValueError, match="residual"):
        F_hip.mbconv3d(*_block_tensors(), residual=True)
    with pytest.raises(ValueError, match="do not fit"):
        F_hip.mbconv3d(*_block_tensors()[:7], torch.zeros(24, 95), torch.zeros(24), torch.zeros(24))
    out_sum, out_w = torch.zeros(1, 3, 10, 10, 10), torch.zeros(1, 1, 10, 10, 10)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.patch_accumulate(torch.zeros(1, 3, 4, 4, 4), [(0, 0, 0, 0)], (8, 8, 8), out_sum, out_w)
    with pytest.raises(ValueError, match="half-resolution"):
        F_hip.patch_accumulate(torch.zeros(1, 3, 4, 4, 5), [(0, 0, 0, 0)], (8, 8, 8), out_sum, out_w)
    with pytest.raises(ValueError, match="one start per patch"):
        F_hip.patch_accumulate(torch.zeros(2, 3, 4, 4, 4), [(0, 0, 0, 0)], (8, 8, 8), out_sum, out_w)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.patch_finalize(out_sum, out_w)


def test_library_refuses_bad_arguments_before_any_launch():
    from fissure_segmentation_amd import _lib
    p = [16] * 10           # non-NULL stand-ins: nothing is dereferenced on the host before the checks

    def mb(B=1, Cin=16, Cmid=96, Cout=24, D=4, H=4, W=4, stride=1, first=0, residual=0, x=16, y=32):
        _lib.call("fsg_mbconv3d_fwd_f32", x, *p[1:], B, Cin, Cmid, Cout, D, H, W, stride, first, residual, y, None)

    for kw, match in ((dict(x=None), "NULL pointer"), (dict(y=16), "must differ"), (dict(D=0), ">= 1"), (dict(Cin=65), "Cin=65"),
                      (dict(Cin=0), "Cin=0"), (dict(Cmid=400), "Cmid=400"), (dict(Cmid=100), "Cmid=100"), (dict(Cout=65), "Cout=65"),
                      (dict(stride=3), "stride=3"), (dict(first=1), "one input channel"), (dict(residual=1), "residual"),
                      (dict(Cout=16, stride=2, residual=1), "residual"), (dict(D=2048, H=2048, W=512), "2\\^31")):
        with pytest.raises(RuntimeError, match=match):
            mb(**kw)
    starts = (_lib.ctypes.c_int * 4)(0, 0, 0, 0)

    def acc(P=1, K=3, pd=8, ph=8, pw=8, st=starts, B=1, D=10, H=10, W=10, logits=16):
        _lib.call("fsg_patch_accumulate_f32", logits, P, K, pd, ph, pw, st, None, 16, 32, B, D, H, W, None)

    for kw, match in ((dict(logits=None), "NULL pointer"), (dict(pd=7), "even"), (dict(K=0), "bad shape"),
                      (dict(st=(_lib.ctypes.c_int * 4)(1, 0, 0, 0)), "outside the volume"),
                      (dict(st=(_lib.ctypes.c_int * 4)(0, 0, 10, 0)), "outside the volume")):
        with pytest.raises(RuntimeError, match=match):
            acc(**kw)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_patch_finalize_f32", 16, None, 1, 3, 4, 4, 4, 16, None)
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("fsg_patch_finalize_f32", 16, 16, 1, 0, 4, 4, 4, 16, None)


def test_modules_refuse_on_the_host():
    from fissure_segmentation_amd.models.seg_cnn import MobileNetASPP
    from fissure_segmentation_amd.data_processing.keypoint_extraction import cnn_point_cloud
    net = MobileNetASPP(cases.NUM_CLASSES, patch_size=(16, 16, 16)).eval()
    for shape in ((1, 1, 16, 16, 18), (1, 1, 6, 16, 16), (1, 1, 16, 15, 16)):
        with pytest.raises(ValueError, match="multiple of 4"):
            net(torch.zeros(shape))
    with pytest.raises(ValueError, match=r"\(B, 1, D, H, W\)"):
        net(torch.zeros(1, 2, 16, 16, 16))
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(RuntimeError, match="GPU only"):
        net.train()(torch.zeros(2, 1, 16, 16, 16))
    with pytest.raises(RuntimeError, match="eval"):
        net.predict_all_patches(torch.zeros(1, 1, 10, 20, 19))
    net.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        net.predict_all_patches(torch.zeros(1, 1, 10, 20, 19))
    with pytest.raises(ValueError, match="min_overlap"):
        net.predict_all_patches(torch.zeros(1, 1, 10, 20, 19), min_overlap=1.0)
    with pytest.raises(ValueError, match="patch_batch"):
        net.predict_all_patches(torch.zeros(1, 1, 10, 20, 19), patch_batch=0)
    with pytest.raises(ValueError, match="multiple of 4"):
        MobileNetASPP(3, patch_size=(16, 16, 18)).eval().predict_all_patches(torch.zeros(1, 1, 10, 20, 19))
    with pytest.raises(RuntimeError, match="GPU only"):
        net.backbone(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(ValueError, match="no model"):
        cnn_point_cloud([], torch.zeros(1, 1, 8, 8, 8), torch.ones(8, 8, 8))
    with pytest.raises(ValueError, match="one volume"):
        cnn_point_cloud(net, torch.zeros(2, 1, 8, 8, 8), torch.ones(8, 8, 8))


@pytest.mark.parametrize("name", [c[0] for c in cases.BLOCK_CASES[:8]])
def test_block_inputs_make_both_clamps_count(name):
    """at both ReLU6 sites of every block configuration the oracle's pre-activations fall below 0, inside [0, 6] and above 6 in
    at least 5 % of the entries each, for the inputs the GPU test feeds the kernel"""
    pre = cases.block_case(name)[5]
    for site, p in zip(("expand", "depthwise"), pre):
        fr = cases.fractions(p)
        print(name, site, "below 0 / inside / above 6:", " ".join(f"{f:.3f}" for f in fr))
        assert min(fr) >= 0.05, (name, site, fr)


def test_keypoint_case_has_few_ambiguous_voxels():
    """tests/test_seg_cnn_gpu.py compares keypoint SETS outside the voxels whose two largest scores lie within the error bar;
    those may be at most 1 % of the masked voxels.  The oracle's own fp32 run must satisfy what the kernels are asked for."""
    _, mask, p64, p32 = cases.keypoint_case()
    err32 = float((p32.double() - p64).abs().max())
    e = cases.bar(err32, p64)
    amb = cases.ambiguous(p64, e) & mask
    kp64, kp32 = so.cnn_keypoint_mask(p64, mask), so.cnn_keypoint_mask(p32, mask)
    print(f"keypoint case: fp32 oracle error {err32:.3e}, bar {e:.3e}, ambiguous {int(amb.sum())} of {int(mask.sum())} masked voxels, "
          f"{int(kp64.sum())} keypoints, {int((kp64 != kp32).sum())} differ in the fp32 run")
    assert int(amb.sum()) <= 0.01 * int(mask.sum())
    assert 0.05 * int(mask.sum()) < int(kp64.sum()) < 0.95 * int(mask.sum())     # both outcomes occur
    assert not bool(((kp64 != kp32) & ~amb).any())
