"""CPU tests of the upstream DGCNN / PointNet port (models/dgcnn_opensrc.py of the reference): the alias import DG-SSM and
affine_dgcnn.py rely on, the constructor / state_dict contract, PointNet against the real reference's fixtures, the torch
oracle of the upstream DGCNN against the same fixtures, and host-side argument checks of fsg_bn_act_maxavg_*."""
import inspect
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from golden_util import cloud, fill_state_dict, load
from opensrc_oracle import OpenDGCNN

DGCNN_FIXTURES = ["open_dynamic", "open_static", "open_fallback_train", "open_fallback_eval", "open_eval"]
POINTNET_FIXTURES = ["open_pointnet_eval", "open_pointnet_train"]
OUT_CHANNELS = 5


def dgcnn_args(g):
    return SimpleNamespace(k=int(g["k"]), emb_dims=int(g["emb"]), dropout=0., static=bool(g["static"]))


def run_step(net, g):
    """forward + backward on the fixture's seeded input and output gradient (B = 2)"""
    seed = int(g["seed"])
    xt = torch.from_numpy(cloud(seed + 1000, 2, int(g["cin"]) if "cin" in g else 3, int(g["N"]))).requires_grad_(True)
    y = net(xt)
    gr = np.random.default_rng(seed + 2000).standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(torch.from_numpy(gr))
    return y, xt.grad


def check_fixture(net, g, tol=1e-5):
    y, gx = run_step(net, g)
    np.testing.assert_allclose(y.detach().numpy(), g["out"], rtol=tol, atol=tol)
    np.testing.assert_allclose(gx.numpy(), g["grad_x"], rtol=1e-4, atol=1e-4 * float(np.abs(g["grad_x"]).max()))
    for n, p in net.named_parameters():
        ref = float(g["gnorm_" + n])
        assert abs(float(p.grad.double().norm()) - ref) <= 1e-4 * ref + 1e-7, n
        head = g["ghead_" + n]
        np.testing.assert_allclose(p.grad.reshape(-1)[:16].numpy(), head, rtol=1e-4,
                                   atol=1e-4 * float(np.abs(head).max()) + 1e-7, err_msg=n)
    for n, b in net.named_buffers():
        if "running" in n:
            np.testing.assert_allclose(b.numpy(), g["buf_" + n], rtol=1e-5, atol=1e-6, err_msg=n)


def test_reference_import_of_dgcnn_and_pointnet_resolves():
    """models/dg_ssm.py:7 and affine_dgcnn.py:15 import DGCNN / PointNet from the aliased models.dgcnn_opensrc"""
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from models.dgcnn_opensrc import DGCNN, PointNet  # noqa: F401
        from fissure_segmentation_amd.models import dgcnn_opensrc
        assert DGCNN is dgcnn_opensrc.DGCNN and PointNet is dgcnn_opensrc.PointNet
    finally:
        sys.modules.clear()
        sys.modules.update(saved)


def test_dgcnn_constructor_and_state_dict_contract():
    from fissure_segmentation_amd.models.dgcnn_opensrc import DGCNN, PointNet
    params = list(inspect.signature(DGCNN.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("args", inspect.Parameter.empty),
                                                     ("input_channels", inspect.Parameter.empty), ("output_channels", 40)]
    params = list(inspect.signature(PointNet.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("args", inspect.Parameter.empty), ("output_channels", 40)]
    net = DGCNN(SimpleNamespace(k=20, emb_dims=1024, dropout=0., static=False), 3, 5)
    assert not hasattr(net, "config")                       # a plain nn.Module in the reference, not a LoadableModel
    assert len(net.state_dict()) == 70
    assert net.k == 20 and net.conv1[1] is net.bn1 and net.conv5[1] is net.bn5
    assert {"conv1.1.weight", "bn1.weight", "conv5.1.running_var", "bn5.running_var"} <= set(net.state_dict())
    assert net.linear3.out_features == 5 and isinstance(net.dp2, torch.nn.Dropout)
    for name in DGCNN_FIXTURES:
        g = load(name)
        net = DGCNN(dgcnn_args(g), int(g["cin"]), OUT_CHANNELS)
        assert list(net.state_dict().keys()) == [str(s) for s in g["keys"]], name
        assert list(OpenDGCNN(dgcnn_args(g), int(g["cin"]), OUT_CHANNELS).state_dict().keys()) == [str(s) for s in g["keys"]]
    for name in POINTNET_FIXTURES:
        g = load(name)
        net = PointNet(SimpleNamespace(emb_dims=int(g["emb"]), dropout=0.), OUT_CHANNELS)
        assert list(net.state_dict().keys()) == [str(s) for s in g["keys"]], name


def test_dgcnn_refuses_cpu_input():
    from fissure_segmentation_amd.models.dgcnn_opensrc import DGCNN
    net = DGCNN(SimpleNamespace(k=4, emb_dims=64, dropout=0., static=False), 3, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.randn(2, 3, 32))


@pytest.mark.parametrize("name", POINTNET_FIXTURES)
def test_pointnet_vs_reference_golden_on_cpu(name):
    from fissure_segmentation_amd.models.dgcnn_opensrc import PointNet
    g = load(name)
    net = fill_state_dict(PointNet(SimpleNamespace(emb_dims=int(g["emb"]), dropout=0.), OUT_CHANNELS), int(g["seed"]))
    check_fixture(net.train(bool(g["train"])), g)


@pytest.mark.parametrize("name", DGCNN_FIXTURES)
def test_upstream_dgcnn_oracle_vs_reference_golden(name):
    """the oracle the GPU tests compare against at DG-SSM scale reproduces the real reference (torch kNN, as the reference)"""
    g = load(name)
    torch.manual_seed(0)
    net = fill_state_dict(OpenDGCNN(dgcnn_args(g), int(g["cin"]), OUT_CHANNELS), int(g["seed"]))
    check_fixture(net.train(bool(g["train"])), g)


def test_bn_act_maxavg_entry_points_reject_bad_arguments():
    """host-side checks, before any launch: NULL pointers and shapes outside the envelope (C % 64 == 0)"""
    from fissure_segmentation_amd import _lib
    assert _lib.lib.fsg_bn_act_maxavg_workspace_bytes(32, 1024, 1024) > _lib.lib.fsg_bn_act_max_workspace_bytes(32, 1024, 1024)
    p = 64                                                  # never dereferenced: the checks fail first
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_bn_act_maxavg_fwd_f32", None, p, p, None, None, 2, 16, 64, 1, 0.1, 1e-5, 0.2, p, p, p, p, p, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):   # the workspace is required in both modes
        _lib.call("fsg_bn_act_maxavg_fwd_f32", p, p, p, None, None, 2, 16, 64, 0, 0.1, 1e-5, 0.2, p, p, p, p, None, None)
    for B, N, C in [(2, 16, 96), (0, 16, 64), (2, 0, 64), (2, 16, 0), (70000, 1, 64)]:
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_bn_act_maxavg_fwd_f32", p, p, p, p, p, B, N, C, 1, 0.1, 1e-5, 0.2, p, p, p, p, p, None)
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_bn_act_maxavg_bwd_f32", p, p, p, p, p, p, p, B, N, C, 1, 0.2, p, p, p, p, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_bn_act_maxavg_bwd_f32", p, p, None, p, p, p, p, 2, 16, 64, 1, 0.2, p, p, p, p, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_bn_act_maxavg_bwd_f32", p, p, p, p, p, p, p, 2, 16, 64, 1, 0.2, p, p, p, None, None)
