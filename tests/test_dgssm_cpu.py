"""CPU tests of the DG-SSM port (reference: models/dg_ssm.py, shape_model/ssm.py, losses/dgssm_loss.py): alias imports, the
constructor / state_dict / checkpoint contract against the real reference's fixtures, the refusals, host-side argument checks
of fsg_ssm_decode_*, and the torch oracle (tests/dgssm_oracle.py) against the same fixtures."""
import inspect
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dgssm_oracle import OracleMultiHeadDGCNN, decode_affine, project, ssm_shapes
from golden_util import cloud, fill_state_dict, load


def _fixture_ssm(g, prefix=""):
    return {n: torch.from_numpy(np.asarray(g[prefix + n])) for n in
            ("num_modes", "percent_of_variance", "mean_shape", "eigenvalues", "eigenvectors")}


def test_reference_imports_of_dgssm_resolve():
    """train_dgcnn_ssm.py:12-15, models/dg_ssm.py:10 and model_trainer.py:17 import these names; the trainer's
    isinstance(loss_function, DGSSMLoss) (model_trainer.py:75,164) must see this package's class"""
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from losses.dgssm_loss import CorrespondingPointDistance, DGSSMLoss, corresponding_point_distance  # noqa: F401
        from models.dg_ssm import DGSSM, MultiHeadDGCNN, RegressionHead, create_in_feature_hook  # noqa: F401
        from shape_model.ssm import LSSM, SSM, shape2vector, vector2shape  # noqa: F401
        import shape_model
        from fissure_segmentation_amd.losses import dgssm_loss
        from fissure_segmentation_amd.models import dg_ssm
        from fissure_segmentation_amd.shape_model import ssm
        assert DGSSM is dg_ssm.DGSSM and SSM is ssm.SSM and shape_model.ssm is ssm
        assert DGSSMLoss is dgssm_loss.DGSSMLoss and isinstance(dgssm_loss.DGSSMLoss(), DGSSMLoss)
        from losses.access_losses import get_loss_fn
        with pytest.raises(NotImplementedError):          # opening the registry name is a later decision
            get_loss_fn("ssm")
    finally:
        sys.modules.clear()
        sys.modules.update(saved)


def test_constructors_and_defaults():
    from fissure_segmentation_amd.losses.dgssm_loss import CorrespondingPointDistance, DGSSMLoss, corresponding_point_distance
    from fissure_segmentation_amd.models.dg_ssm import DGSSM, MultiHeadDGCNN
    from fissure_segmentation_amd.models.modelio import LoadableModel
    from fissure_segmentation_amd.shape_model.ssm import LSSM, SSM
    params = list(inspect.signature(DGSSM.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [
        ("k", inspect.Parameter.empty), ("in_features", inspect.Parameter.empty), ("spatial_transformer", False), ("dynamic", True),
        ("image_feat_module", False), ("predict_affine_params", True), ("ssm_alpha", 3.), ("ssm_targ_var", 0.95), ("ssm_modes", 1),
        ("lssm", False), ("only_affine", False)]
    params = list(inspect.signature(SSM.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("alpha", 2.5), ("target_variance", 0.95), ("dimensionality", 3)]
    net = DGSSM(k=20, in_features=3)
    assert isinstance(net, LoadableModel) and isinstance(net.ssm, SSM) and isinstance(net.dgcnn, MultiHeadDGCNN)
    assert net.config["ssm_modes"] == 1 and net.config["k"] == 20 and net.ssm.alpha == 3.
    assert net.predict_affine_params and not net.only_affine and net.dgcnn.args.emb_dims == 1024 and not net.dgcnn.args.static
    assert list(net.dgcnn.heads.keys()) == ["translation", "rotation", "scaling"]
    assert net.dgcnn.head_active == {"main": True, "translation": True, "rotation": True, "scaling": True}
    assert DGSSM(k=4, in_features=3, predict_affine_params=False, only_affine=True).predict_affine_params
    assert isinstance(DGSSM(k=4, in_features=3, lssm=True).ssm, LSSM)
    for kw in ({"spatial_transformer": True}, {"image_feat_module": True}):
        with pytest.raises(NotImplementedError):
            DGSSM(k=4, in_features=3, **kw)
    assert len(list(net.ssm.parameters())) == 0 and net.ssm.eigenvectors is None      # registered as None until fit
    loss = DGSSMLoss()
    assert (loss.w_point, loss.w_coefficients, loss.w_affine) == (1., 0.5, 0.5) == \
        (DGSSMLoss.DEFAULT_W_POINT, DGSSMLoss.DEFAULT_W_COEFFICIENTS, DGSSMLoss.DEFAULT_W_AFFINE)
    assert (DGSSMLoss(2., 3., 0.).w_point, DGSSMLoss(2., 3., 0.).w_affine) == (2., 0.)
    a, b = torch.zeros(2, 5, 3), torch.ones(2, 5, 3)
    torch.testing.assert_close(corresponding_point_distance(a, b), torch.full((2, 5), 3 ** 0.5))
    torch.testing.assert_close(CorrespondingPointDistance()(a, b), torch.tensor(3.))


def test_state_dict_keys_equal_the_reference_before_and_after_fit_ssm():
    from fissure_segmentation_amd.models.dg_ssm import DGSSM
    from fissure_segmentation_amd.shape_model.ssm import SSM
    g, gs = load("dgssm_step"), load("dgssm_ssm")
    ssm = SSM(alpha=3., target_variance=0.95)
    assert list(ssm.state_dict().keys()) == [str(s) for s in gs["keys_untrained"]] == []
    net = DGSSM(k=int(g["k"]), in_features=3)
    assert list(net.state_dict().keys()) == [str(s) for s in g["keys_before_fit"]]
    shapes = torch.from_numpy(ssm_shapes(int(gs["seed"]), int(gs["n"]), int(gs["P"])))
    torch.manual_seed(0)
    net.fit_ssm(shapes)
    assert list(net.state_dict().keys()) == [str(s) for s in g["keys"]]
    assert list(net.ssm.state_dict().keys()) == [str(s) for s in gs["keys"]]
    assert net.config["ssm_modes"] == int(g["ssm_modes"]) == net.dgcnn.linear3.out_features
    assert not any(p.requires_grad for p in net.ssm.parameters())
    assert net.ssm.eigenvectors.is_contiguous()


def test_ssm_fit_projection_and_decode_on_cpu_vs_reference_golden():
    """torch.pca_lowrank as the reference calls it: num_modes equal, eigenvalues 1e-4 relative, mean shape; signs of the
    eigenvectors are free, so projection and decode are compared through the reconstruction and with the fixture's model"""
    from fissure_segmentation_amd.shape_model.ssm import SSM, shape2vector, vector2shape
    g = load("dgssm_ssm")
    ev = g["eigenvalues"][0]
    assert (ev[:-1] / ev[1:]).min() >= 1.2
    shapes = torch.from_numpy(ssm_shapes(int(g["seed"]), int(g["n"]), int(g["P"])))
    torch.manual_seed(5)
    ssm = SSM(alpha=3., target_variance=0.95)
    ssm.fit(shapes)
    assert int(ssm.num_modes) == int(g["num_modes"]) and ssm.num_modes.dtype == torch.int64
    np.testing.assert_allclose(ssm.eigenvalues.numpy(), g["eigenvalues"], rtol=1e-4)
    np.testing.assert_allclose(float(ssm.percent_of_variance), float(g["percent_of_variance"]), rtol=1e-4)
    np.testing.assert_allclose(ssm.mean_shape.numpy(), g["mean_shape"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ssm.decode(ssm(shapes)).numpy(), g["reconstruction"], atol=1e-4 * float(shapes.abs().max()))
    fixed = SSM(alpha=3., target_variance=0.95)
    fixed.register_parameters_from_state_dict(_fixture_ssm(g))
    np.testing.assert_allclose(fixed(shapes).numpy(), g["projection"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(fixed.decode(torch.from_numpy(g["projection"])).numpy(), g["reconstruction"], rtol=1e-5, atol=1e-6)
    assert fixed.random_samples(4).shape == (4, int(g["num_modes"]))
    assert vector2shape(shape2vector(shapes)).shape == shapes.shape
    # the oracle's restatement of both
    mean, evec = torch.from_numpy(g["mean_shape"]), torch.from_numpy(g["eigenvectors"])
    np.testing.assert_allclose(project(shapes, mean, evec).numpy(), g["projection"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(decode_affine(torch.from_numpy(g["projection"]), mean, evec).numpy(), g["reconstruction"],
                               rtol=1e-5, atol=1e-6)


def test_checkpoint_round_trip(tmp_path):
    """DGSSM.load builds cls(**config) with an UNTRAINED shape model (its five parameters are None), loads non-strictly and
    takes the shape model's parameters from the state dict (dg_ssm.py:157-164); SSM.save / SSM.load alone as well"""
    from fissure_segmentation_amd.models.dg_ssm import DGSSM
    from fissure_segmentation_amd.shape_model.ssm import LSSM, SSM
    g = load("dgssm_step")
    net = DGSSM(k=4, in_features=3, dynamic=False)
    net.ssm.register_parameters_from_state_dict(_fixture_ssm(g, "ssm_"))
    net.config["ssm_modes"] = int(g["ssm_modes"])
    net.dgcnn.linear3 = torch.nn.Linear(256, int(g["ssm_modes"]))
    fill_state_dict(net.dgcnn, 3)
    net.save(tmp_path / "model.pth")
    back = DGSSM.load(tmp_path / "model.pth", "cpu")
    assert back.config == net.config and back.dgcnn.args.static
    assert list(back.state_dict().keys()) == list(net.state_dict().keys())
    for (n, a), (_, b) in zip(net.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a, b), n
    assert not any(p.requires_grad for p in back.ssm.parameters())
    net.ssm.save(tmp_path / "ssm.pth")
    for cls in (SSM, LSSM):     # a checkpoint of the localised model loads too: decode is the same
        ssm = cls.load(tmp_path / "ssm.pth", "cpu")
        assert torch.equal(ssm.eigenvectors, net.ssm.eigenvectors) and ssm.alpha == 3.
        w = torch.randn(2, int(g["ssm_modes"]))
        assert torch.equal(ssm.decode(w), net.ssm.decode(w))


def test_untrained_forward_raises_and_lssm_fit_is_refused():
    from fissure_segmentation_amd.models.dg_ssm import DGSSM
    from fissure_segmentation_amd.shape_model.ssm import LSSM, SSM
    with pytest.raises(ValueError, match="not trained"):
        DGSSM(k=4, in_features=3)(torch.randn(2, 3, 32))
    for call in (lambda s: s(torch.randn(2, 5, 3)), lambda s: s.decode(torch.randn(2, 1)), lambda s: s.random_samples(2)):
        with pytest.raises(ValueError, match="not trained"):
            call(SSM())
    with pytest.raises(NotImplementedError, match="LPCA"):
        LSSM().fit(torch.randn(6, 10, 3))
    with pytest.raises(NotImplementedError, match="LPCA"):
        DGSSM(k=4, in_features=3, lssm=True).fit_ssm(torch.randn(6, 10, 3))


def test_ssm_decode_entry_points_reject_bad_arguments():
    """host-side checks, before any launch: NULL pointers, shapes, M above the limit (FSG_ERR_UNSUPPORTED = 3), v / s / tr
    not all-or-none, a workspace that is too small"""
    from fissure_segmentation_amd import _lib
    from fissure_segmentation_amd import functional as F_hip
    p = 64                                                  # never dereferenced: the checks fail first
    ws = _lib.lib.fsg_ssm_decode_bwd_workspace_bytes
    assert ws(32, 2048, 20) == 32 * 32 * 35 * 4 and ws(1, 1, 1) == 16 * 4 and ws(4, 4097, 64) == 4 * 65 * 79 * 4 and ws(0, 5, 5) == 0
    assert F_hip.SSM_MAX_MODES == 64
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_ssm_decode_fwd_f32", None, p, p, None, None, None, 2, 16, 4, p, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_ssm_decode_fwd_f32", p, p, p, p, p, p, 2, 16, 4, None, None)
    with pytest.raises(RuntimeError, match="all or none"):
        _lib.call("fsg_ssm_decode_fwd_f32", p, p, p, p, None, p, 2, 16, 4, p, None)
    with pytest.raises(RuntimeError, match="all or none"):
        _lib.call("fsg_ssm_decode_fwd_f32", p, p, p, None, p, None, 2, 16, 4, p, None)
    for B, P, M in [(-1, 16, 4), (70000, 16, 4), (2, 0, 4), (2, 16, 0)]:
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_ssm_decode_fwd_f32", p, p, p, p, p, p, B, P, M, p, None)
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_ssm_decode_bwd_f32", p, p, p, p, p, p, B, P, M, p, p, p, p, p, 1 << 30, None)
    with pytest.raises(RuntimeError, match=r"code 3.*M=65"):
        _lib.call("fsg_ssm_decode_fwd_f32", p, p, p, p, p, p, 2, 16, 65, p, None)
    with pytest.raises(RuntimeError, match=r"code 3.*M=65"):
        _lib.call("fsg_ssm_decode_bwd_f32", p, p, p, p, p, p, 2, 16, 65, p, p, p, p, p, 1 << 30, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_ssm_decode_bwd_f32", None, p, p, p, p, p, 2, 16, 4, p, p, p, p, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):      # the workspace is required
        _lib.call("fsg_ssm_decode_bwd_f32", p, p, p, p, p, p, 2, 16, 4, p, p, p, p, None, 1 << 20, None)
    with pytest.raises(RuntimeError, match="all or none"):
        _lib.call("fsg_ssm_decode_bwd_f32", p, p, p, p, p, p, 2, 16, 4, p, p, None, p, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="all or none"):       # decode only: no small gradients
        _lib.call("fsg_ssm_decode_bwd_f32", p, p, p, p, None, None, 2, 16, 4, p, p, None, None, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("fsg_ssm_decode_bwd_f32", p, p, p, p, p, p, 2, 16, 4, p, p, p, p, p, ws(2, 16, 4) - 1, None)
    with pytest.raises(RuntimeError, match="GPU"):
        F_hip.ssm_decode_affine(torch.zeros(2, 4), torch.zeros(48), torch.zeros(48, 4))


def test_dgssm_oracle_vs_reference_golden():
    """the oracle the GPU tests compare against reproduces the real reference's train-mode step: main head, the three
    regression heads, the decoded shapes (before the transform), grad_x, every parameter gradient, the running statistics"""
    g = load("dgssm_step")
    seed, M = int(g["seed"]), int(g["ssm_modes"])
    args = SimpleNamespace(k=int(g["k"]), emb_dims=1024, dropout=0., static=bool(g["static"]))
    torch.manual_seed(0)
    net = fill_state_dict(OracleMultiHeadDGCNN(args, 3, M), seed).train()
    assert ["dgcnn." + k for k in net.state_dict().keys()] == [str(s) for s in g["keys"] if str(s).startswith("dgcnn.")]
    x = torch.from_numpy(cloud(seed + 1000, int(g["B"]), 3, int(g["N"]))).requires_grad_(True)
    main, others = net(x)
    mean, evec, ev = (torch.from_numpy(g["ssm_" + n]) for n in ("mean_shape", "eigenvectors", "eigenvalues"))
    outs = {"decoded": decode_affine(main.squeeze(-1) * ev, mean, evec), "rotation": others["rotation"],
            "translation": others["translation"], "scaling": others["scaling"]}
    rng = np.random.default_rng(seed + 2000)
    loss = 0
    for t in outs.values():
        loss = loss + (t * torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32))).sum()
    loss.backward()
    np.testing.assert_allclose(main.detach().numpy(), g["main"], rtol=1e-5, atol=1e-5)
    for n, t in outs.items():
        np.testing.assert_allclose(t.detach().numpy(), g[n], rtol=1e-5, atol=1e-5, err_msg=n)
    np.testing.assert_allclose(x.grad.numpy(), g["grad_x"], rtol=1e-4, atol=1e-4 * float(np.abs(g["grad_x"]).max()))
    for n, p in net.named_parameters():
        ref = float(g["gnorm_" + n])
        assert abs(float(p.grad.double().norm()) - ref) <= 1e-4 * ref + 1e-7, n
        head = g["ghead_" + n]
        np.testing.assert_allclose(p.grad.reshape(-1)[:16].numpy(), head, rtol=1e-4,
                                   atol=1e-4 * float(np.abs(head).max()) + 1e-7, err_msg=n)
    for n, b in net.named_buffers():
        if "running" in n:
            np.testing.assert_allclose(b.numpy(), g["buf_" + n], rtol=1e-5, atol=1e-6, err_msg=n)
