"""GPU tests of DG-SSM on HIP: the fused decode + similarity-transform kernel (forward and the four gradients) against the fp64
torch composition, bitwise reproducibility, SSM.fit on the device, the model against the real reference's fixtures and
against the CPU oracle at 4 x 1024 points, the loss, the batched test-time ensembling, inactive heads, and a full training
step captured into a hipGraph."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from dgssm_oracle import HEADS, OracleDGSSM, OracleMultiHeadDGCNN, decode_affine, dgssm_loss, pack, ssm_shapes, unpack
from golden_util import cloud, fill_state_dict, load
from test_gpu_parity import GraphTape, _model_vs_oracle, _ReplayRandperm, check_against_golden

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 301, 7), (32, 2048, 20), (4, 4097, 64)]
ROTATIONS = ["zero", "clamped", "ordinary", "near_pi"]
DGSSM_ARGS = dict(k=20, emb_dims=1024, dropout=0., static=False)


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def G(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def N(t):
    return t.detach().cpu().numpy()


def _case(B, P, M, rotation, seed):
    """w, mean, evec, v, s, tr, g on the CPU in fp32.  Rotation vectors: exactly zero; inside so3_exp_map's clamp
    (|v|^2 < 1e-4: t is constant there); ordinary angles in [0.3, 2]; |v| within 1e-3 of pi."""
    rng = np.random.default_rng(seed)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))  # noqa: E731
    axis = rng.standard_normal((B, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = {"zero": np.zeros((B, 1)), "clamped": rng.uniform(1e-3, 9e-3, (B, 1)), "ordinary": rng.uniform(0.3, 2.0, (B, 1)),
             "near_pi": np.pi - rng.uniform(0, 1e-3, (B, 1))}[rotation]
    return dict(w=f(rng.standard_normal((B, M))), mean=f(rng.uniform(-1, 1, 3 * P)),
                evec=f(rng.standard_normal((3 * P, M)) / np.sqrt(M)), v=f(axis * angle), s=f(rng.uniform(0.5, 1.5, (B, 3))),
                tr=f(0.3 * rng.standard_normal((B, 3))), g=f(rng.standard_normal((B, P, 3))))


def _composition(c, dtype, affine=True):
    """the torch composition (oracle: decode, so3_exp_map, bmm, scale, translate) with autograd, in `dtype` on the CPU"""
    names = ("w", "v", "s", "tr") if affine else ("w",)
    t = {n: c[n].to(dtype).requires_grad_(True) for n in names}
    out = decode_affine(t["w"], c["mean"].to(dtype), c["evec"].to(dtype), *([t["v"], t["s"], t["tr"]] if affine else []))
    out.backward(c["g"].to(dtype))
    return {"out": out.detach(), **{"d" + n: t[n].grad for n in names}}


def _fused(fsg, c, device, affine=True):
    names = ("w", "v", "s", "tr") if affine else ("w",)
    t = {n: c[n].to(device).requires_grad_(True) for n in names}
    out = fsg.functional.ssm_decode_affine(t["w"], c["mean"].to(device), c["evec"].to(device),
                                           *([t["v"], t["s"], t["tr"]] if affine else []))
    assert out.is_contiguous() and out.shape == c["g"].shape
    out.backward(c["g"].to(device))
    return {"out": out.detach(), **{"d" + n: t[n].grad for n in names}}


def _check_vs_fp64(got, c, affine, label):
    """bar: 1e-4 of the largest magnitude of the fp64 result, per output; the error of the SAME composition in fp32 torch is
    printed next to it"""
    want, torch32 = _composition(c, torch.float64, affine), _composition(c, torch.float32, affine)
    failures = []
    for name, ref in want.items():
        scale = float(ref.abs().max())
        err = float((got[name].detach().cpu().double() - ref).abs().max())
        err32 = float((torch32[name].double() - ref).abs().max())
        print(f"SSMDEC {label} {name:4s}: max|fp64| {scale:.3e}  fused err {err:.3e} ({err / max(scale, 1e-300):.1e} rel)  "
              f"fp32 torch err {err32:.3e}")
        if not err <= 1e-4 * scale:
            failures.append((name, err, scale))
    assert not failures, failures


@pytest.mark.parametrize("rotation", ROTATIONS)
@pytest.mark.parametrize("B,P,M", SHAPES)
def test_ssm_decode_affine_vs_fp64_composition(fsg, device, B, P, M, rotation):
    """forward and dw, dv, ds, dtr of the fused stage against the fp64 composition: one point / one mode, ragged P (not a
    multiple of the 64-point tile), the DG-SSM shape, and the mode limit"""
    c = _case(B, P, M, rotation, 1000 * P + M + ROTATIONS.index(rotation))
    _check_vs_fp64(_fused(fsg, c, device), c, True, f"{(B, P, M)} {rotation}")


@pytest.mark.parametrize("B,P,M", SHAPES)
def test_ssm_decode_only_vs_fp64_composition(fsg, device, B, P, M):
    """no transform (predict_affine_params=False, SSM.decode): out = mean + evec w, and dw"""
    c = _case(B, P, M, "zero", 77 + P)
    _check_vs_fp64(_fused(fsg, c, device, affine=False), c, False, f"{(B, P, M)} decode only")


def test_ssm_decode_refuses_more_modes_than_the_limit(fsg, device):
    c = _case(2, 16, 65, "ordinary", 1)
    with pytest.raises(RuntimeError, match="M=65"):
        fsg.functional.ssm_decode_affine(c["w"].to(device), c["mean"].to(device), c["evec"].to(device))
    with pytest.raises(ValueError):
        fsg.functional.ssm_decode_affine(c["w"].to(device), c["mean"].to(device), c["evec"].to(device), c["v"].to(device))


def test_ssm_decode_affine_is_bitwise_reproducible(fsg, device):
    """no atomics, fixed summation order: two runs give the same bits (forward and all four gradients)"""
    for B, P, M in [(32, 2048, 20), (4, 4097, 64)]:
        c = _case(B, P, M, "ordinary", 5)
        a, b = _fused(fsg, c, device), _fused(fsg, c, device)
        for name in a:
            assert torch.equal(a[name], b[name]), (B, P, M, name)


def test_ssm_decode_affine_under_autocast_and_broadcast_scale(fsg, device):
    """the Function leaves an ambient autocast region (fp32 in, fp32 out); a (B, 1) scaling broadcasts like
    compose_transform's scaling.expand(-1, 3) and its gradient is the sum over the three coordinates"""
    c = _case(3, 130, 5, "ordinary", 9)
    s1 = c["s"][:, :1].clone()
    t = {n: c[n].to(device).requires_grad_(True) for n in ("w", "v", "tr")}
    s = s1.to(device).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        out = fsg.functional.ssm_decode_affine(t["w"], c["mean"].to(device), c["evec"].to(device), t["v"], s, t["tr"])
    assert out.dtype == torch.float32
    out.backward(c["g"].to(device))
    c3 = dict(c, s=s1.expand(-1, 3).contiguous())
    want = _composition(c3, torch.float64)
    assert float((out.detach().cpu().double() - want["out"]).abs().max()) <= 1e-4 * float(want["out"].abs().max())
    ds = want["ds"].sum(1, keepdim=True)
    assert float((s.grad.cpu().double() - ds).abs().max()) <= 1e-4 * float(want["ds"].abs().max())


# --------------------------------------------------------------------------- the shape model on the device
def _fixture_ssm(g, prefix=""):
    return {n: torch.from_numpy(np.asarray(g[prefix + n])) for n in
            ("num_modes", "percent_of_variance", "mean_shape", "eigenvalues", "eigenvectors")}


def test_ssm_fit_on_gpu_vs_reference_golden(fsg, device):
    """SSM.fit (torch.pca_lowrank) on the device against the real reference's fit: num_modes equal, eigenvalues 1e-4
    relative, decode(forward(x)) of the training shapes within 1e-4 of their magnitude (decode = the HIP kernel).  The signs
    of the eigenvectors are free and not compared; the fixture's retained eigenvalues are separated by a ratio >= 1.2."""
    from fissure_segmentation_amd.shape_model.ssm import SSM
    g = load("dgssm_ssm")
    ev = g["eigenvalues"][0]
    assert (ev[:-1] / ev[1:]).min() >= 1.2
    shapes = G(ssm_shapes(int(g["seed"]), int(g["n"]), int(g["P"])), device)
    torch.manual_seed(11)
    ssm = SSM(alpha=3., target_variance=0.95).to(device)
    ssm.fit(shapes)
    assert int(ssm.num_modes) == int(g["num_modes"])
    assert ssm.eigenvectors.is_cuda and ssm.eigenvectors.is_contiguous() and not ssm.eigenvectors.requires_grad
    np.testing.assert_allclose(N(ssm.eigenvalues), g["eigenvalues"], rtol=1e-4)
    np.testing.assert_allclose(N(ssm.mean_shape), g["mean_shape"], rtol=1e-5, atol=1e-6)
    scale = float(shapes.abs().max())
    recon = ssm.decode(ssm(shapes))
    assert recon.shape == shapes.shape
    err_fixture = float(np.abs(N(recon) - g["reconstruction"]).max())
    err_shapes = float((recon - shapes).abs().max())
    print(f"SSMFIT reconstruction vs fixture {err_fixture:.3e}, vs training shapes {err_shapes:.3e}, magnitude {scale:.3e}")
    assert err_fixture <= 1e-4 * scale
    # the fixture's model on the device: projection and decode (kernel) against the reference's own numbers
    fixed = SSM(alpha=3., target_variance=0.95)
    fixed.register_parameters_from_state_dict(_fixture_ssm(g))
    fixed = fixed.to(device)
    np.testing.assert_allclose(N(fixed(shapes)), g["projection"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(N(fixed.decode(G(g["projection"], device))), g["reconstruction"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(N(fixed.decode(G(g["projection"], device)[:, :, None])), g["reconstruction"], rtol=1e-5, atol=1e-5)


# --------------------------------------------------------------------------- the model
def _dgssm_from_fixture(g, device, k=None, **kw):
    """DGSSM with the fixture's shape model and a main head of its number of modes (what fit_ssm leaves behind)"""
    from fissure_segmentation_amd.models.dg_ssm import DGSSM
    M = int(g["ssm_modes"])
    net = DGSSM(k=int(g["k"]) if k is None else k, in_features=3, ssm_modes=M, **kw)
    net.ssm.register_parameters_from_state_dict(_fixture_ssm(g, "ssm_"))
    return net.to(device) if device is not None else net


def test_dgssm_heads_and_decode_vs_reference_golden(fsg, device):
    """The real reference's train-mode step (MultiHeadDGCNN.forward, ssm.decode(coefficients * eigenvalues), seeded output
    gradients on the decoded shapes and the three heads): method and bars of test_upstream_dgcnn_vs_reference_golden for an
    ill-conditioned (train mode, k = 20) case -- outputs 3e-4, `loose` gradients, running statistics 1e-4.  The fixture is a
    case where the net is continuous at the level of fp32 rounding, which a comparison without replayed graphs needs
    (tools/make_golden_dgssm.py states the reasoning and checks it on the reference): 8 x 1024 points, k = 20, the graph
    built from the coordinates (`dynamic=False`, as open_static).  With the feature-space graph and four clouds two fp32
    implementations differ by 0.19 at the main head (a flipped neighbour, amplified by the heads' BatchNorms), with two
    clouds by 1.5e-3 (BatchNorm over two samples: noise of 1e-7 in the pooled feature moves the main head by 2e-4 .. 4e-4 in
    fp64); the dynamic net is compared at 4 x 1024 against the oracle with the graphs replayed, below."""
    g = load("dgssm_step")
    seed = int(g["seed"])
    net = _dgssm_from_fixture(g, None, dynamic=not bool(g["static"]))
    assert list(net.state_dict().keys()) == [str(s) for s in g["keys"]]
    fill_state_dict(net.dgcnn, seed)
    net = net.to(device).train()
    xt = G(cloud(seed + 1000, int(g["B"]), 3, int(g["N"])), device).requires_grad_(True)
    main, others = net.dgcnn(xt)
    decoded = net.ssm.decode(main.squeeze(-1) * net.ssm.eigenvalues)
    outs = {"decoded": decoded, "rotation": others["rotation"], "translation": others["translation"],
            "scaling": others["scaling"]}
    rng = np.random.default_rng(seed + 2000)
    loss = 0
    for t in outs.values():
        loss = loss + (t * G(rng.standard_normal(tuple(t.shape)).astype(np.float32), device)).sum()
    loss.backward()
    tol = dict(rtol=3e-4, atol=3e-4)
    for n, t in outs.items():
        np.testing.assert_allclose(N(t), g[n], err_msg=n, **tol)
    check_against_golden(net.dgcnn, g, main, xt.grad, "main", loose=True, out_tol=tol)
    for n, b in net.dgcnn.named_buffers():
        if "running" in n:
            np.testing.assert_allclose(N(b), g["buf_" + n], rtol=1e-4, atol=1e-4, err_msg=n)


class _Packed(nn.Module):
    """DGSSM with its triple packed into one tensor and only the trainable part (dgcnn) visible as parameters"""

    def __init__(self, model):
        super().__init__()
        self.dgcnn = model.dgcnn
        self._model = (model,)

    def forward(self, x):
        return pack(self._model[0](x))


class _PackedOracle(OracleDGSSM):
    def forward(self, x):
        return pack(super().forward(x))


def _loss_target(g, B, seed):
    """a target triple on the CPU: shapes decoded from seeded weights, their weights, small affine parameters"""
    rng = np.random.default_rng(seed)
    mean, evec, ev = (torch.from_numpy(g["ssm_" + n]) for n in ("mean_shape", "eigenvectors", "eigenvalues"))
    w = torch.from_numpy(rng.standard_normal((B, ev.shape[1])).astype(np.float32)) * ev
    affine = np.concatenate([0.3 * rng.standard_normal((B, 3)), 0.1 * rng.standard_normal((B, 3)), rng.uniform(0.9, 1.0, (B, 3))], 1)
    return decode_affine(w, mean, evec), w, torch.from_numpy(affine.astype(np.float32))


def test_dgssm_forward_backward_vs_oracle_through_the_point_loss(fsg, device, monkeypatch):
    """DGSSM.forward + DGSSMLoss with ONLY the point term (w_coefficients = w_affine = 0) at 4 x 1024, k = 20, train mode,
    against the CPU oracle with the HIP graphs replayed: every gradient then flows through ssm_decode_affine -- to linear3
    through the decode, to the rotation / translation / scaling heads through the transform (the path that carried no
    gradient before).  Outputs 1e-4, loss 1e-4, gradients at the flip-aware bar of _model_vs_oracle on all tensors; the
    gradients of the three heads and of linear3 are non-zero."""
    from fissure_segmentation_amd.losses.dgssm_loss import DGSSMLoss
    g = load("dgssm_step")
    M, B = int(g["ssm_modes"]), 4
    ssm = _fixture_ssm(g, "ssm_")
    ref = _PackedOracle(fill_state_dict(OracleMultiHeadDGCNN(SimpleNamespace(**DGSSM_ARGS), 3, M), 31),
                        ssm["mean_shape"], ssm["eigenvalues"], ssm["eigenvectors"]).train()
    model = _dgssm_from_fixture(g, None)
    model.dgcnn.load_state_dict(ref.dgcnn.state_dict())
    model = model.to(device).train()
    net = _Packed(model)
    target = _loss_target(g, B, 32)
    crit = DGSSMLoss(1., 0., 0.)

    def hip_loss(y, x):
        total, comp = crit(unpack(y, M), tuple(t.to(device) for t in target))
        assert set(comp) == {"Point-Loss", "Coefficients"}
        return total

    def ref_loss(y, x):
        return dgssm_loss(unpack(y, M), tuple(t.to(y.dtype) for t in target), 1., 0., 0.)[0]

    _model_vs_oracle(net, ref, cloud(5400, B, 3, 1024), 0, device, 1e-4, 1e-3, tape=GraphTape(fsg, monkeypatch),
                     loss_fn=hip_loss, ref_loss_fn=ref_loss)
    scale = max(float(p.grad.norm()) for p in model.dgcnn.parameters())
    for name in ("linear3.weight", "linear3.bias") + tuple(f"heads.{h}.layers.{i}.weight" for h in HEADS for i in (0, 4, 8)):
        p = dict(model.dgcnn.named_parameters())[name]
        assert p.grad is not None and float(p.grad.norm()) > 1e-6 * scale, name
    assert all(p.grad is None for p in model.ssm.parameters())


def test_dgssm_only_affine_and_no_affine_paths(fsg, device):
    """only_affine: zero weights (the mean shape, moved); predict_affine_params=False: decode alone, returned transposed
    (B, 3, P) as the reference does, identity affine parameters"""
    g = load("dgssm_step")
    x = G(cloud(41, 3, 3, 256), device)
    mean = G(g["ssm_mean_shape"], device).view(1, -1, 3)
    torch.manual_seed(1)
    net = _dgssm_from_fixture(g, device, k=8, only_affine=True).eval()
    with torch.no_grad():
        recon, w, affine = net(x)
    assert w.shape == (3, int(g["ssm_modes"]), 1) and float(w.abs().max()) == 0 and affine.shape == (3, 9)
    want = decode_affine(torch.zeros(3, int(g["ssm_modes"]), dtype=torch.float64), mean.cpu().double(),
                         torch.from_numpy(g["ssm_eigenvectors"]).double(), *(affine[:, i].cpu().double() for i in
                                                                             (slice(0, 3), slice(6, 9), slice(3, 6))))
    assert float((recon.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    net = _dgssm_from_fixture(g, device, k=8, predict_affine_params=False).eval()
    with torch.no_grad():
        recon, w, affine = net(x)
    assert recon.shape == (3, 3, mean.shape[1]) and w.shape == (3, int(g["ssm_modes"]))
    want = decode_affine(w.cpu().double(), mean.cpu().double(), torch.from_numpy(g["ssm_eigenvectors"]).double())
    assert float((recon.transpose(1, 2).cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert torch.equal(affine.cpu(), torch.tensor([[0., 0, 0, 0, 0, 0, 1, 1, 1]]).expand(3, 9))


# --------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("w_affine", [0.5, 0.])
def test_dgssm_loss_vs_fp64_oracle(fsg, device, w_affine):
    """total and every component against the fp64 oracle at 1e-4 relative; w_affine = 0 drops the 'Affine-Params' component;
    the gradient reaches the predicted shape, weights and affine parameters"""
    from fissure_segmentation_amd.losses.dgssm_loss import DGSSMLoss
    rng = np.random.default_rng(51)
    B, P, M = 4, 700, 7
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    pred = (f(B, P, 3), f(B, M), f(B, 9))
    targ_affine = torch.cat([0.3 * f(B, 3), 0.1 * f(B, 3), 1 + 0.1 * f(B, 3)], 1)
    target = (pred[0] + 0.1 * f(B, P, 3), f(B, M), targ_affine)
    crit = DGSSMLoss(0.7, 0.4, w_affine)
    pred_dev = tuple(t.to(device).requires_grad_(True) for t in pred)
    total, comp = crit(pred_dev, tuple(t.to(device) for t in target))
    want, want_comp = dgssm_loss(tuple(t.double() for t in pred), tuple(t.double() for t in target), 0.7, 0.4, w_affine)
    assert list(comp) == ["Point-Loss", "Coefficients"] + (["Affine-Params"] if w_affine else [])
    assert set(comp) == set(want_comp)
    for n in comp:
        print(f"DGSSMLOSS {n}: {float(comp[n]):.8e} vs fp64 {float(want_comp[n]):.8e}")
        assert abs(float(comp[n]) - float(want_comp[n])) <= 1e-4 * abs(float(want_comp[n])), n
    assert abs(float(total) - float(want)) <= 1e-4 * abs(float(want))
    total.backward()
    assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in pred_dev[:2])
    assert (pred_dev[2].grad is not None and float(pred_dev[2].grad.abs().max()) > 0) == bool(w_affine)


def test_trainer_special_case_runs_under_disabled_autocast(fsg, device):
    """model_trainer.py:157-169 literally: autocast(enabled=False) because the loss is a DGSSMLoss (:75), output = model(x),
    target weights = model.ssm(shape) under no_grad, y = (shape, target_weights, affine); then loss and backward"""
    from fissure_segmentation_amd.losses.dgssm_loss import DGSSMLoss
    g = load("dgssm_step")
    torch.manual_seed(2)
    model = _dgssm_from_fixture(g, device, k=8).train()
    loss_function = DGSSMLoss()
    autocast_enabled = not isinstance(loss_function, (DGSSMLoss,))
    x = G(cloud(61, 4, 3, 256), device)
    y = _loss_target(g, 4, 62)
    with torch.autocast("cuda", enabled=autocast_enabled):
        output = model(x)
        shape = y[0].to(device)
        with torch.no_grad():
            target_weights = model.ssm(shape)
        y = (shape, target_weights, y[2].to(device))
        loss, components = loss_function(output, y)
    assert target_weights.shape == output[1].shape == (4, int(g["ssm_modes"])) and output[0].shape == shape.shape
    loss.backward()
    assert torch.isfinite(loss) and set(components) == {"Point-Loss", "Coefficients", "Affine-Params"}
    want, _ = dgssm_loss(tuple(t.detach().cpu().double() for t in output), tuple(t.cpu().double() for t in y))
    assert abs(float(loss) - float(want)) <= 1e-4 * abs(float(want))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.dgcnn.parameters())


# --------------------------------------------------------------------------- ensembling, heads
def _close_prediction(got, want, **tol):
    assert got[0].shape == want[0].shape and set(got[1]) == set(want[1]) == set(HEADS)
    torch.testing.assert_close(got[0], want[0], **tol)
    for name in HEADS:
        torch.testing.assert_close(got[1][name], want[1][name], **tol)


def test_multihead_predict_full_pointcloud_batched_equals_sequential(fsg, device):
    """eval mode, no grad: the runs go through the net in chunks of `ensemble_max_clouds` and equal the reference's
    sequential loop (dg_ssm.py:66-82) under the same generator state, for the main head and the three other heads (1e-5,
    the bar of the backbone's ensembling test: the batch size changes the GEMM tiling only).  Train mode takes the loop."""
    from fissure_segmentation_amd.models.dg_ssm import DGSSM
    torch.manual_seed(3)
    net = DGSSM(k=16, in_features=3, ssm_modes=6).to(device).dgcnn
    pc = G(cloud(12, 2, 3, 3000), device)
    net.train()
    with torch.no_grad():                       # running statistics away from their initial values
        for _ in range(2):
            net(pc[..., :512].contiguous())
    net.eval()
    net.ensemble_max_clouds = 8                 # 4 runs of 2 clouds per forward: 10 runs = chunks of 4, 4, 2
    assert net._ensemble_batchable(pc) is False        # grad mode on: sequential
    calls = []
    hook = net.register_forward_pre_hook(lambda m, inp: calls.append(inp[0].shape[0]))
    with torch.no_grad():
        assert net._ensemble_batchable(pc)
        torch.manual_seed(77)
        got = net.predict_full_pointcloud(pc, sample_points=512, n_runs_min=10)
        assert calls == [8, 8, 4]
        net._ensemble_batchable = lambda _pc: False
        torch.manual_seed(77)
        want = net.predict_full_pointcloud(pc, sample_points=512, n_runs_min=10)
        del net._ensemble_batchable
    assert got[0].shape == (2, 6, 1) and got[1]["rotation"].shape == (2, 3)
    _close_prediction(got, want, rtol=0, atol=1e-5)
    net.train()
    with torch.no_grad():
        assert net._ensemble_batchable(pc) is False     # train mode couples the batch through BatchNorm
        calls.clear()
        net.predict_full_pointcloud(pc, sample_points=512, n_runs_min=3)
    assert calls == [2, 2, 2]
    hook.remove()


@pytest.mark.parametrize("batched", [True, False])
def test_multihead_predict_full_pointcloud_vs_reference_golden(fsg, device, monkeypatch, batched):
    """dg_ssm.py:66-82 as run by the reference on its own MultiHeadDGCNN (eval mode): the recorded randperm rows are
    replayed -- same calls in the same order -- and all four outputs agree (bar of the segmentation nets' ensembling test)"""
    from fissure_segmentation_amd.models.dg_ssm import DGSSM
    g = load("dgssm_ensemble")
    net = DGSSM(k=int(g["k"]), in_features=3, ssm_modes=int(g["modes"])).dgcnn
    net = fill_state_dict(net, int(g["seed"])).to(device).eval()
    replay = _ReplayRandperm(g, device)
    monkeypatch.setattr(torch, "randperm", replay)
    if not batched:
        net._ensemble_batchable = lambda _pc: False
    with torch.no_grad():
        main, others = net.predict_full_pointcloud(G(cloud(int(g["seed"]) + 1000, int(g["B"]), 3, int(g["N"])), device),
                                                   sample_points=int(g["sample_points"]), n_runs_min=int(g["n_runs"]))
    assert replay.i == len(replay.rows) == int(g["n_runs"])
    np.testing.assert_allclose(N(main), g["main"], rtol=1e-4, atol=1e-5)
    for name in HEADS:
        np.testing.assert_allclose(N(others[name]), g[name], rtol=1e-4, atol=1e-5, err_msg=name)


def test_set_head_active(fsg, device):
    """an inactive head returns zeros (ones for the scaling) and its parameters get no gradient; the main head too"""
    g = load("dgssm_step")
    torch.manual_seed(4)
    net = _dgssm_from_fixture(g, device, k=8).train()
    x = G(cloud(71, 4, 3, 256), device)
    net.set_head_active("rotation", False)
    net.set_head_active("scaling", False)
    recon, w, affine = net(x)
    assert float(affine[:, 0:3].abs().max()) == 0 and bool((affine[:, 6:9] == 1).all()) and float(affine[:, 3:6].abs().max()) > 0
    recon.square().mean().backward()
    named = dict(net.dgcnn.named_parameters())
    for n, p in named.items():
        inactive = n.startswith("heads.rotation") or n.startswith("heads.scaling")
        assert (p.grad is None) == inactive, n
    assert float(named["heads.translation.layers.8.weight"].grad.abs().max()) > 0
    assert float(named["linear3.weight"].grad.abs().max()) > 0
    net.set_head_active("rotation", True)
    net.set_head_active("scaling", True)
    net.set_head_active("main", False)
    recon, w, affine = net(x)
    assert float(w.abs().max()) == 0 and float(affine[:, 0:3].abs().max()) > 0
    assert net.dgcnn.head_active == {"main": False, "translation": True, "rotation": True, "scaling": True}


# --------------------------------------------------------------------------- a full training step as a hipGraph
def test_dgssm_full_step_graph_replay_equals_eager(fsg, device):
    """forward, DGSSMLoss, backward and FlatAdam at 32 x 1024 points, k = 20: the step captures (nothing in it synchronises
    with the host -- a capture fails otherwise) and its replay from the same state gives the bits of the eager step: loss,
    components, parameters after the update, running statistics.  (Ordered Chamfer backward: set_deterministic.)"""
    from fissure_segmentation_amd.losses.dgssm_loss import DGSSMLoss
    from fissure_segmentation_amd.optim import FlatAdam
    g = load("dgssm_step")
    B = 32
    torch.manual_seed(0)
    net = _dgssm_from_fixture(g, device).train()
    opt = FlatAdam(net.parameters(), lr=1e-3, capturable=True)
    crit = DGSSMLoss()
    x = G(cloud(5500, B, 3, 1024), device)
    target = tuple(t.to(device) for t in _loss_target(g, B, 5501))
    was = fsg.functional.deterministic()
    fsg.functional.set_deterministic(True)
    try:
        def step():
            opt.zero_grad(set_to_none=True)
            loss, comp = crit(net(x), target)
            loss.backward()
            opt.step()
            return [loss.detach()] + [c.detach() for c in comp.values()]

        def snapshot(vals):
            return [v.clone() for v in vals] + [opt.flat.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + \
                   [b.clone() for n, b in net.named_buffers() if "running" in n]

        def restore(state):
            net.load_state_dict(state["net"])                 # in place: the graph keeps pointing at these tensors
            with torch.no_grad():
                opt.exp_avg.copy_(state["m"]); opt.exp_avg_sq.copy_(state["v"]); opt._state.copy_(state["s"])

        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                                            # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        state = dict(net=copy.deepcopy(net.state_dict()), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), s=opt._state.clone())
        eager = snapshot(step())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = step()
        restore(state)
        graph.replay()
        torch.cuda.synchronize()
        replayed = snapshot(static)
    finally:
        fsg.functional.set_deterministic(was)
    assert bool(torch.isfinite(eager[0]))
    assert float(eager[len(static) + 1].abs().max()) > 0                  # Adam's first moment: a real update
    for i, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), f"graph replay vs eager, tensor {i}"
