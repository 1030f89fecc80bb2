"""CPU tests of tests/edgeconv_oracle.py: the fp64 EdgeConv compositions against the recorded reference (the fixtures and
tolerances of test_oracle_golden.py::test_edgeconv_restatement), the degree-prescribed graphs, the near-tie rows."""
import numpy as np
import pytest
import torch

import edgeconv_oracle as eo
from golden_util import cloud, fill_state_dict, load
from oracle import ref_cpu
from test_oracle_golden import TOL, T


@pytest.mark.parametrize("name", ["edgeconv_first", "edgeconv_feat", "edgeconv_c15"])
def test_edgeconv_fp64_oracle_vs_reference(name):
    g = load(name)
    seed, cin, k, N = int(g["seed"]), int(g["cin"]), int(g["k"]), int(g["N"])
    couts = [int(c) for c in g["couts"]]
    ec = fill_state_dict(ref_cpu.EdgeConv(cin, couts, k, first_layer=bool(g["first"])), seed)
    x = T(cloud(seed + 1000, 2, cin, N))
    idx = ref_cpu.knn(x[:, :3] if bool(g["first"]) else x, k, self_loop=True)
    x64 = x.double().requires_grad_(True)
    P, stats = [], []
    for blk in ec.shared_mlp:
        conv, bn = blk.layers[0], blk.layers[1]
        P.append([conv.weight.detach().double().view(conv.weight.shape[0], -1).requires_grad_(True),
                  bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True),
                  bn.running_mean.double(), bn.running_var.double()])
    if len(P) == 1:
        r = eo.edgeconv1_fp64(x64, idx, *P[0], True, 0.2, 1e-5, 0.1)
        stats = [(r["rm"], r["rv"])]
    else:
        r = eo.edgeconv2_fp64(x64, idx, *P[0], *P[1], True, 0.2, 1e-5, 0.1)
        stats = [(r["rm1"], r["rv1"]), (r["rm2"], r["rv2"])]
    assert r["act"].shape == (2, N, k, couts[-1]) and torch.equal(r["act"].max(2)[0].permute(0, 2, 1), r["out"])
    gr = np.random.default_rng(seed + 2000).standard_normal(tuple(r["out"].shape)).astype(np.float32)
    r["out"].backward(T(gr).double())
    np.testing.assert_allclose(r["out"].detach().numpy(), g["y"], **TOL)
    np.testing.assert_allclose(x64.grad.numpy(), g["grad_x"], **TOL)
    for li, (L, (rm, rv)) in enumerate(zip(P, stats)):
        pre = f"shared_mlp.{li}.layers."
        np.testing.assert_allclose(L[0].grad.numpy().reshape(g["grad_" + pre + "0.weight"].shape), g["grad_" + pre + "0.weight"],
                                   rtol=1e-3, atol=2e-4)
        np.testing.assert_allclose(L[1].grad.numpy(), g["grad_" + pre + "1.weight"], rtol=1e-3, atol=2e-4)
        np.testing.assert_allclose(L[2].grad.numpy(), g["grad_" + pre + "1.bias"], rtol=1e-3, atol=2e-4)
        np.testing.assert_allclose(rm.numpy(), g["buf_" + pre + "1.running_mean"], **TOL)
        np.testing.assert_allclose(rv.numpy(), g["buf_" + pre + "1.running_var"], **TOL)


def test_aten_composition_matches_fp64_oracle():
    """the fp32 yardstick computes the same function (output, running statistics, grad_x) as the fp64 oracle"""
    x, layers, G = eo.case_inputs(3, 2, 5, 40, [64, 64])
    idx = eo.graph_with_in_degrees(2, 40, 6, seed=3)
    x64 = T(x).double().requires_grad_(True)
    r = eo.edgeconv2_fp64(x64, idx, *[T(a).double() for a in layers[0]], *[T(a).double() for a in layers[1]], True)
    r["out"].backward(T(G).double().permute(0, 2, 1))
    x32 = T(x).requires_grad_(True)
    P = [[T(a).clone() for a in L] for L in layers]
    a = eo.edgeconv_aten_fp32(x32, idx, P, True)
    a["out"].backward(T(G).permute(0, 2, 1))
    assert float((a["out"].detach().double() - r["out"]).abs().max()) <= 1e-5 * float(r["out"].detach().abs().max())
    assert eo.norm_error(x32.grad, x64.grad) <= 1e-5
    for got, want in zip((P[0][3], P[0][4], P[1][3], P[1][4]), (r["rm1"], r["rv1"], r["rm2"], r["rv2"])):
        assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("B,N,k", [(2, 300, 20), (1, 77, 7), (2, 130, 64), (2, 100, 3), (3, 513, 16)])
def test_graph_with_in_degrees(B, N, k):
    idx = eo.graph_with_in_degrees(B, N, k, seed=N + k)
    assert idx.dtype == torch.int32 and idx.shape == (B, N, k)
    a = idx.numpy()
    assert a.min() >= 0 and a.max() < N
    deg = eo.fitted_degrees(N, k)
    want = eo.STANDARD_DEGREES
    assert deg == want[:len(deg)] and sum(deg) <= N * k and (len(deg) == len(want) or sum(want[:len(deg) + 1]) > N * k)
    assert np.array_equal(np.bincount(a[0].reshape(-1), minlength=N)[:len(deg)], deg)
    for b in range(1, B):
        assert np.array_equal(a[b, :, 0], np.arange(N))
    assert torch.equal(idx, eo.graph_with_in_degrees(B, N, k, seed=N + k))                 # seeded
    assert not torch.equal(idx[0], eo.graph_with_in_degrees(B, N, k, seed=N + k + 1)[0])
    if N * k >= sum(want):
        assert len(deg) == len(want) and int(np.bincount(a[0].reshape(-1)).max()) == 1100


def test_tie_rows_hand_made():
    """B = 1, N = 6, k = 3, two channels.  Point 0, channel 0: slots -> points (1, 2, 3) with activations (5, 5, 1): an exact tie
    between two DIFFERENT points -> rows 0, 1, 2.  Point 4, channel 1: slots -> (5, 5, 3) with (7, 7, 1): the tie is between two
    slots of the same point -> nothing.  Everything else has a clear winner."""
    idx = torch.tensor([[[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [5, 5, 3], [0, 1, 2]]], dtype=torch.int32)
    act = torch.zeros(1, 6, 3, 2, dtype=torch.float64)
    act[..., 0] = torch.tensor([3.0, 2.0, 1.0])
    act[..., 1] = torch.tensor([1.0, 2.0, 3.0])
    act[0, 0, :, 0] = torch.tensor([5.0, 5.0, 1.0])
    act[0, 4, :, 1] = torch.tensor([7.0, 7.0, 1.0])
    assert eo.tie_rows(act, idx, 0.0).tolist() == [True, True, True, False, False, False]
    act[0, 0, :, 0] = torch.tensor([5.0, 4.0, 1.0])                                        # a clear winner: nothing at all
    assert not eo.tie_rows(act, idx, 0.0).any()
    assert eo.tie_rows(act, idx, 1.0).tolist() == [True, True, True, True, False, True]     # margins of 1 everywhere but at point 4, which nobody names
    # a near-tie inside the noise, and the LeakyReLU kink: a best activation within the noise of zero marks i and the winner
    act[0, 0, :, 0] = torch.tensor([5.0, 5.0 - 1e-7, 1.0])
    assert eo.tie_rows(act, idx, 1e-6).tolist() == [True, True, True, False, False, False]
    act[0, 0, :, 0] = torch.tensor([5.0, 4.0, 1.0])
    act[0, 3, :, 1] = torch.tensor([-3.0, -2.0, 1e-7])
    assert eo.tie_rows(act, idx, 1e-6).tolist() == [False, False, True, True, False, False]
