"""GPU tests of the fused EdgeConv kernels (csrc/edgeconv.hip, csrc/edgeconv2.hip) against the fp64 oracle of
tests/edgeconv_oracle.py: graphs with prescribed in-degrees (0, 1, around the 20-edge rounds and the 64-edge chunks of the
backward gathers, a hub above the CSR builder's LDS sort capacity), every route by which the output gradient can arrive,
clouds with duplicated points, reproducibility.

How a case is judged (test_edgeconv1_vs_fp64, test_edgeconv2_vs_fp64 and the tests built on `_check`):
  * output and running statistics: max error <= 1e-4 * scale (scale = max |fp64 value|).
  * grad_x PER ROW (edgeconv_oracle.row_error) on the rows that edgeconv_oracle.tie_rows keeps; parameter gradients in norm,
    mathematically zero ones skipped.  Bound: max(floor, 3 x the same statistic of the pure-ATen fp32 composition against fp64).
    Floors: 2e-3 in norm for parameters (the seg-head test's); per row ROW_FLOOR, see MEASURED below.
  * tie_rows may leave out at most 2 % of the B*N rows (a condition on the inputs: it is evaluated with the fp64 oracle alone,
    on the CPU; the seeds below were picked so that every case meets it), and on a degrees graph none of the listed
    destinations (in-degree 0 ... hub) may be among them.

MEASURED (CPU ATen composition over the case lists below; the GPU ATen composition is evaluated by the tests themselves):
  * per-row statistic of the ATen composition against fp64 (kept rows): 8e-8 ... 9.3e-7, the largest at edgeconv2
    (2,3,130,40,64,train); parameters in norm 6e-8 ... 3.1e-6.  ROW_FLOOR = 5e-6: the 3x rule applied to the largest value of
    the list (a case whose own ATen error happens to be tiny is held to what the worst case of the list is allowed).  A lost or
    doubled in-edge moves a row by 1e-2 ... 1 in this statistic.
  * share of rows left out per case (edgeconv_oracle.NOISE_C = 6), in the order of CASES1, the slope-0 case, CASES2 and the
    eval case of FP32_MFMA_CASES: 0, 0, 0.0032, 0, 0, 0 | 0 | 0, 0, 0.0115, 0.0058, 0, 0.0150, 0.0039, 0, 0 | 0.
    Seeds 19 and 20 of the last two put 9 % / 8 % of their 77 / 260 rows on a near-tie; 419 and 220 were taken instead.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import edgeconv_oracle as eo
from oracle import c_api

pytestmark = pytest.mark.gpu

ROW_FLOOR = 5e-6
PARAM_FLOOR = 2e-3
MAX_LEFT_OUT = 0.02

# (B, C, N, k, Co, train, graph, seed)
CASES1 = [(2, 3, 300, 20, 64, True, "degrees", 1), (1, 64, 77, 7, 128, True, "degrees", 2), (3, 15, 513, 40, 64, False, "knn", 3),
          (2, 128, 130, 64, 256, True, "degrees", 4), (2, 3, 65, 3, 64, True, "knn", 5), (1, 3, 5, 1, 64, False, "self", 6)]
SLOPE0_CASE = (2, 3, 300, 20, 64, True, "degrees", 7)
# (B, C, N, k, C2, train, seed): the degrees graph wherever N*k holds the hub, a true kNN graph otherwise
CASES2 = [(2, 3, 300, 20, 64, True, 11), (1, 15, 77, 7, 64, True, 12), (2, 3, 130, 40, 64, True, 13), (2, 3, 257, 30, 64, True, 14),
          (1, 3, 90, 64, 64, True, 15), (2, 3, 100, 3, 64, True, 16), (3, 6, 513, 16, 64, False, 17), (2, 3, 130, 40, 128, True, 18),
          (1, 6, 77, 7, 128, False, 419)]
FP32_MFMA_CASES = [(2, 3, 300, 20, 64, True, 11), (2, 3, 130, 40, 64, False, 220)]
HUB1, HUB2 = CASES1[0], CASES2[0]


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def graph_kind2(N, k):
    return "degrees" if N * k >= sum(eo.STANDARD_DEGREES) else "knn"


def make_graph(kind, x, k, seed):
    B, _, N = x.shape
    if kind == "degrees":
        return eo.graph_with_in_degrees(B, N, k, seed=seed)
    if kind == "self":
        return torch.arange(N, dtype=torch.int32).view(1, N, 1).expand(B, N, k).contiguous()
    return T(c_api.knn_dense(x, k)[0].astype(np.int32))          # the exact kNN graph (self loop first), as functional.knn_graph builds it


def fp64_case(widths, x, layers, G, idx, train, slope):
    """the fp64 oracle on the CPU -> SimpleNamespace(out (B,Co,N), gx (B*N,C) rows, grads {name: tensor}, stats {name: tensor},
    act / pre before the max)"""
    B, C, N = x.shape
    x64 = T(x).double().requires_grad_(True)
    P = [[T(a).double().requires_grad_(i < 3) for i, a in enumerate(L)] for L in layers]
    if len(widths) == 1:
        r = eo.edgeconv1_fp64(x64, idx, *P[0], train, slope)
        stats = dict(rm1=r["rm"], rv1=r["rv"])
    else:
        r = eo.edgeconv2_fp64(x64, idx, *P[0], *P[1], train, slope)
        stats = dict(rm1=r["rm1"], rv1=r["rv1"], rm2=r["rm2"], rv2=r["rv2"])
    r["out"].backward(T(G).double().permute(0, 2, 1))
    grads = {}
    for li, L in enumerate(P, 1):
        grads.update({f"W{li}": L[0].grad, f"gamma{li}": L[1].grad, f"beta{li}": L[2].grad})
    return SimpleNamespace(out=r["out"].detach(), gx=x64.grad.transpose(1, 2).reshape(B * N, C), grads=grads, stats=stats,
                           act=r["act"].detach(), pre=r["pre"].detach())


@functools.lru_cache(maxsize=None)
def setup_case(widths, B, C, N, k, train, kind, seed, slope=0.2):
    """inputs, graph and fp64 reference of one case: computed once, shared by the tests that use it, never modified"""
    x, layers, G = eo.case_inputs(seed, B, C, N, list(widths))
    idx = make_graph(kind, x, k, seed)
    ref = fp64_case(widths, x, layers, G, idx, train, slope)
    A = ref.pre if slope == 0 else ref.act       # slope 0: every negative activation is exactly 0, ties among them are harmless
    left_out = eo.tie_rows(A, idx, eo.noise_level(A))
    return SimpleNamespace(widths=widths, B=B, C=C, N=N, k=k, train=train, kind=kind, slope=slope, x=x, layers=layers, G=G, idx=idx,
                           ref=ref, keep=~left_out, left_out=float(left_out.float().mean()))


def check_inputs(S):
    """the conditions on the inputs: at most 2 % of the rows ambiguous, none of the prescribed destinations among them"""
    assert S.left_out <= MAX_LEFT_OUT, ("near-tie rows", S.left_out)
    if S.kind == "degrees":
        deg = eo.fitted_degrees(S.N, S.k)
        assert np.array_equal(np.bincount(S.idx[0].reshape(-1).numpy(), minlength=S.N)[:len(deg)], deg)
        assert bool(S.keep[:len(deg)].all()), "a destination of the degree list is a near-tie row: choose another seed"


def run_aten(S, device):
    """the pure-ATen fp32 composition on the GPU -> (gx rows, grads)"""
    x32 = T(S.x).to(device).requires_grad_(True)
    P = [[T(a).to(device).clone().requires_grad_(i < 3) for i, a in enumerate(L)] for L in S.layers]
    r = eo.edgeconv_aten_fp32(x32, S.idx.to(device), P, S.train, S.slope)
    r["out"].backward(T(S.G).to(device).permute(0, 2, 1))
    grads = {}
    for li, L in enumerate(P, 1):
        grads.update({f"W{li}": L[0].grad, f"gamma{li}": L[1].grad, f"beta{li}": L[2].grad})
    return x32.grad.transpose(1, 2).reshape(S.B * S.N, S.C).cpu(), {n: v.cpu() for n, v in grads.items()}


def run_kernel(fsg, S, device, routes=None):
    """functional.edgeconv1 / edgeconv2 with both="twice" and a backward through the given routes: {"g": (B,Co,N) tensor,
    "pm": (B,N,Co), "pm2": (B,N,Co)} (default: the whole gradient through the channel-major tensor, as the unit tests of
    test_gpu_parity.py do) -> SimpleNamespace(out, out_pm, gx rows, grads, stats), all on the CPU"""
    from fissure_segmentation_amd.norm import BatchNorm2d
    F_hip = fsg.functional
    xt = T(S.x).to(device).requires_grad_(True)
    Ws, bns = [], []
    cin = 2 * S.C
    for (W, gamma, beta, rm, rv), width in zip(S.layers, S.widths):
        Ws.append(T(W).to(device).view(width, cin, 1, 1).clone().requires_grad_(True))
        bn = BatchNorm2d(width).to(device)
        with torch.no_grad():
            bn.weight.copy_(T(gamma)); bn.bias.copy_(T(beta)); bn.running_mean.copy_(T(rm)); bn.running_var.copy_(T(rv))
        bn.train(S.train)
        bns.append(bn)
        cin = width
    idx = S.idx.to(device)
    if len(S.widths) == 1:
        assert F_hip.edgeconv1_supported(S.widths[0], S.k)
        out, out_pm, out_pm2 = F_hip.edgeconv1(xt, idx, Ws[0], bns[0], S.slope, both="twice")
    else:
        assert F_hip.edgeconv2_supported(S.widths[0], S.widths[1], S.k)
        out, out_pm, out_pm2 = F_hip.edgeconv2(xt, idx, Ws[0], bns[0], Ws[1], bns[1], S.slope, both="twice")
    if routes is None:
        routes = {"g": T(S.G).to(device).permute(0, 2, 1).contiguous()}
    outs = {"g": out, "pm": out_pm, "pm2": out_pm2}
    torch.autograd.backward([outs[r] for r in routes], [routes[r] for r in routes])
    grads, stats = {}, {}
    for li, (W, bn) in enumerate(zip(Ws, bns), 1):
        grads.update({f"W{li}": W.grad.view(W.shape[0], -1).cpu(), f"gamma{li}": bn.weight.grad.cpu(), f"beta{li}": bn.bias.grad.cpu()})
        stats.update({f"rm{li}": bn.running_mean.detach().cpu(), f"rv{li}": bn.running_var.detach().cpu()})
    return SimpleNamespace(out=out.detach().cpu(), out_pm=out_pm.detach().cpu(), grads=grads, stats=stats,
                           gx=xt.grad.transpose(1, 2).reshape(S.B * S.N, S.C).cpu())


def gradient_errors(S, got_gx, got_grads, keep=None):
    """{name: error against fp64}: grad_x per row on the kept rows, parameters in norm (mathematically zero ones left out)"""
    errs = {"x": eo.row_error(got_gx, S.ref.gx, S.keep if keep is None else keep)}
    gmax = max(float(v.norm()) for v in S.ref.grads.values())
    for n, want in S.ref.grads.items():
        if float(want.norm()) >= 1e-6 * gmax:
            errs[n] = eo.norm_error(got_grads[n], want)
    return errs


def check_forward(S, res):
    scale = float(S.ref.out.abs().max())
    e = float((res.out.double() - S.ref.out).abs().max()) / scale
    print("\nEC", S.widths, (S.B, S.C, S.N, S.k, S.train, S.kind), "rows left out %.4f  out err/scale %.3g" % (S.left_out, e))
    assert e <= 1e-4, ("out", e)
    assert torch.equal(res.out_pm, res.out.transpose(1, 2)), "point-major output differs from the channel-major one"
    for n, want in S.ref.stats.items():
        e = float((res.stats[n].double() - want).abs().max()) / float(want.abs().max())
        assert e <= 1e-4, (n, e)


def check_gradients(S, res, aten, keep=None):
    e_k, e_a = gradient_errors(S, res.gx, res.grads, keep), gradient_errors(S, *aten, keep)
    print("   gradient errors vs fp64 (kernel, ATen fp32):", {n: ("%.2g" % e_k[n], "%.2g" % e_a[n]) for n in e_k})
    bad = {n: (e_k[n], e_a[n]) for n in e_k if e_k[n] > max(ROW_FLOOR if n == "x" else PARAM_FLOOR, 3 * e_a[n])}
    assert not bad, bad


def _check(fsg, device, S):
    check_inputs(S)
    res = run_kernel(fsg, S, device)
    check_forward(S, res)
    check_gradients(S, res, run_aten(S, device))
    return res


# ------------------------------------------------------------------------------------------------------------ (a), (b)
@pytest.mark.parametrize("B,C,N,k,Co,train,kind,seed", CASES1)
def test_edgeconv1_vs_fp64(fsg, device, B, C, N, k, Co, train, kind, seed):
    """the one-layer kernel against fp64, see the module docstring.  C = 3 / 15 / 64 / 128, Co = 64 / 128 / 256 (1, 2, 4 channel
    groups), k = 1 ... 64, ragged N, N < one tile, train / eval, degree graphs with the hub wherever N*k holds it."""
    _check(fsg, device, setup_case((Co,), B, C, N, k, train, kind, seed))


def test_edgeconv1_slope0_vs_fp64(fsg, device):
    """slope = 0 (ReLU): the near-ties are taken from the values BEFORE the activation (all negative ones are exactly 0 behind it)"""
    B, C, N, k, Co, train, kind, seed = SLOPE0_CASE
    _check(fsg, device, setup_case((Co,), B, C, N, k, train, kind, seed, 0.0))


@pytest.mark.parametrize("B,C,N,k,C2,train,seed", CASES2)
def test_edgeconv2_vs_fp64(fsg, device, B, C, N, k, C2, train, seed):
    """the two-layer kernel against fp64: both tile heights of the split kernels (k = 30: 128 rows), the 16-point cap (k = 3),
    one point per tile (k = 64), ragged last tiles, the fp32-MFMA kernels at C2 = 128"""
    _check(fsg, device, setup_case((64, C2), B, C, N, k, train, graph_kind2(N, k), seed))


@pytest.mark.parametrize("B,C,N,k,C2,train,seed", FP32_MFMA_CASES)
def test_edgeconv2_fp32_mfma_vs_fp64(fsg, device, B, C, N, k, C2, train, seed):
    """the fp32-MFMA kernels at C2 = 64 (fsg_debug_ec2_use_fp32_mfma), train and eval"""
    import ctypes
    lib = fsg._lib.lib
    lib.fsg_debug_ec2_use_fp32_mfma.argtypes = [ctypes.c_int]
    lib.fsg_debug_ec2_use_fp32_mfma.restype = None
    S = setup_case((64, C2), B, C, N, k, train, graph_kind2(N, k), seed)
    try:
        lib.fsg_debug_ec2_use_fp32_mfma(1)
        _check(fsg, device, S)
    finally:
        lib.fsg_debug_ec2_use_fp32_mfma(0)


# ------------------------------------------------------------------------------------------------------------ (c) routes
@pytest.mark.parametrize("widths", [(64,), (64, 64)])
def test_edgeconv_gradient_routes(fsg, device, monkeypatch, widths):
    """The output gradient through every route of the backward: the channel-major tensor g, the point-major g_pm, its alias
    g_pm2 (the model's route: both="twice", g = None), and g_pm as the slice [:, :, 64:128] of a (B,N,192) tensor (the gradient
    of the concatenated features; row stride 192, handed to the kernel as it is -- functional._pm_grad must not copy it).
    One G through any single route: bitwise equal gradients.  G = G1 + G2 + G3 over the three routes, two of them strided:
    held to the fp64 oracle like every other case."""
    F_hip = fsg.functional
    B, C, N, k, Co, train, kind, seed = HUB1
    S = setup_case(widths, B, C, N, k, train, kind, seed if len(widths) == 1 else HUB2[-1])
    check_inputs(S)
    Gd = T(S.G).to(device)

    def strided(g):
        big = torch.zeros(B, N, 192, device=device)
        big[:, :, 64:128] = g
        return big[:, :, 64:128]
    seen = []
    plain = F_hip._pm_grad

    def spy(g, B_, N_, C_):
        r = plain(g, B_, N_, C_)
        if g is not None:
            seen.append((g.stride(1), r[1], r[0].data_ptr() == g.data_ptr()))
        return r
    monkeypatch.setattr(F_hip, "_pm_grad", spy)
    runs = {"g": run_kernel(fsg, S, device, {"g": Gd.permute(0, 2, 1).contiguous()}),
            "pm": run_kernel(fsg, S, device, {"pm": Gd.clone()}),
            "pm2": run_kernel(fsg, S, device, {"pm2": Gd.clone()})}
    assert seen == [(Co, Co, True)] * 2, seen
    del seen[:]
    runs["pm strided"] = run_kernel(fsg, S, device, {"pm": strided(Gd)})
    assert seen == [(192, 192, True)], seen
    for name, r in runs.items():
        assert torch.equal(r.gx, runs["g"].gx), name
        for n in r.grads:
            assert torch.equal(r.grads[n], runs["g"].grads[n]), (name, n)
    # the three routes together: G1 + G2 + G3 = G up to one rounding per entry
    g = torch.Generator().manual_seed(5)
    G1, G2 = torch.randn(B, N, Co, generator=g).to(device), torch.randn(B, N, Co, generator=g).to(device)
    G3 = Gd - G1 - G2
    del seen[:]
    res = run_kernel(fsg, S, device, {"g": G1.permute(0, 2, 1).contiguous(), "pm": strided(G2), "pm2": strided(G3)})
    assert seen == [(192, 192, True)] * 2, seen
    check_forward(S, res)
    check_gradients(S, res, run_aten(S, device))


# ------------------------------------------------------------------------------------------------------------ (d) duplicates
@pytest.mark.parametrize("widths", [(64,), (64, 64)])
def test_edgeconv_duplicate_points(fsg, device, widths):
    """A cloud in which 10 % of the points are exact copies of other points (voxel-snapped keypoints), true kNN graph, k = 20:
    the arg-max ties between copies are exact, so single rows of grad_x are legitimately ambiguous -- but the SUM over each
    group of identical points is not: the gradient mass of a tie must be neither split nor duplicated.  Group sums per row
    bound (groups that contain a near-tie row between DIFFERENT positions are left out, at most 2 % of the rows)."""
    B, C, N, k, seed = 2, 3, 300, 20, 31 + len(widths)
    x, layers, G = eo.case_inputs(seed, B, C, N, list(widths))
    rng = np.random.default_rng(seed)
    group = np.tile(np.arange(N), (B, 1))
    for b in range(B):
        dup = rng.permutation(N)[:N // 10]
        src = rng.permutation(np.setdiff1d(np.arange(N), dup))[:N // 10]
        x[b][:, dup] = x[b][:, src]
        group[b, dup] = src
    idx = fsg.functional.knn_graph(T(x).to(device), k).cpu()
    ref = fp64_case(widths, x, layers, G, idx, True, 0.2)
    gid = T(group + np.arange(B)[:, None] * N).reshape(-1)                     # group id of every row
    # near-ties are judged on the graph of GROUPS (a copy and its original are one point here)
    left_out = eo.tie_rows(ref.act, torch.gather(T(group), 1, idx.long().view(B, -1)).view(B, N, k), eo.noise_level(ref.act))
    assert float(left_out.float().mean()) <= MAX_LEFT_OUT, float(left_out.float().mean())
    S = SimpleNamespace(widths=widths, B=B, C=C, N=N, k=k, train=True, kind="knn", slope=0.2, x=x, layers=layers, G=G, idx=idx,
                        ref=ref, keep=~left_out, left_out=float(left_out.float().mean()))
    res = run_kernel(fsg, S, device)
    check_forward(S, res)

    def sums(gx):
        return torch.zeros(B * N, C, dtype=gx.dtype).index_add_(0, gid, gx)
    bad_group = torch.zeros(B * N, dtype=torch.bool).index_put_((gid[left_out],), torch.tensor(True))
    keep = ~bad_group & (torch.bincount(gid, minlength=B * N) > 0)
    gx_a, grads_a = run_aten(S, device)
    S.ref = SimpleNamespace(gx=sums(ref.gx), grads=ref.grads)
    res.gx = sums(res.gx)
    check_gradients(S, res, (sums(gx_a), grads_a), keep)


# ------------------------------------------------------------------------------------------------------------ (e) reproducibility
@pytest.mark.parametrize("widths", [(64,), (64, 64)])
def test_edgeconv_hub_case_is_reproducible(fsg, device, widths):
    """two runs of the hub case give bitwise equal outputs and gradients (fixed summation order, sorted in-edges -- the hub's
    1100 in-edges are above the LDS sort capacity of the CSR builder)"""
    B, C, N, k, Co, train, kind, seed = HUB1
    S = setup_case(widths, B, C, N, k, train, kind, seed if len(widths) == 1 else HUB2[-1])
    a, b = run_kernel(fsg, S, device), run_kernel(fsg, S, device)
    assert torch.equal(a.out, b.out) and torch.equal(a.gx, b.gx)
    for n in a.grads:
        assert torch.equal(a.grads[n], b.grads[n]), n
    for n in a.stats:
        assert torch.equal(a.stats[n], b.stats[n]), n
