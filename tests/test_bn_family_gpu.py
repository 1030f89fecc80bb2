"""GPU tests of the BatchNorm-fused stages one by one against tests/bn_oracle.py (float64): fsg_bn_act_* (BatchNorm + LeakyReLU on
rows), fsg_bn_act_max_* (the same + max over the points of a cloud), fsg_bn_rows_* ([relu](BatchNorm [+ residual])) and, through
them, the shared record kernels of csrc/edgeconv.hip (bn_finalize_kernel, sum_partials_kernel) beyond their first round of
4 x 128 / 4 x 64 records; the module semantics of functional._bn_args / _bn_step / bump_bn_counter for all four fused stages.

How a value is judged: max |got - fp64| / mag, mag the sum of the absolute summands of that value (bn_oracle's `mag`), against
max(1e-6, 2 x the same figure of the fp32 ATen composition of the same operation on the GPU: norm.BatchNorm1d -> leaky_relu
[-> max] with autograd) -- FLOOR and MARGIN of tests/test_pw_family_gpu.py.  invstd and the running statistics are measured
relative to their float64 value with the floor 4 x 2^-24 of that file's bn_finalize_max lines.  Where ATen cannot run (one row
in training) the floor alone is the bar.  Every figure is printed before it is asserted (`BNFAM <case> <quantity> kernel ...
aten ...`); profiles/bn_family_parity.txt holds one run.  The inputs are generated and pinned by tests/test_bn_oracle_cpu.py
(no activation argument within KINK_MARGIN of 0, every selection above 4 x SEL_NOISE x mag), so no element is left out here.
The one value compared differently is dgamma of the gamma == 0 channel of bn_act_max, where every row of a cloud ties in the
activation: it is compared with the sum over the clouds of g f'(beta) yhat[row the kernel reports], floor alone.

MEASURED on an MI355X (profiles/bn_family_parity.txt, 306 figures, all under their bars; the largest bar is 2 x 5.2e-4, ATen's
dy of bn_act 300 x 1024).  Relative to mag, 173 of 211 figures are under the floor; the largest of a kernel is 2.5e-4 (dgamma of
bn_rows on TWO rows of 512 channels; ATen 2.5e-4 there: with two rows yhat is +-1 up to the rounding of the inputs), then dy of
bn_act_max 5 x 130 x 192 at 1.3e-4 (ATen 1.1e-4) and dy of bn_rows 1023 x 64 at 9.2e-5 (ATen 1.5e-4).  dgamma through the second
round of sum_partials_kernel: 4.8e-8 at 32769 rows, 3.9e-8 at 65665 (ATen 3.7e-7, 1.5e-7).  Furthest above ATen: dbeta of
bn_act_max 129 x 500 x 64, 1.7e-7 against 2.1e-8 (bnmax_bwd_kernel adds the 129 clouds in fp32), under the floor.  Relative
figures: the largest is invstd of bn_act_max on 2 x 3 rows, 2.8e-6 (ATen 3.1e-6).
Why the figure is a maximum over the whole tensor and not per channel: dy's mag takes |d_beta| and |d_gamma| as they are, so in
a row with a small h of a channel whose d_beta cancels, the figure is the rounding of d_beta relative to |d_beta| -- ONE random
rounding per channel, for the kernel and for ATen alike (max 5 x 130 x 192, channel 116: d_beta -8.4e-4 of summands 5.4, off by
6e-8, gives 6.5e-5 in that row).  With a bar per channel, 2 x ATen is then a coin flip: measured, 11 cases fail on dy that way
with the kernel between 2 and 3 x ATen's figure of that channel, and pass against ATen's figure of the tensor.
Two findings, both in the fp32 running sums of the bn_act kernels, which now carry them in fp64 and round once per record:
(1) dy of bn_act in a constant channel whose d_beta cancels to 2 % of sum |h| was 2.5e-6 (ATen 3.0e-7), now 5.6e-7
(bnact_bwd_reduce_kernel); (2) running_var of bn_act after two momentum=None calls on 210 rows of N(1, 2^2) was 3.62e-7 off its
fp64 value against max(2.38e-7, 2 x ATen's 1.66e-7), now 7.3e-8 (bnact_stats_kernel).
"""
import copy

import numpy as np
import pytest
import torch

import bn_oracle as bo
import pw_oracle as po

pytestmark = pytest.mark.gpu

FLOOR, MARGIN = 1e-6, 2.0          # tests/test_pw_family_gpu.py
REL_FLOOR = 4 * 2.0 ** -24         # fp64 inside, one rounding to fp32 on the way out (its bn_finalize_max lines)


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def G(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)          # a copy: the shared case inputs are read-only


def judge(name, got, aten, ref, mag, floor=FLOOR):
    """max |got - ref| / mag against max(floor, MARGIN x the ATen composition's); aten None: the floor alone.  An element without
    summands (mag == 0: d_gamma of a constant channel, dy behind gamma == 0 or behind a closed ReLU in eval mode) must equal the
    reference, which is 0 there, exactly, and takes no part in either figure: a rounding of ATen's in such an element would
    otherwise make ATen's figure, and with it the bar of the whole tensor, unbounded."""
    ref, mag = ref.to(got.device), mag.to(got.device)
    assert got.shape == ref.shape == mag.shape, (name, got.shape, ref.shape, mag.shape)
    assert bool(torch.isfinite(got).all()), name
    none = mag == 0
    assert bool((got.double()[none] == ref[none]).all()), (name, "a value without summands must be exact")
    safe = torch.where(none, torch.ones_like(mag), mag)

    def figure(x):
        return float(((x.double() - ref).abs() / safe).masked_fill(none, 0.0).max())
    e_k = figure(got)
    e_a = None if aten is None else figure(aten)
    print("BNFAM %-44s kernel %.3g  aten %s" % (name, e_k, "-" if e_a is None else "%.3g" % e_a))
    assert e_a is None or e_a < 1.0, (name, "the yardstick itself is off", e_a)
    assert e_k <= max(floor, MARGIN * (e_a or 0.0)), (name, e_k, e_a)


def judge_rel(name, got, aten, ref):
    judge(name, got, aten, ref, ref.abs(), floor=REL_FLOOR)


def make_bn(d, training, device, **kw):
    """norm.BatchNorm1d carrying the case's parameters and running statistics"""
    from fissure_segmentation_amd.norm import BatchNorm1d
    C = d["gamma"].size
    bn = BatchNorm1d(C, eps=bo.EPS, **kw).to(device)
    with torch.no_grad():
        if bn.affine:
            bn.weight.copy_(G(d["gamma"], device)); bn.bias.copy_(G(d["beta"], device))
        if bn.track_running_stats:
            bn.running_mean.copy_(G(d["rm"], device)); bn.running_var.copy_(G(d["rv"], device))
    return bn.train(training)


def step(fn, bn, leaves, g):
    """forward + backward of fn(*leaves) -> dict of everything the stage leaves behind"""
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in leaves]
    out = fn(*leaves)
    out.backward(g)
    torch.cuda.synchronize()
    r = dict(out=out.detach(), dy=leaves[0].grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
             rm=None if bn.running_mean is None else bn.running_mean.clone(),
             rv=None if bn.running_var is None else bn.running_var.clone(),
             tracked=None if bn.num_batches_tracked is None else int(bn.num_batches_tracked))
    if len(leaves) > 1 and leaves[1] is not None:
        r["dres"] = leaves[1].grad
    return r


def _stream():
    return torch.cuda.current_stream().cuda_stream


def direct_forward(fsg, stage, t, dims, slope_or_relu, device):
    """the training forward through the C entry point on copies of the running buffers -> (out, mean, invstd, arg | None)"""
    C = dims[-1]
    f32 = dict(dtype=torch.float32, device=device)
    mean, invstd = torch.full((C,), -777.0, **f32), torch.full((C,), -777.0, **f32)
    rm, rv = t["rm"].clone(), t["rv"].clone()
    ws = fsg._lib.workspace("fsg_bn_" + {"act": "act", "max": "act_max", "rows": "rows"}[stage], *dims, device=device)
    arg = None
    if stage == "act":
        out = torch.empty_like(t["y"])
        fsg._lib.call("fsg_bn_act_fwd_f32", t["y"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), rm.data_ptr(), rv.data_ptr(),
                      dims[0], C, 1, bo.MOMENTUM, bo.EPS, slope_or_relu, out.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(),
                      _stream())
    elif stage == "max":
        B, N, _ = dims
        out, ysel = torch.empty(B, C, **f32), torch.empty(B, C, **f32)
        arg = torch.full((B, C), -7, dtype=torch.int32, device=device)
        fsg._lib.call("fsg_bn_act_max_fwd_f32", t["y"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), rm.data_ptr(),
                      rv.data_ptr(), B, N, C, 1, bo.MOMENTUM, bo.EPS, slope_or_relu, out.data_ptr(), ysel.data_ptr(), arg.data_ptr(),
                      mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), _stream())
    else:
        out = torch.empty_like(t["x"])
        fsg._lib.call("fsg_bn_rows_fwd_f32", t["x"].data_ptr(), t["res"].data_ptr() if t["res"] is not None else None,
                      t["gamma"].data_ptr(), t["beta"].data_ptr(), rm.data_ptr(), rv.data_ptr(), dims[0], C, 1, bo.MOMENTUM, bo.EPS,
                      int(slope_or_relu), out.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out, mean, invstd, arg


def aten_batch_stats(rows):
    """save_mean / save_invstd of ATen's training BatchNorm on (M, C) rows"""
    _, m, r = torch.native_batch_norm(rows, None, None, None, None, True, 0.0, bo.EPS)
    return m, r


_refs = {}


def shared(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def check_common(name, got, aten, ref, d, training, device, keep_dgamma=None):
    """out, dy, dgamma, dbeta [, dres], the running statistics and the counter of one case"""
    mag = ref["mag"]
    at = (lambda k: None) if aten is None else (lambda k: aten[k])
    judge(name + " out", got["out"], at("out"), ref["out"], mag["out"])
    judge(name + " dy", got["dy"], at("dy"), ref["dy"], mag["dy"])
    k = slice(None) if keep_dgamma is None else keep_dgamma
    kc = k if keep_dgamma is None else keep_dgamma.cpu()
    judge(name + " dgamma", got["dgamma"][k], None if aten is None else aten["dgamma"][k], ref["dgamma"][kc], mag["dgamma"][kc])
    judge(name + " dbeta", got["dbeta"], at("dbeta"), ref["dbeta"], mag["dbeta"])
    if ref.get("dres") is not None:
        judge(name + " dres", got["dres"], at("dres"), ref["dres"], mag["dres"])
    if training:
        judge_rel(name + " running_mean", got["rm"], at("rm"), ref["running_mean"])
        judge_rel(name + " running_var", got["rv"], at("rv"), ref["running_var"])
    else:
        assert torch.equal(got["rm"], G(d["rm"], device)) and torch.equal(got["rv"], G(d["rv"], device))
    assert got["tracked"] == ref["num_batches_tracked"] == (1 if training else 0)


def check_saved_stats(name, mean, invstd, rows, ref, with_aten):
    am, ar = aten_batch_stats(rows) if with_aten else (None, None)
    judge(name + " mean", mean, am, ref["mean"], ref["mag"]["mean"])
    judge_rel(name + " invstd", invstd, ar, ref["invstd"])


# --------------------------------------------------------------------------------------------------------------------- the cases

@pytest.mark.parametrize("case", bo.CASES_ACT, ids=bo.case_id)
def test_bn_act_vs_fp64(fsg, device, case):
    M, C, training, slope, _ = case
    F = fsg.functional
    d = bo.act_inputs(case)
    ref = shared(("act", case), lambda: bo.act_oracle(case))
    t = {k: G(v, device) for k, v in d.items()}
    name = "act " + bo.case_id(case)
    bn, bn_a = make_bn(d, training, device), make_bn(d, training, device)
    got = step(lambda y: F.bn_act(y, bn, slope), bn, [t["y"]], t["g"])
    with_aten = not (training and M == 1)
    aten = step(lambda y: torch.nn.functional.leaky_relu(bn_a(y), slope), bn_a, [t["y"]], t["g"]) if with_aten else None
    check_common(name, got, aten, ref, d, training, device)
    if training:
        out, mean, invstd, _ = direct_forward(fsg, "act", t, (M, C), slope, device)
        assert torch.equal(out, got["out"])
        check_saved_stats(name, mean, invstd, t["y"], ref, with_aten)


@pytest.mark.parametrize("case", bo.CASES_MAX, ids=bo.case_id)
def test_bn_act_max_vs_fp64(fsg, device, case):
    B, N, C, training, _ = case
    F = fsg.functional
    d = bo.max_inputs(case)
    ref = shared(("max", case), lambda: bo.max_oracle(case))
    t = {k: G(v, device) for k, v in d.items()}
    name = "max " + bo.case_id(case)
    z = bo.ZERO_GAMMA
    keep = torch.ones(C, dtype=torch.bool)
    keep[z] = False
    bn, bn_a = make_bn(d, training, device), make_bn(d, training, device)
    got = step(lambda y: F.bn_act_max(y, bn, bo.MAX_SLOPE), bn, [t["y"]], t["g"])
    with_aten = not (training and B * N == 1)
    aten = step(lambda y: torch.nn.functional.leaky_relu(bn_a(y.view(B * N, C)), bo.MAX_SLOPE).view(B, N, C).max(dim=1)[0], bn_a,
                [t["y"]], t["g"]) if with_aten else None
    check_common(name, got, aten, ref, d, training, device, keep_dgamma=keep.to(device))
    # the gamma == 0 channel: out = f(beta), dy exactly 0, dgamma through the row the kernel reports
    beta64 = bo.T64(d["beta"])
    bz = torch.from_numpy(np.array(d["beta"]))[z]
    assert torch.equal(got["out"][:, z].cpu(), torch.where(bz > 0, bz, bz * bo.MAX_SLOPE).expand(B))
    assert bool((got["dy"][:, :, z] == 0).all())
    if training:
        out, mean, invstd, arg = direct_forward(fsg, "max", t, (B, N, C), bo.MAX_SLOPE, device)
        assert torch.equal(out, got["out"])
        check_saved_stats(name, mean, invstd, t["y"].view(B * N, C), ref, with_aten)
    else:
        f32 = dict(dtype=torch.float32, device=device)
        out, ysel, arg = torch.empty(B, C, **f32), torch.empty(B, C, **f32), torch.full((B, C), -7, dtype=torch.int32, device=device)
        mean, invstd = t["rm"].clone(), torch.rsqrt(t["rv"] + bo.EPS)
        ws = fsg._lib.workspace("fsg_bn_act_max", B, N, C, device=device)
        fsg._lib.call("fsg_bn_act_max_fwd_f32", t["y"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), None, None, B, N, C, 0,
                      0.0, bo.EPS, bo.MAX_SLOPE, out.data_ptr(), ysel.data_ptr(), arg.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                      ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert torch.equal(out, got["out"])
    arg = arg.cpu().long()
    assert bool(((arg >= 0) & (arg < N)).all())
    assert torch.equal(arg[:, keep], ref["arg"][:, keep])
    y64 = bo.T64(d["y"])[:, :, z]
    yhat = (y64.gather(1, arg[:, z][:, None]).squeeze(1) - ref["mean"][z]) * ref["invstd"][z]
    h = bo.T64(d["g"])[:, z] * po.dlrelu(beta64[z].expand(B), bo.MAX_SLOPE)
    judge(name + " dgamma[gamma == 0]", got["dgamma"][z], None, (h * yhat).sum(), (h * yhat).abs().sum())
    assert torch.equal(arg[:, z], ref["arg"][:, z])          # the contract names the row: the largest y, lowest index


@pytest.mark.parametrize("case", bo.CASES_ROWS, ids=bo.case_id)
def test_bn_rows_edges_vs_fp64(fsg, device, case):
    M, C, training, relu, has_res, _ = case
    F = fsg.functional
    d = bo.rows_inputs(case)
    ref = shared(("rows", case), lambda: bo.rows_oracle(case))
    t = {k: (G(v, device) if v is not None else None) for k, v in d.items()}
    name = "rows " + bo.case_id(case)
    bn, bn_a = make_bn(d, training, device), make_bn(d, training, device)
    got = step(lambda x, r: F.bn_rows(x, bn, relu=relu, residual=r), bn, [t["x"], t["res"]], t["g"])

    def composed(x, r):
        v = bn_a(x) if r is None else bn_a(x) + r
        return torch.relu(v) if relu else v
    with_aten = not (training and M == 1)
    aten = step(composed, bn_a, [t["x"], t["res"]], t["g"]) if with_aten else None
    check_common(name, got, aten, ref, d, training, device)
    if has_res:
        assert torch.equal(got["dres"].cpu().double(), ref["dres"])        # a masked copy of the gradient
    if training:
        out, mean, rstd, _ = direct_forward(fsg, "rows", t, (M, C), relu, device)
        assert torch.equal(out, got["out"])
        check_saved_stats(name, mean, rstd, t["x"], ref, with_aten)


@pytest.mark.parametrize("M", [1024, 1025])
def test_bn_rows_one_launch_kernels_end_at_1024_rows(fsg, device, M):
    """which path runs is visible in the workspace: the one-launch kernels (M <= 1024, forward in training and backward) keep their
    sums in registers and leave it alone, the three-launch path writes its per-workgroup records there.  (Both paths give
    correct values at 1024 rows, so parity alone does not see the switch move; the 1024-row kernel is the measured choice.)"""
    case = [c for c in bo.CASES_ROWS if c[0] == M and c[1] == 64][0]
    C = case[1]
    t = {k: G(v, device) for k, v in bo.rows_inputs(case).items() if v is not None}
    f32 = dict(dtype=torch.float32, device=device)
    out, gx = torch.empty_like(t["x"]), torch.empty_like(t["x"])
    mean, rstd, dgamma, dbeta = (torch.empty(C, **f32) for _ in range(4))
    ws = fsg._lib.workspace("fsg_bn_rows", M, C, device=device)
    for what in ("fwd", "bwd"):
        ws.fill_(0xA5)
        if what == "fwd":
            fsg._lib.call("fsg_bn_rows_fwd_f32", t["x"].data_ptr(), None, t["gamma"].data_ptr(), t["beta"].data_ptr(), None, None, M, C, 1,
                          bo.MOMENTUM, bo.EPS, 1, out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), _stream())
        else:
            fsg._lib.call("fsg_bn_rows_bwd_f32", t["g"].data_ptr(), t["x"].data_ptr(), out.data_ptr(), t["gamma"].data_ptr(),
                          mean.data_ptr(), rstd.data_ptr(), M, C, 1, 1, gx.data_ptr(), None, dgamma.data_ptr(), dbeta.data_ptr(),
                          ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        untouched = bool((ws == 0xA5).all())
        assert untouched == (M <= 1024), (what, M)


# --------------------------------------------------------------------------------------------------------------------- ties

def test_bn_act_max_exact_ties_route_to_one_row(fsg, device):
    """exact ties in the max of bn_act_max (rows n / n + 4 of one wave, n / n + 1 of two waves in both orders, rows of two tiles; at
    the maximum of the gamma > 0 channels and at the minimum of the gamma < 0 ones; eval mode): the whole gradient of a (cloud,
    channel) lands on exactly one tied row, the lowest, and every other row gets exact zeros"""
    d = bo.tie_inputs()
    B, N, C = bo.TIE_B, bo.TIE_N, bo.TIE_C
    ref = bo.bn_act_max(bo.T64(d["y"]), bo.T64(d["gamma"]), bo.T64(d["beta"]), bo.T64(d["g"]), False, bo.MAX_SLOPE, bo.T64(d["rm"]),
                        bo.T64(d["rv"]))
    bn = make_bn(d, False, device)
    got = step(lambda y: fsg.functional.bn_act_max(y, bn, bo.MAX_SLOPE), bn, [G(d["y"], device)], G(d["g"], device))
    dy = got["dy"].cpu()
    first = torch.tensor([bo.TIE_PAIRS[c % 5][0] for c in range(C)])
    second = torch.tensor([bo.TIE_PAIRS[c % 5][1] for c in range(C)])
    nz = dy != 0
    assert bool((nz.sum(1) == 1).all()), "the gradient of a (cloud, channel) must land on exactly one row"
    assert bool((nz.float().argmax(1) == first[None]).all()), "the lowest tied row"
    assert bool((dy.gather(1, second[None, None, :].expand(B, 1, C)) == 0).all())
    judge("ties out", got["out"], None, ref["out"], ref["mag"]["out"])
    judge("ties dy", got["dy"], None, ref["dy"], ref["mag"]["dy"])
    judge("ties dgamma", got["dgamma"], None, ref["dgamma"], ref["mag"]["dgamma"])
    judge("ties dbeta", got["dbeta"], None, ref["dbeta"], ref["mag"]["dbeta"])


# --------------------------------------------------------------------------------------------------------------------- conditioning

def test_bn_constant_and_shifted_channels(fsg, device):
    """the exactly constant channels and the two mean >> spread kinds (N(5, 0.05^2), N(-50, 0.5^2)) through all three stages in
    training: everything finite; a constant channel has mean == the constant exactly and invstd == 1 / sqrt(eps) to fp32 rounding.
    In the max stage every row of a constant channel ties (the oracle and the kernel take row 0, ATen any row), so there the
    constant channels are judged by the floor alone."""
    F = fsg.functional
    B, N, C = 2, 150, 64
    M = B * N
    rng = np.random.default_rng(11)
    y, gamma, beta = bo.channels("act", M, C, rng)
    rm, rv = bo.running_buffers(y, C, True, rng)
    const = np.array([bo.channel_kind(c) == bo.CONSTANT_KIND for c in range(C)])
    y, _ = bo.settle(y, gamma, beta, True, rm, rv, N=N, movable=~const)
    assert bo.kinks(y, gamma, beta, True, rm, rv) == 0
    d = dict(y=y, gamma=gamma, beta=beta, rm=rm, rv=rv)
    t = {k: G(v, device) for k, v in d.items()}
    t["x"], t["res"] = t["y"], None
    shifted = torch.tensor([bo.channel_kind(c) in (1, 2) for c in range(C)])
    cst = torch.from_numpy(const)
    e32 = float(np.float32(bo.EPS))
    for stage in ("act", "max", "rows"):
        g = rng.standard_normal((B, C) if stage == "max" else (M, C)).astype(np.float32)
        a64 = [bo.T64(v) for v in (gamma, beta, g)]
        bn, bn_a = make_bn(d, True, device), make_bn(d, True, device)
        if stage == "act":
            ref = bo.bn_act(bo.T64(y), *a64, True, 0.2, bo.T64(rm), bo.T64(rv))
            got = step(lambda v: F.bn_act(v, bn, 0.2), bn, [t["y"]], G(g, device))
            aten = step(lambda v: torch.nn.functional.leaky_relu(bn_a(v), 0.2), bn_a, [t["y"]], G(g, device))
            _, mean, invstd, _ = direct_forward(fsg, "act", t, (M, C), 0.2, device)
        elif stage == "max":
            y3 = t["y"].view(B, N, C)
            ref = bo.bn_act_max(bo.T64(y).view(B, N, C), *a64, True, 0.2, bo.T64(rm), bo.T64(rv))
            got = step(lambda v: F.bn_act_max(v, bn, 0.2), bn, [y3], G(g, device))
            aten = step(lambda v: torch.nn.functional.leaky_relu(bn_a(v.view(M, C)), 0.2).view(B, N, C).max(dim=1)[0], bn_a, [y3],
                        G(g, device))
            _, mean, invstd, arg = direct_forward(fsg, "max", t, (B, N, C), 0.2, device)
            assert bool((arg[:, cst.to(device)] == 0).all())
        else:
            ref = bo.bn_rows(bo.T64(y), None, *a64, True, True, bo.T64(rm), bo.T64(rv))
            got = step(lambda v: F.bn_rows(v, bn, relu=True), bn, [t["y"]], G(g, device))
            aten = step(lambda v: torch.relu(bn_a(v)), bn_a, [t["y"]], G(g, device))
            _, mean, invstd, _ = direct_forward(fsg, "rows", t, (M, C), True, device)
        for k in ("out", "dy", "dgamma", "dbeta", "rm", "rv"):
            assert bool(torch.isfinite(got[k]).all()), (stage, k)
        assert torch.equal(mean[cst.to(device)], t["y"][0, cst.to(device)])
        rel = (invstd[cst.to(device)].double() * e32 ** 0.5 - 1).abs().max()
        print("BNFAM cond %s invstd of the constant channels: rel %.3g" % (stage, float(rel)))
        assert float(rel) <= 2.0 ** -23
        for what, sel in (("shifted", shifted), ("constant", cst)):
            use_aten = not (stage == "max" and what == "constant")
            for k in ("out", "dy", "dgamma", "dbeta"):
                gv, av, rv_, mv = (v[..., sel.to(v.device)] for v in (got[k], aten[k], ref[k], ref["mag"][k]))
                judge("cond %s %s %s" % (stage, what, k), gv, av if use_aten else None, rv_, mv)
            judge("cond %s %s mean" % (stage, what), mean[sel.to(device)], aten_batch_stats(t["y"])[0][sel.to(device)],
                  ref["mean"][sel], ref["mag"]["mean"][sel])
            judge_rel("cond %s %s invstd" % (stage, what), invstd[sel.to(device)], aten_batch_stats(t["y"])[1][sel.to(device)],
                      ref["invstd"][sel])
            judge_rel("cond %s %s running_var" % (stage, what), got["rv"][sel.to(device)], aten["rv"][sel.to(device)],
                      ref["running_var"][sel])
            judge_rel("cond %s %s running_mean" % (stage, what), got["rm"][sel.to(device)], aten["rm"][sel.to(device)],
                      ref["running_mean"][sel])


# --------------------------------------------------------------------------------------------------------------------- module semantics

STAGES = ["bn_act", "bn_act_max", "bn_act_maxavg", "bn_rows"]


def _stage_fn(F, stage, bn):
    if stage == "bn_act":
        return lambda y: F.bn_act(y, bn, 0.2)
    if stage == "bn_act_max":
        return lambda y: F.bn_act_max(y, bn, 0.2)
    if stage == "bn_act_maxavg":
        return lambda y: F.bn_act_maxavg(y, bn, 0.2)
    return lambda y: F.bn_rows(y, bn, relu=True)


def _aten_fn(stage, bn, shape):
    lr = torch.nn.functional.leaky_relu
    if stage == "bn_act":
        return lambda y: lr(bn(y), 0.2)
    if stage == "bn_rows":
        return lambda y: torch.relu(bn(y))
    B, N, C = shape
    if stage == "bn_act_max":
        return lambda y: lr(bn(y.view(B * N, C)), 0.2).view(B, N, C).max(dim=1)[0]

    def maxavg(y):
        a = lr(bn(y.view(B * N, C)), 0.2).view(B, N, C)
        return torch.cat((a.max(dim=1)[0], a.mean(dim=1)), 1)
    return maxavg


@pytest.mark.parametrize("stage", STAGES)
def test_bn_module_semantics(fsg, device, stage):
    """what functional._bn_args / _bn_step / bump_bn_counter make of a BatchNorm1d module, for every fused stage: momentum=None
    (cumulative average over two training calls), track_running_stats=False (batch statistics in train AND eval, no buffer, the
    training-form backward), half-precision and non-contiguous inputs (bit-identical to the contiguous fp32 tensor of the same
    values), affine=False (a ValueError that says so)"""
    F = fsg.functional
    three_d = stage in ("bn_act_max", "bn_act_maxavg")
    B, N, C = 3, 70, 64
    shape = (B, N, C) if three_d else (B * N, C)
    gshape = {"bn_act_max": (B, C), "bn_act_maxavg": (B, 2 * C)}.get(stage, shape)
    rng = np.random.default_rng(STAGES.index(stage) + 40)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    gamma[::4] *= -1
    beta = rng.uniform(0.1, 1.5, C).astype(np.float32)
    # well-conditioned rows N(1, 2^2), settled like the cases (off the kinks, selections above the noise) ...
    ys = []
    for _ in range(2):
        y, _ = bo.settle((rng.standard_normal((B * N, C)) * 2 + 1).astype(np.float32), gamma, beta, True, None, None, N=N if three_d else 0)
        assert bo.kinks(y, gamma, beta, True, None, None) == 0
        ys.append(torch.from_numpy(y.reshape(shape)))
    # ... and values a half holds exactly for the bitwise comparison of the input forms
    yh = torch.from_numpy((rng.standard_normal(shape) * 2 + 1).astype(np.float16).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal(gshape).astype(np.float32))
    d = dict(gamma=gamma, beta=beta, rm=np.zeros(C, np.float32), rv=np.ones(C, np.float32))
    gam64, bet64 = bo.T64(d["gamma"]), bo.T64(d["beta"])

    def oracle(y, **kw):
        y64, g64 = y.double(), g.double()
        if stage == "bn_act":
            return bo.bn_act(y64, gam64, bet64, g64, True, 0.2, **kw)
        if stage == "bn_act_max":
            return bo.bn_act_max(y64, gam64, bet64, g64, True, 0.2, **kw)
        if stage == "bn_rows":
            return bo.bn_rows(y64, None, gam64, bet64, g64, True, True, **kw)
        return bo.bn_act_maxavg(y64, gam64, bet64, g64, True, 0.2, **kw)

    # ---- momentum=None: the cumulative average, the counter counts
    bn, bn_a = make_bn(d, True, device, momentum=None), make_bn(d, True, device, momentum=None)
    rm, rv, tracked = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), 0
    for y in ys:
        got = step(_stage_fn(F, stage, bn), bn, [y.to(device)], g.to(device))
        aten = step(_aten_fn(stage, bn_a, shape), bn_a, [y.to(device)], g.to(device))
        ref = bo.batch_stats(y.double().view(-1, C), True, rm, rv, momentum=None, tracked=tracked)
        rm, rv, tracked = ref["running_mean"], ref["running_var"], ref["num_batches_tracked"]
        bn.zero_grad(); bn_a.zero_grad()
    assert got["tracked"] == tracked == 2
    judge_rel("%s momentum=None running_mean" % stage, got["rm"], aten["rm"], rm)
    judge_rel("%s momentum=None running_var" % stage, got["rv"], aten["rv"], rv)

    # ---- track_running_stats=False: batch statistics in both modes, nothing appears, nothing is written
    runs = {}
    for training in (True, False):
        bn, bn_a = (make_bn(d, training, device, track_running_stats=False) for _ in range(2))
        runs[training] = step(_stage_fn(F, stage, bn), bn, [ys[0].to(device)], g.to(device))
        aten = step(_aten_fn(stage, bn_a, shape), bn_a, [ys[0].to(device)], g.to(device))
        assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
        assert [n for n, _ in bn.named_buffers()] == []
        ref = oracle(ys[0])
        assert ref["running_mean"] is None
        for k in ("out", "dy", "dgamma", "dbeta"):
            judge("%s untracked %s %s" % (stage, "train" if training else "eval", k), runs[training][k], aten[k], ref[k],
                  ref["mag"][k])
    for k in ("out", "dy", "dgamma", "dbeta"):        # eval without buffers IS the training computation
        assert torch.equal(runs[True][k], runs[False][k]), k

    # ---- half-precision and transposed-view inputs against the contiguous fp32 tensor of the same values
    base_bn = make_bn(d, True, device)
    variants = {}
    y32 = yh.to(device)
    perm = (1, 0) if not three_d else (0, 2, 1)
    for what, yin in (("fp32", y32), ("half", y32.half()), ("view", y32.permute(*perm).contiguous().permute(*perm))):
        bn = copy.deepcopy(base_bn)
        assert what != "view" or not yin.is_contiguous()
        variants[what] = step(_stage_fn(F, stage, bn), bn, [yin], g.to(device))
    for what in ("half", "view"):
        for k in ("out", "dgamma", "dbeta", "rm", "rv"):
            assert torch.equal(variants[what][k], variants["fp32"][k]), (what, k)
        want = variants["fp32"]["dy"]
        assert torch.equal(variants[what]["dy"].float(), want.half().float() if what == "half" else want), (what, "dy")
        assert variants[what]["out"].dtype == torch.float32

    # ---- affine=False
    bn = make_bn(d, True, device, affine=False)
    with pytest.raises(ValueError, match="affine=False"):
        _stage_fn(F, stage, bn)(y32)
    assert int(bn.num_batches_tracked) == 0


# --------------------------------------------------------------------------------------------------------------------- reproducibility

def test_bn_fused_stages_are_reproducible(fsg, device):
    """the kernels claim a fixed summation order: two runs of the largest bn_act and bn_act_max cases (514 / 516 records, the second
    round of both record kernels), forward and backward, are bitwise equal"""
    F = fsg.functional
    act = [c for c in bo.CASES_ACT if c[0] == 65665][0]
    mx = [c for c in bo.CASES_MAX if c[0] == 129][0]
    for stage, case, d in (("act", act, bo.act_inputs(act)), ("max", mx, bo.max_inputs(mx))):
        runs = []
        for _ in range(2):
            bn = make_bn(d, True, device)
            fn = (lambda y: F.bn_act(y, bn, case[3])) if stage == "act" else (lambda y: F.bn_act_max(y, bn, bo.MAX_SLOPE))
            runs.append(step(fn, bn, [G(d["y"], device)], G(d["g"], device)))
        for k in ("out", "dy", "dgamma", "dbeta", "rm", "rv"):
            assert torch.equal(runs[0][k], runs[1][k]), (stage, k)
