"""GPU tests of the fused PointTransformerLayer (csrc/pt_attn.hip: ten kernels behind functional.pt_attn, fsg_pt_attn_fwd_f32 and
fsg_pt_attn_bwd_f32) stage by stage against tests/pt_oracle.py in float64, on the case list of that file: a workgroup's second
tile (C = 32 ... 512), the edge-strided kernels beyond one pass and pt_bn_finalize_kernel beyond 64 records, nsample 1 ... 16,
grad_p == NULL (the production route), graphs with a hub / points without in-edges / a row of self loops / duplicates, eval
mode, a per-channel offset of +-30 and a saturated softmax.  tests/test_pt_oracle_cpu.py proves from the kernel's own constants
that each case reaches its path and that the judge used here can fail.

How a value is judged.  Every figure is compared with max(floor, 3 x the same figure of the fp32 ATen composition of the layer
on the GPU -- pt_oracle.pt_layer in float32 -- against the same fp64 run): the rule of tests/test_edgeconv_gpu.py.
  * out, u1, sm, dq, dk, dv, dp: per row, pt_oracle.row_error (|got_r - want_r| / (|want_r| + rms row norm)); rows are points for
    out / dq / dk / dv / dp and edges for u1 / sm.
  * the 14 parameter gradients: pt_oracle.norm_error.  In training the biases lp1_b, lw1_b, lw2_b sit in front of a BatchNorm or
    the softmax: their gradient is mathematically zero and what an fp32 run leaves is cancellation noise, judged as
    max |got - fp64| / sum |summands| (pt_oracle.zero_bias_mags).  In eval mode lp1_b and lw1_b are ordinary gradients; lw2_b
    stays a zero gradient there too (the softmax does not see a per-channel shift) and is judged as in training.
  * stats (mean and invstd of the three BatchNorms) and the running buffers: relative to their fp64 value, floor REL_FLOOR =
    4 x 2^-24 of tests/test_bn_family_gpu.py (the kernels carry those sums in double and round once).
Every figure is printed before it is asserted (`PTFAM <case> <quantity> kernel ... aten ...`); profiles/pt_family_parity.txt
holds one run.  The inputs are settled (pt_oracle.settle: no ReLU argument within KINK_MARGIN of 0 in the fp64 run, asserted
here again on the oracle run that is used), so no element is left out of any comparison.

Exact expectations: dk / dv rows of a point without in-edges are 0; with ns = 1 (softmax exactly 1) dq, dk and the gradients of
linear_w, bn1, bn2 are 0; out, u1, sm, stats, dq, every parameter gradient and the running buffers carry the same bits on a
second run (no atomics on those routes); q, k, v in three separate tensors give the bits of the packed call; eval mode leaves
the buffers and the counters alone; num_batches_tracked counts the training calls; momentum=None averages over two calls.

FLOORS: each is 3 x the largest value the statistic takes for the ATen composition over the whole case list (a case whose own
ATen error happens to be tiny is held to what the worst case of the list is allowed), measured on an MI355X:
  FWD_ROW_FLOOR   2.2e-5 = 3 x 7.41e-6, sm of c64-n300-ns16-offset        GRAD_ROW_FLOOR  2.0e-5 = 3 x 6.67e-6, dk of the same case
  DP_ROW_FLOOR    1.7e-5 = 3 x 5.63e-6, dp of the same case               PARAM_FLOOR     4.2e-5 = 3 x 1.40e-5, lp1_w of c32-n2-ns2
  ZERO_BIAS_FLOOR 3.4e-7 = 3 x 1.14e-7, lp1_b of c512-n20-ns1
The row floors are 17 ... 44 x the fp32 composition's figures on the plain cases (out 5e-7, dq / dk / dv 1.2e-6): the offset case
sets them.  Its w0 = k_j - q_i + p_r reaches +-60 in some channels on a spread of 0.15, so one fp32 rounding of w0 (4e-6) is 3e-5
of the channel's standard deviation, and every stage behind bn1 inherits that; without that case the ATen maxima are u1 3.1e-7,
sm 1.7e-6 and out 4.5e-7 (the saturated case; 9.0e-7 and 2.4e-7 at c32-n8300-ns16 without it), dq / dk / dv 1.8e-6 (saturated;
1.25e-6 without), dp 5.5e-6 (two points) and 2.4e-6 (c32-n8300-ns3).  PARAM_FLOOR comes from the two-point case (four edges,
invstd_p = 41); the plain cases reach 2.8e-6 (lw1_w of c32-n8300-ns16).  A dropped tile or hub edge misses these bars by a factor
of 100 and more (tests/test_pt_oracle_cpu.py prints it).

MEASURED on an MI355X (profiles/pt_family_parity.txt, 956 figures, all under their bars; no kernel was changed).  The largest
figure of a kernel per statistic: rows of u1 / sm / out 4.2e-6 / 4.5e-6 / 8.4e-7 (offset case; ATen 4.8e-6 / 7.4e-6 / 1.7e-6),
dq 5.9e-6 (offset; ATen 6.4e-6), dp 7.8e-6 (two points; ATen 5.5e-6), parameters 9.0e-6 (lp1_w of the two-point case; ATen
1.4e-5), zero biases 1.3e-7.  Second tile: c512-n300-ns16 has every row and parameter figure under 8e-7.  Furthest above ATen
with a figure over REL_FLOOR: lp2_b of the offset case 8.4e-7 against 1.5e-7 and bnp_g of c64-n4201-ns5 3.7e-7 against 7.7e-8,
both under PARAM_FLOOR; bn1_rm of c32-n61-ns7 2.4e-6 against 9.5e-7.  Relative
figures of a mean are large wherever the mean nearly cancels, for the kernel and ATen alike: mean_2 of the offset case 6.6e-5
against 5.5e-5, bn1_rm of c512-n300-ns16 under ATen's 1.0e-4.
Tried against the kernels themselves: with pt_b2_kernel leaving out every tile after a workgroup's first and pt_bn_finalize_kernel
stopping after 192 records, 21 of the 84 tests fail -- forward stages and both backward routes of the six multi-tile training
cases, the backward of the multi-tile eval case, the two-call average at 1051 tiles -- and the 63 others pass.
"""
import numpy as np
import pytest
import torch

import pt_oracle as po

pytestmark = pytest.mark.gpu

MARGIN = 3.0
REL_FLOOR = 4 * 2.0 ** -24         # tests/test_bn_family_gpu.py
FWD_ROW_FLOOR = 2.2e-5             # out, u1, sm rows
GRAD_ROW_FLOOR = 2.0e-5            # dq, dk, dv rows
DP_ROW_FLOOR = 1.7e-5              # dp rows: a sum of +- terms that cancels
PARAM_FLOOR = 4.2e-5               # parameter gradients in norm (must stay below 3e-3, or a dropped tile goes unnoticed)
ZERO_BIAS_FLOOR = 3.4e-7           # |gradient| / sum |summands| of a mathematically-zero (bias) gradient


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def judge(case, quantity, e_k, e_a, floor):
    print("PTFAM %-24s %-14s kernel %.3g  aten %s" % (case, quantity, e_k, "-" if e_a is None else "%.3g" % e_a))
    assert np.isfinite(e_k), (case, quantity)
    assert e_a is None or e_a < 1.0, (case, quantity, "the yardstick itself is off", e_a)
    assert e_k <= max(floor, MARGIN * (e_a or 0.0)), (case, quantity, e_k, e_a)


# ------------------------------------------------------------------------------------------------------------ running the layer
def modules(fsg, inp, device, momentum=po.MOMENTUM):
    """linear_p / linear_w in the reference's module layout, carrying the case's parameters and running buffers"""
    from fissure_segmentation_amd.norm import BatchNorm1d
    nn = torch.nn
    c = inp["c"]
    cs = c // 8
    bn = lambda L: BatchNorm1d(L, eps=po.EPS, momentum=momentum)   # noqa: E731
    lp = nn.Sequential(nn.Linear(3, 3), bn(3), nn.ReLU(inplace=True), nn.Linear(3, c))
    lw = nn.Sequential(bn(c), nn.ReLU(inplace=True), nn.Linear(c, cs), bn(cs), nn.ReLU(inplace=True), nn.Linear(cs, cs))
    mods = dict(lp1=lp[0], bnp=lp[1], lp2=lp[3], bn1=lw[0], lw1=lw[2], bn2=lw[3], lw2=lw[5])
    with torch.no_grad():
        for name, t in inp["params"].items():
            tag, kind = name.split("_")
            getattr(mods[tag], "weight" if kind in ("w", "g") else "bias").copy_(t)
        for name, t in inp["running"].items():
            tag, kind = name.split("_")
            getattr(mods[tag], "running_mean" if kind == "rm" else "running_var").copy_(t)
    lp, lw = lp.to(device).train(inp["training"]), lw.to(device).train(inp["training"])
    return lp, lw, mods


def module_state(mods):
    running = {}
    for tag in ("bnp", "bn1", "bn2"):
        running[tag + "_rm"], running[tag + "_rv"] = mods[tag].running_mean.clone(), mods[tag].running_var.clone()
    return running, [int(mods[tag].num_batches_tracked) for tag in ("bnp", "bn1", "bn2")]


def kernel_run(fsg, inp, device, grad_p, momentum=po.MOMENTUM, calls=1):
    """functional.pt_attn forward + backward -> dict(out, dp, dq, dk, dv, grads, running, tracked)"""
    lp, lw, mods = modules(fsg, inp, device, momentum)
    c = inp["c"]
    p = inp["p"].to(device).requires_grad_(grad_p)
    qkv = inp["qkv"].to(device).requires_grad_(True)
    idx = inp["idx"].to(device)
    for _ in range(calls - 1):
        with torch.no_grad():
            fsg.functional.pt_attn(p, idx, qkv, lp, lw)
    out = fsg.functional.pt_attn(p, idx, qkv, lp, lw)
    out.backward(inp["g"].to(device))
    torch.cuda.synchronize()
    grads = {}
    for name in po.PARAM_NAMES:
        tag, kind = name.split("_")
        grads[name] = getattr(mods[tag], "weight" if kind in ("w", "g") else "bias").grad
    running, tracked = module_state(mods)
    return dict(out=out.detach(), dp=p.grad, dq=qkv.grad[:, :c], dk=qkv.grad[:, c:2 * c], dv=qkv.grad[:, 2 * c:], grads=grads,
                running=running, tracked=tracked)


def _ptr(t, off=0):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def direct(fsg, inp, device, separate=False, backward=False):
    """The C entry points on copies of the running buffers.  separate: q, k, v (and dq, dk, dv) as three tensors with
    ld = ldg = c instead of slices of one (n, 3c) tensor.  -> dict(out, stats, u1, sm, running [, dq, dk, dv])"""
    import ctypes
    lib = fsg._lib
    n, ns, c, training = inp["n"], inp["ns"], inp["c"], inp["training"]
    cs = c // 8
    f32 = dict(dtype=torch.float32, device=device)
    P = {k: v.to(device) for k, v in inp["params"].items()}
    R = {k: v.to(device).clone() for k, v in inp["running"].items()}
    prm = lib.PTLayerParams()
    for name, t in P.items():
        setattr(prm, name, t.data_ptr())
    for name, t in R.items():
        setattr(prm, name, t.data_ptr() if training else None)
    prm.eps_p = prm.eps_1 = prm.eps_2 = po.EPS
    prm.mom_p = prm.mom_1 = prm.mom_2 = po.MOMENTUM if training else 0.0
    p, idx, g = inp["p"].to(device), inp["idx"].to(device), inp["g"].to(device)
    qkv = inp["qkv"].to(device)
    if separate:
        q, k, v = (qkv[:, i * c:(i + 1) * c].contiguous() for i in range(3))
        ptrs, ld = (_ptr(q), _ptr(k), _ptr(v)), c
    else:
        ptrs, ld = (_ptr(qkv), _ptr(qkv, c), _ptr(qkv, 2 * c)), 3 * c
    if training:
        stats = torch.full((2 * (3 + c + cs),), -777.0, **f32)
    else:
        stats = torch.cat([t for tag in ("bnp", "bn1", "bn2") for t in (R[tag + "_rm"], torch.rsqrt(R[tag + "_rv"] + po.EPS))])
    out, u1, sm = torch.empty(n, c, **f32), torch.empty(n, ns, cs, **f32), torch.empty(n, ns, cs, **f32)
    ws = lib.workspace("fsg_pt_attn", n, ns, c, device=device)
    stream = torch.cuda.current_stream().cuda_stream
    lib.call("fsg_pt_attn_fwd_f32", _ptr(p), _ptr(idx), *ptrs, ld, ctypes.byref(prm), n, ns, c, int(training), _ptr(out),
             _ptr(stats), _ptr(u1), _ptr(sm), _ptr(ws), stream)
    r = dict(out=out, stats=stats, u1=u1, sm=sm, running=R)
    if backward:
        gs = lib.PTLayerGrads()
        r["grads"] = {k: torch.empty_like(t) for k, t in P.items()}
        for name, t in r["grads"].items():
            setattr(gs, name, t.data_ptr())
        if separate:
            dq, dk, dv = (torch.zeros(n, c, **f32) for _ in range(3))
            dptrs, ldg = (_ptr(dq), _ptr(dk), _ptr(dv)), c
        else:
            dqkv = torch.zeros(n, 3 * c, **f32)
            dq, dk, dv = dqkv[:, :c], dqkv[:, c:2 * c], dqkv[:, 2 * c:]
            dptrs, ldg = (_ptr(dqkv), _ptr(dqkv, c), _ptr(dqkv, 2 * c)), 3 * c
        lib.call("fsg_pt_attn_bwd_f32", _ptr(p), _ptr(idx), *ptrs, ld, ctypes.byref(prm), n, ns, c, int(training), _ptr(g),
                 _ptr(stats), _ptr(u1), _ptr(sm), *dptrs, ldg, None, ctypes.byref(gs), _ptr(ws), stream)
        r.update(dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return r


_refs = {}


def shared(case, device):
    """the settled inputs, the fp64 oracle run and the fp32 ATen composition's run of a case, computed once and left unchanged"""
    if case[0] not in _refs:
        inp, _ = po.case_inputs(case, device)
        r64, g64 = po.run(inp, torch.float64, device, keep_grads=True)
        assert po.kinks(r64) == 0, (case[0], "the inputs are not settled")
        r32, g32 = po.run(inp, torch.float32, device)
        keep = ("out", "u1", "sm", "stats", "bnp_rm", "bnp_rv", "bn1_rm", "bn1_rv", "bn2_rm", "bn2_rv")
        mags = po.zero_bias_mags(r64, inp["training"])
        perr_aten = po.param_errors(g32, g64, mags)
        det = lambda r: {k: ([t.detach() for t in r[k]] if k == "stats" else r[k].detach()) for k in keep}   # noqa: E731
        _refs[case[0]] = dict(inp=inp, r64=det(r64), r32=det(r32), g64=g64, g32=g32, mags=mags, perr_aten=perr_aten,
                              dp_mag=po.dp_mags(r64, inp["idx"]))
    return _refs[case[0]]


STAT_NAMES = ("mean_p", "invstd_p", "mean_1", "invstd_1", "mean_2", "invstd_2")
RUNNING = ("bnp_rm", "bnp_rv", "bn1_rm", "bn1_rv", "bn2_rm", "bn2_rv")


def split_stats(stats, c):
    cs = c // 8
    return torch.split(stats, [3, 3, c, c, cs, cs])


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", po.CASES, ids=po.case_id)
def test_pt_forward_stages_vs_fp64(fsg, device, case):
    s = shared(case, device)
    inp, r64, r32 = s["inp"], s["r64"], s["r32"]
    name, c, n, ns, training = case[:5]
    cs = c // 8
    k = direct(fsg, inp, device)
    if training:
        for nm, got, a, w in zip(STAT_NAMES, split_stats(k["stats"], c), r32["stats"], r64["stats"]):
            judge(name, nm, po.rel_error(got, w), po.rel_error(a, w), REL_FLOOR)
        for nm in RUNNING:
            judge(name, nm, po.rel_error(k["running"][nm], r64[nm]), po.rel_error(r32[nm], r64[nm]), REL_FLOOR)
    else:
        for nm in RUNNING:
            assert torch.equal(k["running"][nm], inp["running"][nm].to(device)), nm
    judge(name, "u1", po.row_error(k["u1"].view(n * ns, cs), r64["u1"]), po.row_error(r32["u1"], r64["u1"]), FWD_ROW_FLOOR)
    sm64 = r64["sm"].reshape(n * ns, cs)
    judge(name, "sm", po.row_error(k["sm"].view(n * ns, cs), sm64), po.row_error(r32["sm"].reshape(n * ns, cs), sm64), FWD_ROW_FLOOR)
    judge(name, "out", po.row_error(k["out"], r64["out"]), po.row_error(r32["out"], r64["out"]), FWD_ROW_FLOOR)
    # the module route: the same bits, the buffers moved the same way (or left alone), the counters
    m = kernel_run(fsg, inp, device, grad_p=False)
    assert torch.equal(m["out"], k["out"])
    for nm in RUNNING:
        assert torch.equal(m["running"][nm], k["running"][nm]), nm
    assert m["tracked"] == [1 if training else 0] * 3


@pytest.mark.parametrize("name", ["c128-n50-ns15", "c128-n2101-ns8"])
def test_pt_cumulative_average_over_two_calls(fsg, device, name):
    """momentum=None: the running buffers are the average of the (identical) statistics of two calls"""
    case = po.CASE_BY_NAME[name]
    inp = shared(case, device)["inp"]
    m = kernel_run(fsg, inp, device, grad_p=False, momentum=None, calls=2)
    assert m["tracked"] == [2, 2, 2]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        run = inp
        for mom in (1.0, 0.5):
            with torch.no_grad():
                r = po.pt_layer(run["p"].to(device), run["idx"].to(device), run["qkv"].to(device),
                                {k: v.to(device) for k, v in run["params"].items()},
                                {k: v.to(device) for k, v in run["running"].items()}, True, dtype, momentum=mom)
            run = dict(run, running={k: r[k] for k in RUNNING})
        ref[dtype] = run["running"]
    for nm in RUNNING:
        judge(name + "-cma", nm, po.rel_error(m["running"][nm], ref[torch.float64][nm]),
              po.rel_error(ref[torch.float32][nm], ref[torch.float64][nm]), REL_FLOOR)


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("grad_p", [True, False], ids=["dp", "nodp"])
@pytest.mark.parametrize("case", po.CASES, ids=po.case_id)
def test_pt_backward_vs_fp64(fsg, device, case, grad_p):
    s = shared(case, device)
    inp, g64, g32 = s["inp"], s["g64"], s["g32"]
    name, c, n, ns, training = case[:5]
    tag = name + ("" if grad_p else "-nodp")
    k = kernel_run(fsg, inp, device, grad_p)
    assert (k["dp"] is not None) == grad_p
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * c, (i + 1) * c)
        judge(tag, nm, po.row_error(k[nm], g64["qkv"][:, sl]), po.row_error(g32["qkv"][:, sl], g64["qkv"][:, sl]), GRAD_ROW_FLOOR)
    if grad_p and n == 1:   # every d is 0 and dp cancels to exactly 0 in the oracle: held against the summands, as the zero biases are
        fig = lambda t: float(((t.double() - g64["p"]).abs().sum(1) / s["dp_mag"]).max())   # noqa: E731
        judge(tag, "dp/summands", fig(k["dp"]), fig(g32["p"]), ZERO_BIAS_FLOOR)
    elif grad_p:
        judge(tag, "dp", po.row_error(k["dp"], g64["p"]), po.row_error(g32["p"], g64["p"]), DP_ROW_FLOOR)
    exact_zero = ("lw1_w", "lw1_b", "lw2_w", "lw2_b", "bn1_g", "bn1_b", "bn2_g", "bn2_b") if ns == 1 else ()
    e_k = po.param_errors(k["grads"], g64, s["mags"])
    for nm in po.PARAM_NAMES:
        if nm in exact_zero:
            assert bool((k["grads"][nm] == 0).all()), (tag, nm)
        else:
            judge(tag, nm, e_k[nm], s["perr_aten"][nm], ZERO_BIAS_FLOOR if nm in s["mags"] else PARAM_FLOOR)
    if ns == 1:
        assert bool((k["dq"] == 0).all()) and bool((k["dk"] == 0).all())
    lonely = torch.from_numpy(po.in_degree(inp["idx"], n) == 0).to(device)
    if case[5] == "noself":
        assert int(lonely.sum()) >= po.LONELY
    assert bool((k["dk"][lonely] == 0).all()) and bool((k["dv"][lonely] == 0).all())


# ------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("case", po.CASES, ids=po.case_id)
def test_pt_second_run_same_bits(fsg, device, case):
    """no atomics on the routes of out, u1, sm, stats, dq, the parameter gradients and the running buffers"""
    inp = shared(case, device)["inp"]
    a, b = (direct(fsg, inp, device, backward=True) for _ in range(2))
    for nm in ("out", "u1", "sm", "stats", "dq"):
        assert torch.equal(a[nm], b[nm]), nm
    for nm in po.PARAM_NAMES:
        assert torch.equal(a["grads"][nm], b["grads"][nm]), nm
    for nm in RUNNING:
        assert torch.equal(a["running"][nm], b["running"][nm]), nm


@pytest.mark.parametrize("name", ["c64-n4201-ns5", "c512-n300-ns16"])
def test_pt_separate_qkv_same_bits_as_packed(fsg, device, name):
    inp = shared(po.CASE_BY_NAME[name], device)["inp"]
    a, b = direct(fsg, inp, device, backward=True), direct(fsg, inp, device, separate=True, backward=True)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dq"], b["dq"])
    for nm in ("dk", "dv"):
        assert po.row_error(b[nm], a[nm]) <= GRAD_ROW_FLOOR, nm
