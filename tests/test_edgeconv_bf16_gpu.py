"""GPU tests of the two-layer EdgeConv in bf16 operand mode (csrc/edgeconv2.hip: fsg_edgeconv2_{fwd,bwd}_bf16 -- the NP = 1 split
kernels ec2s_{fwd,bwd}_kernel<1,2|4> and the fp32-MFMA kernels with BF = true) against the fp64 rounded-operand model of
tests/edgeconv_bf16_oracle.py, stage by stage.  _EdgeConv2.apply is driven with pq as the leaf under mfma_operands("bf16").

Forward, per element:  |ysel2 - y2_oracle at the KERNEL's slot| <= T_flip + max(F_FWD, 3 A) mag,  mag = sum_c |rnd z1| |rnd W2|,
A = the largest error / mag of the fp32 yardstick on that case over the elements with T_flip = 0.  The kernel's slot must be a
valid arg-max: the oracle's value there lies within the two elements' bounds of the oracle's best.  mean, 1/std and the running
statistics of both BatchNorms: relative to fp64 (means: to the rms of the channel, the size of the summed terms),
max(REL_FLOOR, 3 x yardstick), layer 2 plus what the mean T_flip of the channel can move them by.  out / out_pm: the bound of
ysel2 scaled by |a2|, plus the bars of the statistics they are normalised with and four fp32 roundings of the summed terms.
Backward, routing (slot, sign of u2) taken from the kernel:  grad_pq per row (edgeconv_oracle.row_error), grad_w2, dgamma1,
dbeta1, dgamma2, dbeta2 in norm (norm_error), each <= max(floor, 3 x the same figure of the fp32 yardstick under the same routing
against fp64).  In addition the MEDIAN over the rows of the same per-row figure of grad_pq ("pq_median"), same rule: the few rows
that a single re-rounded operand moves (below) do not reach it, so it is held 400 times tighter than the largest row.  Exact: dbeta2 = sum h to fp32 summation (21 roundings at the size of sum |h|: 16 + 3 additions of the partial
sums, the product, the result), the P half of grad_pq of a point without in-edges is 0, a second run gives the same bits.

MEASURED on an MI355X (profiles/edgeconv_bf16_parity.txt holds the run; every figure under its bar).  All of these rest on GPU
measurements -- the yardstick is evaluated on the GPU by these tests; the CPU stand-in of tests/test_edgeconv_bf16_oracle_cpu.py
gave the same forward figure (A 7e-8 ... 2.3e-7) and backward figures within 3 x of the GPU's:
  * forward: A = 7.3e-8 ... 2.5e-7 (the kernels: 6.5e-8 ... 1.4e-7), F_FWD = 7.5e-7 = 3 x the largest; 0.08 ... 0.13 % of the z1
    operands are ambiguous at C_Z = 6, no operand of the yardstick's outside that set rounds the other way, C_Z did not have to
    rise.  The kernel's slot was the oracle's in every entry (gap 0).
  * backward, largest yardstick figure of the list -> floor = 3 x:       C2 = 64 (nine cases)        C2 = 128 (three cases)
        grad_pq per row                                                  5.0e-4 -> 1.5e-3            5.5e-4 -> 1.7e-3
        grad_pq, median row                                              1.15e-6 -> 3.5e-6           2.43e-6 -> 7.3e-6
        grad_w2                                                          5.7e-5 -> 1.7e-4            7.9e-5 -> 2.4e-4
        dgamma1                                                          3.9e-5 -> 1.2e-4            5.1e-5 -> 1.6e-4
        dbeta1                                                           8.1e-5 -> 2.5e-4            1.1e-4 -> 3.5e-4
        dgamma2                                                          1.8e-5 -> 5.6e-5            4.5e-5 -> 1.4e-4
        dbeta2                                                           1.1e-7 -> 3.5e-7            1.1e-7 -> 3.3e-7
    The kernels' figures are of the yardstick's size, between a tenth of it and 2.8 x (64x61-k20: rows 1.39e-3 against 5.0e-4, the
    figure of the CPU stand-in on that case; bar 1.5e-3).
The yardstick's figures are not summation noise: they are set by single operands that IT rounds the other way than the oracle (a
z1 or dy2 operand within fp32 noise of a bf16 midpoint moves by 2^-8 relative).  One such dy2 operand moves a row of grad_pq with
few in-edges by up to 2^-8 / sqrt(selected entries of the row): the row floors are ten times the parameter floors, and the eval
cases, where dy2 = a2 h has no summed part, sit at 5e-8 ... 1.2e-7.  What that costs, from the CPU stand-in of the mutants
(tests/test_edgeconv_bf16_oracle_cpu.py::test_floors_against_mutants, MISSED there): the LARGEST-row judge of grad_pq does not
see the arithmetic mutants (they reach 9e-4 ... 4e-3 per row, half of that is not above 1.5e-3 / 1.7e-3) -- it is there for lost or
doubled edges (1e-2 ... 0.2).  The median row does see every one of them (4.6e-5 ... 2e-3 against 3.5e-6 / 7.3e-6; the kernels:
2.9e-8 ... 2.5e-6, at or below the yardstick's in every case but 64x61-k20 and 2x130-k40-c128, 1.5 x and 1.04 x), and so do
the forward bound (z1 / W2 mutants: 1.6e-3 ... 4.6e-3 against 7.5e-7) and grad_w2 / dgamma1 / dbeta1 (dy2 mutants: 1.5e-3 ...
8e-3 against 1.2e-4 ... 3.5e-4); nothing moves dbeta2, which is held to sum h instead.

MUTANT RUN (once, not committed): this file against a library with two arithmetic-only changes in csrc/edgeconv2.hip -- the dy2
packing of ec2s_bwd_kernel<1,*> truncating instead of rounding to nearest even, and the W2 fragments of ec2s_fwd_kernel<1,*>
truncated (a bf16 MFMA operand cannot be left unrounded; truncation is the arithmetic-only stand-in).  22 of the 62 tests failed:
test_forward_vs_rounded_fp64 of all eight split cases (ysel2 error / mag 3.7e-3 ... 4e-3 against 7.5e-7),
test_statistics_vs_rounded_fp64 of the six train-mode split cases, test_backward_vs_rounded_fp64 of all eight split cases
(2x300-k20: grad_w2 8.1e-3, dgamma1 3.2e-3, dbeta1 1.4e-2, dgamma2 2.0e-3, rows 2.4e-3; the eval case 2x77-k25, where only
the dy2 mutant acts on them: grad_w2 3.8e-3, dgamma1 3.8e-3, dbeta1 3.5e-3, rows 3.4e-3; the median row of the eight cases
9.1e-4 ... 2.2e-3 against 3.5e-6).  The four fp32-MFMA cases, whose kernels
were not touched, the input conditions, the bit-reproducibility and the edge-gather tests passed.
"""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import edgeconv_bf16_oracle as bo
import edgeconv_oracle as eo

pytestmark = pytest.mark.gpu

REL_FLOOR = 4 * 2.0 ** -24         # tests/test_bn_family_gpu.py
MARGIN = 3.0
F_FWD = 7.5e-7                       # 3 x the largest A of the list; must stay below 1e-5 (one operand rounded the wrong way: 3e-5)
# 3 x the largest yardstick figure per quantity: {C2: {quantity: floor}}
FLOORS = {64: dict(pq=1.5e-3, pq_median=3.5e-6, W2=1.7e-4, gamma1=1.2e-4, beta1=2.5e-4, gamma2=5.6e-5, beta2=3.5e-7),
          128: dict(pq=1.7e-3, pq_median=7.3e-6, W2=2.4e-4, gamma1=1.6e-4, beta1=3.5e-4, gamma2=1.4e-4, beta2=3.3e-7)}
QUANTITIES = ("pq", "pq_median") + bo.GRADS


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def run_kernel(fsg, inp, device):
    """_EdgeConv2.apply on the case's inputs in bf16 operand mode, gradient through the channel-major output -> everything the
    kernels leave behind (on the device)"""
    F_hip = fsg.functional
    lib = fsg._lib.lib
    lib.fsg_debug_ec2_use_fp32_mfma.argtypes = [ctypes.c_int]
    lib.fsg_debug_ec2_use_fp32_mfma.restype = None
    d = lambda t: t.to(device).clone()   # noqa: E731
    pq, W2 = d(inp.pq).requires_grad_(True), d(inp.W2).requires_grad_(True)
    g1, b1, rm1, rv1 = [d(t) for t in inp.bn1]
    g2, b2, rm2, rv2 = [d(t) for t in inp.bn2]
    for t in (g1, b1, g2, b2):
        t.requires_grad_(True)
    G = inp.G.to(device)
    try:
        if inp.case[6]:
            lib.fsg_debug_ec2_use_fp32_mfma(1)
        with F_hip.mfma_operands("bf16"):
            out, out_pm, _ = F_hip._EdgeConv2.apply(pq, inp.idx.to(device), W2, g1, b1, rm1, rv1, g2, b2, rm2, rv2, inp.train,
                                                    0.1, 0.1, 1e-5, 1e-5, 0.2)
            assert out.grad_fn.bf16 is True
            saved = out.grad_fn.saved_tensors
            mean1, invstd1, mean2, invstd2, ysel2, arg2 = saved[5], saved[6], saved[10], saved[11], saved[12], saved[13]
            # the sign of u2 at the selected slot as the backward will see it: from the kernel's own fp32 tensors, evaluated in
            # fp64.  Where that is a matter of rounding (|u2| within 2^-20 of the summed terms) the output gradient is set to
            # zero: h = 0 there whichever slope the kernel takes.
            with torch.no_grad():
                t = g2.double() * ((ysel2.double() - mean2.double()) * invstd2.double())
                u2 = t + b2.double()
                unsure = u2.abs() <= 2.0 ** -20 * (t.abs() + b2.double().abs())
                G = G.masked_fill(unsure, 0.0)
            out.backward(G.permute(0, 2, 1).contiguous())
        torch.cuda.synchronize()
    finally:
        lib.fsg_debug_ec2_use_fp32_mfma(0)
    return SimpleNamespace(out=out.detach(), out_pm=out_pm.detach(), ysel2=ysel2, arg2=arg2, mean1=mean1, invstd1=invstd1,
                           mean2=mean2, invstd2=invstd2, rm1=rm1, rv1=rv1, rm2=rm2, rv2=rv2, G=G, pos=u2 > 0, unsure=int(unsure.sum()),
                           grads=dict(pq=pq.grad, W2=W2.grad, gamma1=g1.grad, beta1=b1.grad, gamma2=g2.grad, beta2=b2.grad))


_STATE = {}


def state(fsg, device, case):
    """kernel (two runs), fp64 oracle and fp32 yardstick of a case: computed once, shared by the tests, never modified"""
    if case in _STATE:
        return _STATE[case]
    inp = bo.case_inputs(case)
    k1, k2 = run_kernel(fsg, inp, device), run_kernel(fsg, inp, device)
    with torch.no_grad():
        slot, pos = k1.arg2.long(), k1.pos
        used = SimpleNamespace(**{**vars(inp), "G": k1.G.cpu()})       # the output gradient as the kernel received it
        f64, g64 = bo.run(used, torch.float64, device, slot, pos)
        f32, g32 = bo.run(used, torch.float32, device, slot, pos)
        amb = bo.ambiguous(f64)
        tf = bo.t_flip(f64, amb)
        rel = (f32.y2.double() - f64.y2).abs() / f64.mag
        A = float(rel[tf == 0].max())
        bound = tf + max(F_FWD, MARGIN * A) * f64.mag
    S = SimpleNamespace(case=case, name=bo.case_id(case), inp=inp, k1=k1, k2=k2, slot=slot, pos=pos, f64=f64,
                        g64=g64, f32=f32, g32=g32, amb=amb, tf=tf, A=A, bound=bound)
    _STATE[case] = S
    return S


def show(S, quantity, kernel, aten, bar=None):
    print("EC2BF %-28s %-12s kernel %.3g  aten %s%s" % (S.name, quantity, kernel, "-" if aten is None else "%.3g" % aten,
                                                       "" if bar is None else "  bar %.3g" % bar))


@pytest.mark.parametrize("case", bo.CASES, ids=bo.case_id)
def test_inputs(fsg, device, case):
    """the conditions on the inputs, on the GPU's own fp64 / fp32 evaluations: every z1 operand the yardstick rounds the other way
    is in the ambiguous set, which holds at most 1 % of the operands; at most 2 % of the rows on the kink of layer 2; the sign of
    u2 at the kernel's slot is a matter of rounding in at most 8 entries (their output gradient is zeroed)"""
    S = state(fsg, device, case)
    differs = S.f32.zr.double() != S.f64.zr
    share = float(S.amb.float().mean())
    kink = float(bo.kink_rows(S.f64, bo.at_slot(S.bound, S.f64.slot)).float().mean())
    show(S, "ambiguous z1", share, float(differs.float().mean()))
    show(S, "kink rows", kink, None)
    show(S, "unsure u2 signs", S.k1.unsure, None)
    assert torch.equal(S.f64.zr, S.f64.zr.float().bfloat16().double())            # the oracle's operands are bf16 values to the bit
    assert not bool((differs & ~S.amb).any())
    assert share <= bo.MAX_AMBIGUOUS and kink <= bo.MAX_LEFT_OUT
    assert S.k1.unsure <= 8


@pytest.mark.parametrize("case", bo.CASES, ids=bo.case_id)
def test_forward_vs_rounded_fp64(fsg, device, case):
    """ysel2 per element at the kernel's slot, the slot a valid arg-max, out / out_pm: see the module docstring"""
    S = state(fsg, device, case)
    f, k = S.f64, S.k1
    want, bnd, mag = bo.at_slot(f.y2, S.slot), bo.at_slot(S.bound, S.slot), bo.at_slot(f.mag, S.slot)
    err = (k.ysel2.double() - want).abs()
    settled = bo.at_slot(S.tf, S.slot) == 0
    show(S, "ysel2 err/mag", float((err / mag)[settled].max()), S.A, max(F_FWD, MARGIN * S.A))
    show(S, "ysel2 err/bound", float((err / bnd).max()), None, 1.0)
    assert max(F_FWD, MARGIN * S.A) < 1e-5, ("the bound no longer sees a single operand rounded the wrong way", S.A)
    assert bool((err <= bnd).all()), float((err / bnd).max())
    # a valid arg-max: within the two elements' bounds of the oracle's best
    v = f.y2 * f.sgn
    gap = bo.at_slot(v, f.slot) - bo.at_slot(v, S.slot)
    room = bo.at_slot(S.bound, f.slot) + bnd
    show(S, "slot gap/room", float((gap / room).max()), None, 1.0)
    assert bool((gap <= room).all())
    assert int(S.slot.max()) < case[2]
    # out / out_pm
    a2 = (f.g2 * f.r2).abs()
    bars = stat_bars(S)
    u2 = (want - f.mu2) * f.r2 * f.g2 + f.b2
    terms = (a2 * want).abs() + (a2 * f.mu2).abs() + f.b2.abs()
    bnd_out = a2 * (bnd + bars["mean2"][2]) + (u2 - f.b2).abs() * bars["invstd2"][2] / f.r2 + 4 * 2.0 ** -24 * terms
    e_out = (k.out_pm.double() - torch.nn.functional.leaky_relu(u2, 0.2)).abs()
    show(S, "out err/bound", float((e_out / bnd_out).max()), None, 1.0)
    assert bool((e_out <= bnd_out).all())
    assert torch.equal(k.out, k.out_pm.transpose(1, 2))


def stat_bars(S):
    """{name: (kernel value, fp64 value, absolute bar per channel, yardstick error per channel)} of the BatchNorm statistics"""
    f, y, k, m = S.f64, S.f32, S.k1, 0.1
    train = S.inp.train
    meanT = S.tf.mean((0, 1, 2)) if train else torch.zeros_like(f.mu2)
    std2 = 1.0 / f.r2
    rms1 = (1.0 / f.r1 ** 2 + f.mu1 ** 2).sqrt()
    rms2 = (std2 ** 2 + f.mu2 ** 2).sqrt()
    rm1_0, rm2_0 = S.inp.bn1[2].to(f.mu1.device).double(), S.inp.bn2[2].to(f.mu1.device).double()
    spec = dict(mean1=(k.mean1, f.mu1, y.mu1, rms1, 0), invstd1=(k.invstd1, f.r1, y.r1, f.r1, 0),
                rm1=(k.rm1, f.rm1, y.rm1, (1 - m) * rm1_0.abs() + m * rms1, 0), rv1=(k.rv1, f.rv1, y.rv1, f.rv1, 0),
                mean2=(k.mean2, f.mu2, y.mu2, rms2, meanT), invstd2=(k.invstd2, f.r2, y.r2, f.r2, f.r2 * meanT / std2),
                rm2=(k.rm2, f.rm2, y.rm2, (1 - m) * rm2_0.abs() + m * rms2, m * meanT),
                rv2=(k.rv2, f.rv2, y.rv2, f.rv2, 2 * m * meanT * std2 * (S.f64.y2[..., 0].numel() / max(S.f64.y2[..., 0].numel() - 1, 1))))
    bars = {}
    for name, (got, want, aten, mag, flip) in spec.items():
        e_a = (aten.double() - want).abs() / mag
        bars[name] = (got, want, torch.clamp(MARGIN * e_a.max(), min=REL_FLOOR) * mag + flip, e_a, mag)
    return bars


@pytest.mark.parametrize("case", bo.CASES, ids=bo.case_id)
def test_statistics_vs_rounded_fp64(fsg, device, case):
    """mean / 1/std as the backward reads them and the running statistics of both BatchNorms (eval: the running statistics
    themselves, untouched to the bit)"""
    S = state(fsg, device, case)
    bad = []
    for name, (got, want, bar, e_a, mag) in stat_bars(S).items():
        err = (got.double() - want).abs()
        show(S, name, float((err / mag).max()), float(e_a.max()), float((bar / mag).max()))
        if not bool((err <= bar).all()):
            bad.append(name)
    assert not bad, bad
    if not S.inp.train:
        d = S.k1.rm1.device
        assert torch.equal(S.k1.rm1, S.inp.bn1[2].to(d)) and torch.equal(S.k1.rv1, S.inp.bn1[3].to(d))
        assert torch.equal(S.k1.rm2, S.inp.bn2[2].to(d)) and torch.equal(S.k1.rv2, S.inp.bn2[3].to(d))


def gradient_errors(g, g64):
    rows = bo.row_errors(g["pq"], g64["pq"])
    e = {"pq": float(rows.max()), "pq_median": float(rows.median())}
    e.update({n: eo.norm_error(g[n], g64[n]) for n in bo.GRADS})
    return e


@pytest.mark.parametrize("case", bo.CASES, ids=bo.case_id)
def test_backward_vs_rounded_fp64(fsg, device, case):
    """every gradient under the kernel's routing, dbeta2 against sum h, points without in-edges: see the module docstring"""
    S = state(fsg, device, case)
    e_k, e_a = gradient_errors(S.k1.grads, S.g64), gradient_errors(S.g32, S.g64)
    floors = FLOORS[case[3]]
    bad = {}
    for q in QUANTITIES:
        bar = max(floors[q], MARGIN * e_a[q])
        show(S, "grad " + q, e_k[q], e_a[q], bar)
        if not e_k[q] <= bar:
            bad[q] = (e_k[q], e_a[q])
    assert not bad, bad
    # dbeta2 = sum h, to fp32 summation
    h = S.k1.G * torch.where(S.pos, 1.0, 0.2).float()
    e = (S.k1.grads["beta2"].double() - h.double().sum((0, 1))).abs() / h.double().abs().sum((0, 1))
    show(S, "dbeta2 vs sum h", float(e.max()), None, 21 * 2.0 ** -24)
    assert float(e.max()) <= 21 * 2.0 ** -24
    # a point without in-edges receives nothing through P
    deg = torch.bincount(S.f64.flat, minlength=S.inp.B * S.inp.N)
    lonely = deg == 0
    if bo.graph_kind(case[1], case[2]) == "degrees":
        assert bool(lonely[0])
    assert bool((S.k1.grads["pq"].reshape(-1, 128)[lonely][:, :64] == 0).all())
    if bool(lonely.any()):
        assert bool((S.k1.grads["pq"].reshape(-1, 128)[lonely][:, 64:] != 0).any())


@pytest.mark.parametrize("case", bo.CASES, ids=bo.case_id)
def test_second_run_same_bits(fsg, device, case):
    """everything the forward and the backward leave behind, bit for bit"""
    S = state(fsg, device, case)
    a, b = S.k1, S.k2
    for n in ("out", "out_pm", "ysel2", "arg2", "mean1", "invstd1", "mean2", "invstd2", "rm1", "rv1", "rm2", "rv2"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    for n in a.grads:
        assert torch.equal(a.grads[n], b.grads[n]), n


# ------------------------------------------------------------------------------------------------------------ edge gather, bf16
@pytest.mark.parametrize("B,C,N,k,kind", [(2, 16, 300, 12, "random"), (2, 5, 300, 20, "degrees")])   # C = 5: a ragged channel chunk
def test_edge_gather_bf16_backward_vs_fp64_sum(fsg, device, B, C, N, k, kind):
    """fsg_edge_gather_bwd_bf16 against the fp64 sum of the bf16 gradient values it reads (hub of 1100 in-edges included):
    |got - want| <= 1/2 ulp_bf16(want) + 2^-20 sum |terms| -- the fp32 atomic accumulation plus the one rounding to the leaf's type.
    The terms are what the kernel adds: g_rel to the neighbour, (g_ctr - g_rel) to the centre."""
    gen = torch.Generator().manual_seed(70 + k)
    if kind == "degrees":
        idx = eo.graph_with_in_degrees(B, N, k, seed=7).to(device)
    else:
        idx = torch.randint(0, N, (B, N, k), generator=gen, dtype=torch.int32).to(device)
    xb = torch.randn(B, C, N, generator=gen).to(device).bfloat16().requires_grad_(True)
    e = fsg.functional.edge_features(xb, idx)
    assert e.dtype == torch.bfloat16 and e.shape == (B, 2 * C, N, k)
    g = torch.randn(B, 2 * C, N, k, generator=gen).to(device).bfloat16()
    e.backward(g)
    assert xb.grad.dtype == torch.bfloat16
    g64 = g.double()
    rel, own = g64[:, :C], g64[:, C:] - g64[:, :C]                       # (B,C,N,k)
    tgt = idx.long().unsqueeze(1).expand(B, C, N, k).reshape(B, C, N * k)
    want = own.sum(3).scatter_add(2, tgt, rel.reshape(B, C, N * k))
    terms = own.abs().sum(3).scatter_add(2, tgt, rel.abs().reshape(B, C, N * k))
    bound = 0.5 * bo.bf16_ulp(want) + 2.0 ** -20 * terms
    err = (xb.grad.double() - want).abs()
    print("EC2BF edge_gather_bf16 %s  err/bound %.3g  largest in-degree %d" % (kind, float((err / bound).max()),
                                                                              int(torch.bincount(idx[0].reshape(-1).long()).max())))
    assert bool((err <= bound).all())
