"""GPU tests of the members of the point-wise head family (csrc/pointwise.hip) one by one against tests/pw_oracle.py (float64):
every instantiated (prologue, epilogue, tile) of fsg_pw_rowgemm_f32, fsg_pw_tn_f32 with its prologues / second segment / ones
column / deferred reduction, and the small members that were reached only through functional.seg_head.

How a value is judged: |got - fp64| relative to the sum of the absolute summands of that value (pw_oracle's `mag`), against
max(1e-6, 2 x the same ratio of an fp32 ATen composition of the identical operation on the GPU), measured in the test -- the rule
and the margin 2 of test_pw_linear_is_fp32_grade.  Every figure is printed before it is asserted; profiles/pw_family_parity.txt
holds them.  The inputs of the parametrised cases are generated and pinned by tests/test_pw_oracle_cpu.py (no LeakyReLU argument
within pw_oracle.KINK_MARGIN of 0, selection margins above 4 x pw_oracle.SEL_NOISE), so no element is left out here; the one
comparison not made is sel_arg of the 'meanshift' cases, whose rows are near-copies of each other by construction (sel_val is
compared there).

MEASURED on an MI355X (profiles/pw_family_parity.txt, 385 figures): the kernels' largest is 8.8e-7 (invstd of a BatchNorm whose
per-cloud shift the kernel forms in fp32; the ATen composition has 5.7e-6 there), the largest of a product 6.7e-7 (ATen 9.9e-7);
the records' M2 is where the kernels sit furthest above ATen (4.9e-7 against 9.8e-8), still under the floor.  No case needed
more than max(1e-6, 2 x ATen), so the constant stays the one of test_pw_linear_is_fp32_grade.  The head at other widths: d levels
per row 8.8e-7 ... 3.4e-6 (ATen 8.8e-7 ... 8.4e-6).
fsg_pw_bn_finalize_f32 accepts a record with n = 0 (it adds nothing; a cloud or a whole call without rows gives mean 0): one
case carries such a record.  The head at other widths (test_seg_head_other_widths): logits 1e-4 of their scale; d levels per
row (edgeconv_oracle.row_error) on the rows the near-tie rule of test_seg_head_fused_vs_fp64_and_unfused keeps (at most 16 left
out), parameters in norm; bound max(floor, 3 x the fp32 ATen head), floors 5e-6 per row and 2e-3 in norm as in
tests/test_edgeconv_gpu.py.
"""
import numpy as np
import pytest
import torch

import edgeconv_oracle as eo
import pw_oracle as po

pytestmark = pytest.mark.gpu

FLOOR, MARGIN = 1e-6, 2.0


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def G(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def judge(name, got, aten, ref, mag, floor=FLOOR):
    """max |got - ref| / mag against max(floor, MARGIN x the ATen composition's)"""
    ref, mag = ref.to(got.device), mag.to(got.device).clamp_min(1e-300)
    e_k = float(((got.double() - ref).abs() / mag).max())
    e_a = float(((aten.double() - ref).abs() / mag).max())
    print("PWFAM %-40s kernel %.3g  aten %.3g" % (name, e_k, e_a))
    assert e_k <= max(floor, MARGIN * e_a), (name, e_k, e_a)


def lrelu32(u, slope):
    return torch.where(u > 0, u, u * slope)


def dl32(u, slope):
    return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))


def rows_of(tab, M, rpc, per_cloud):
    return tab[torch.arange(M, device=tab.device) // rpc] if per_cloud else tab[:1]


def run_rowgemm(F, c, t, store_n0=0, sel_n=None):
    """the kernel on the case's tensors `t` (GPU float32) -> dict like pw_oracle.rowgemm's"""
    dev = t["A1"].device
    M, K1, K2, N, BM = c["M"], c["K1"], c["K2"], c["N"], c["BM"]
    pro, epi = c["pro"], c["epi"]
    f32 = dict(dtype=torch.float32, device=dev)
    kw = dict(A1=t["A1"], lda1=t["A1"].stride(0), K1=K1, K2=K2, Bimg=t["img"], M=M, N=N, rows_per_cloud=c["rpc"], slope=c["slope"],
              store_n0=store_n0)
    out = {}
    if K2:
        kw.update(A2=t["A2"][:, 4:4 + K2], lda2=t["A2"].stride(0))
    if pro:
        kw.update(alpha=t["alpha"], delta=t["delta"], tstride=K1 if c["per_cloud"] else 0)
    if pro == po.PRO_BNBWD:
        kw.update(Y1=t["Y1"], P=t["P"], Q=t["Q"])
    if epi & po.PW_STORE:
        out["C"] = torch.full((M, N - store_n0 + 3), -777.0, **f32)
        kw.update(C=out["C"], ldc=out["C"].stride(0))
    if epi & po.PW_BIAS:
        kw.update(bias=t["bias"])
    R = M // BM
    if epi & po.PW_STATS:
        out["rec"] = torch.full((R, 3, N), -777.0, **f32)
        kw.update(rec=out["rec"])
    if epi & po.PW_SEL:
        sn = N if sel_n is None else sel_n
        out["sel_val"] = torch.full((R, sn), -777.0, **f32)
        out["sel_arg"] = torch.full((R, sn), -7, dtype=torch.int32, device=dev)
        kw.update(sgn=t["sgn"], sel_val=out["sel_val"], sel_arg=out["sel_arg"], sel_n=sn)
    if epi & po.PW_BWDSTATS:
        out["rec2"] = torch.full((R, 2, N), -777.0, **f32)
        kw.update(Yp=t["Yp"], ldyp=N, ealpha=t["ealpha"], edelta=t["edelta"], emu=t["emu"], er=t["er"],
                  etstride=N if c["per_cloud"] else 0, rec2=out["rec2"])
    F.pw_rowgemm(pro, epi, c["tile"], **kw)
    torch.cuda.synchronize()
    return out


def aten_rowgemm(c, t, store_n0=0):
    """the same operation as fp32 tensor ops + `@` on the GPU (the yardstick)"""
    M, K1, K2, N, BM, rpc, pc, slope = c["M"], c["K1"], c["K2"], c["N"], c["BM"], c["rpc"], c["per_cloud"], c["slope"]
    a = t["A1"][:, :K1]
    if c["pro"] == po.PRO_BNACT:
        a = lrelu32(t["alpha"] * a + rows_of(t["delta"], M, rpc, pc), slope)
    elif c["pro"] == po.PRO_BNBWD:
        y = t["Y1"][:, :K1]
        a = t["alpha"] * a * dl32(t["alpha"] * y + rows_of(t["delta"], M, rpc, pc), slope) - rows_of(t["P"], M, rpc, pc) - t["Q"] * y
    if K2:
        a = torch.cat([a, t["A2"][:, 4:4 + K2]], 1)
    cc = a @ t["W"].t()
    out = {"c": cc}
    epi = c["epi"]
    if epi & po.PW_STORE:
        out["C"] = (cc + t["bias"] if epi & po.PW_BIAS else cc)[:, store_n0:]
    if epi & po.PW_STATS:
        ct = cc.view(-1, BM, N)
        mean = ct.mean(1)
        out["rec"] = torch.stack([torch.full_like(mean, BM), mean, (ct - mean[:, None]).pow(2).sum(1)], 1)
    if epi & po.PW_SEL:
        s = torch.where(t["sgn"] < 0, -1.0, 1.0)
        out["sel_val"] = (cc.view(-1, BM, N) * s).max(1)[0]
    if epi & po.PW_BWDSTATS:
        fp = dl32(t["ealpha"] * t["Yp"] + rows_of(t["edelta"], M, rpc, pc), slope)
        h = cc * fp
        yh = (t["Yp"] - rows_of(t["emu"], M, rpc, pc)) * t["er"]
        out["rec2"] = torch.stack([h.view(-1, BM, N).sum(1), (h * yh).view(-1, BM, N).sum(1)], 1)
    return out


def case_tensors(F, c, d, device):
    t = {k: G(v, device) for k, v in d.items()}
    t["img"] = F.pw_weight_image(t["W"])
    return t


@pytest.mark.parametrize("case", po.rowgemm_cases(), ids=po.case_id)
def test_rowgemm_vs_fp64(fsg, device, case):
    """stored product, (n, mean, M2) records, selection and BatchNorm-backward sums of one instantiated combination; padding of C
    untouched; two runs bitwise equal"""
    F = fsg.functional
    d = po.rowgemm_inputs(case)
    t = case_tensors(F, case, d, device)
    ref = po.rowgemm_oracle(case, d)
    got, aten = run_rowgemm(F, case, t), aten_rowgemm(case, t)
    name, N, epi = po.case_id(case), case["N"], case["epi"]
    judge(name + " C", got["C"][:, :N], aten["C"], ref["C"], ref["mag"])
    assert bool((got["C"][:, N:] == -777.0).all())
    if epi & po.PW_STATS:
        assert torch.equal(got["rec"][:, 0].cpu(), ref["rec"][:, 0].float())
        for i, what in ((1, "mean"), (2, "M2")):
            judge(name + " rec " + what, got["rec"][:, i], aten["rec"][:, i], ref["rec"][:, i], ref["rec_mag"][:, i])
    if epi & po.PW_SEL:
        mag_t = ref["mag"].view(-1, case["BM"], N).max(1)[0]
        judge(name + " sel_val", got["sel_val"], aten["sel_val"], ref["sel_val"], mag_t)
        if case["kind"] in ("a", "b"):
            assert torch.equal(got["sel_arg"].cpu(), ref["sel_arg"])
    if epi & po.PW_BWDSTATS:
        for i, what in ((0, "sum h"), (1, "sum h yhat")):
            judge(name + " rec2 " + what, got["rec2"][:, i], aten["rec2"][:, i], ref["rec2"][:, i], ref["rec2_mag"][:, i])
    again = run_rowgemm(F, case, t)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("tile", [1, 2])
def test_rowgemm_store_n0_and_sel_n(fsg, device, tile):
    """STORE | STATS | SEL with store_n0 = sel_n = 64 of N = 128: only the right half is stored, the statistics cover all the
    columns, the selection only the left ones"""
    F = fsg.functional
    BM = po.tile_rows(tile)
    case = dict(pro=0, epi=7, tile=tile, BM=BM, kind="a", rpc=2 * BM, M=4 * BM, K1=96, K2=0, N=128, per_cloud=False, slope=0.2,
                seed=5000 + tile)
    d = po.rowgemm_inputs(case)
    t = case_tensors(F, case, d, device)
    ref = po.rowgemm_oracle(case, d, store_n0=64, sel_n=64)
    got, aten = run_rowgemm(F, case, t, store_n0=64, sel_n=64), aten_rowgemm(case, t, store_n0=64)
    assert ref["C"].shape == (4 * BM, 64) and got["sel_val"].shape[1] == 64
    judge("store_n0 tile%d C" % tile, got["C"][:, :64], aten["C"], ref["C"], ref["mag"][:, 64:])
    assert bool((got["C"][:, 64:] == -777.0).all())
    judge("store_n0 tile%d mean" % tile, got["rec"][:, 1], aten["rec"][:, 1], ref["rec"][:, 1], ref["rec_mag"][:, 1])
    judge("store_n0 tile%d sel_val" % tile, got["sel_val"], aten["sel_val"][:, :64], ref["sel_val"],
          ref["mag"].view(-1, BM, 128).max(1)[0][:, :64])
    s = torch.where(torch.from_numpy(d["sgn"]) < 0, -1.0, 1.0).double()
    margins = po.selection_margins(ref["c"] * s, BM)[:, :64]
    keep = margins > 4 * po.SEL_NOISE * ref["mag"].view(-1, BM, 128).max(1)[0][:, :64]
    assert bool(keep.all())
    assert torch.equal(got["sel_arg"].cpu(), ref["sel_arg"])


@pytest.mark.parametrize("tile", [1, 2])
def test_rowgemm_selection_is_exact_on_integers(fsg, device, tile):
    """small integers (every product and partial sum representable), rows duplicated inside a tile and across the tiles of a
    cloud: sel_val bit-exact, sel_arg the lowest row, for both signs of sgn"""
    F = fsg.functional
    BM = po.tile_rows(tile)
    g = np.random.default_rng(60 + tile)
    M, K, N = 4 * BM, 96, 77
    A = g.integers(-8, 9, (M, K)).astype(np.float32)
    for r in (3, 40, BM - 1, BM + 7, 2 * BM + 5):
        A[r] = A[BM // 2]                                     # copies inside tile 0, in tile 1 (same cloud) and in the next cloud
    A[3 * BM + 9] = A[2 * BM + 5]
    W = g.integers(-8, 9, (N, K)).astype(np.float32)
    sgn = np.where(np.arange(N) % 2 == 0, 1.0, -2.0).astype(np.float32)
    case = dict(pro=0, epi=7, tile=tile, BM=BM, kind="int", rpc=2 * BM, M=M, K1=K, K2=0, N=N, per_cloud=False, slope=0.2)
    d = {"A1": A, "W": W, "sgn": sgn}
    t = case_tensors(F, case, d, device)
    ref = po.rowgemm_oracle(case, d)
    got = run_rowgemm(F, case, t)
    assert torch.equal(got["C"][:, :N].cpu().double(), ref["C"])
    assert torch.equal(got["sel_val"].cpu().double(), ref["sel_val"])
    assert torch.equal(got["sel_arg"].cpu(), ref["sel_arg"])
    v = (ref["c"] * torch.where(torch.from_numpy(sgn) < 0, -1.0, 1.0)).view(-1, BM, N)
    assert int((v == v.max(1, keepdim=True)[0]).sum(1).max()) >= 2          # there were ties to resolve
    # ... and across the tiles of a cloud: the finish takes the lowest row too
    f32 = dict(dtype=torch.float32, device=device)
    out, ysel, arg = torch.empty(2, N, **f32), torch.empty(2, N, **f32), torch.empty(2, N, dtype=torch.int32, device=device)
    al, de = torch.ones(N, **f32), torch.zeros(N, **f32)
    fsg._lib.call("fsg_pw_max_finish_f32", got["sel_val"].data_ptr(), got["sel_arg"].data_ptr(), t["sgn"].data_ptr(), al.data_ptr(),
                  de.data_ptr(), 2, 2, N, 0.2, out.data_ptr(), ysel.data_ptr(), arg.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _, ysel64, arg64 = po.max_finish(ref["sel_val"], ref["sel_arg"], torch.from_numpy(sgn).double(), torch.ones(N).double(),
                                     torch.zeros(N).double(), 2, 2, 0.2)
    assert torch.equal(arg.cpu(), arg64) and torch.equal(ysel.cpu().double(), ysel64)


# --------------------------------------------------------------------------------------------------------------------- tn

def run_tn(F, c, t, defer=None, poison=-555.0):
    dev = t["R"].device
    N1a, N1b, N2 = c["N1a"], c["N1b"], c["N2"]
    f32 = dict(dtype=torch.float32, device=dev)
    C1 = torch.full((N1a, N2 + 4), poison, **f32)
    C2 = torch.full((N1b + c["ones"], N2 + 8), poison, **f32) if N1b + c["ones"] and N1b else None
    kw = dict(L1=t["L1"], ldl1=t["L1"].stride(0), N1a=N1a, N1b=N1b, lpro=c["lpro"], R=t["R"], ldr=t["R"].stride(0), N2=N2, rpro=c["rpro"],
              slope=0.2, M=c["M"], rows_per_cloud=c["rpc"], rows_per_slice=c["rps"], ones=c["ones"])
    if N1b:
        kw.update(L2=t["L2"], ldl2=t["L2"].stride(0))
    if c["lpro"]:
        kw.update(LY1=t["LY1"], lalpha=t["lalpha"], ldelta=t["ldelta"], lP=t["lP"], lQ=t["lQ"], lts=N1a if c["lpc"] else 0)
    if c["rpro"]:
        kw.update(ralpha=t["ralpha"], rdelta=t["rdelta"], rts=N2 if c["rpc_tab"] else 0)
    F.pw_tn(c["tile"], C1, C1.stride(0), C2, C2.stride(0) if C2 is not None else 0, defer=defer, **kw)
    return C1, C2


def aten_tn(c, t):
    M, N1a, N2, rpc = c["M"], c["N1a"], c["N2"], c["rpc"]
    left, right = t["L1"][:, :N1a], t["R"][:, :N2]
    if c["lpro"]:
        y = t["LY1"][:, :N1a]
        left = t["lalpha"] * left * dl32(t["lalpha"] * y + rows_of(t["ldelta"], M, rpc, c["lpc"]), 0.2) - \
            rows_of(t["lP"], M, rpc, c["lpc"]) - t["lQ"] * y
    if c["rpro"]:
        right = lrelu32(t["ralpha"] * right + rows_of(t["rdelta"], M, rpc, c["rpc_tab"]), 0.2)
    if c["N1b"]:
        left = torch.cat([left, t["L2"]], 1)
    if c["ones"]:
        left = torch.cat([left, torch.ones(M, 1, dtype=torch.float32, device=left.device)], 1)
    return left.t() @ right


@pytest.mark.parametrize("case", po.tn_cases(), ids=lambda c: c["name"])
def test_tn_vs_fp64(fsg, device, case):
    """value against fp64 (mag-relative, M the contraction length), padding of C1 / C2 untouched, bitwise reproducible, and the
    same bits when the slices are left in the workspace and folded by fsg_pw_tn_reduce_f32"""
    F = fsg.functional
    d = po.tn_inputs(case)
    t = {k: G(v, device) for k, v in d.items()}
    ref, mag = po.tn_oracle(case, d)
    C1, C2 = run_tn(F, case, t)
    torch.cuda.synchronize()
    N1a, N2 = case["N1a"], case["N2"]
    got = torch.cat([C1[:, :N2]] + ([C2[:, :N2]] if C2 is not None else []), 0)
    judge("tn " + case["name"], got, aten_tn(case, t), ref, mag)
    assert bool((C1[:, N2:] == -555.0).all()) and (C2 is None or bool((C2[:, N2:] == -555.0).all()))
    B1, B2 = run_tn(F, case, t)
    assert torch.equal(C1, B1) and (C2 is None or torch.equal(C2, B2))
    jobs = []
    D1, D2 = run_tn(F, case, t, defer=jobs)
    assert bool((D1 == -555.0).all())                          # nothing written before the fold
    F.pw_tn_reduce(jobs)
    assert torch.equal(C1, D1) and (C2 is None or torch.equal(C2, D2))


@pytest.mark.parametrize("njobs", [1, 4, 6])
def test_tn_deferred_reduction_of_several_products(fsg, device, njobs):
    """1, 4 and 6 products of different shapes folded in ONE launch == each folded at once, bitwise; a 7th job is refused"""
    F = fsg.functional
    cases = po.tn_cases()[:njobs]
    ts = [{k: G(v, device) for k, v in po.tn_inputs(c).items()} for c in cases]
    now = [run_tn(F, c, t) for c, t in zip(cases, ts)]
    jobs = []
    later = [run_tn(F, c, t, defer=jobs) for c, t in zip(cases, ts)]
    assert len(jobs) == njobs
    F.pw_tn_reduce(jobs)
    for (a1, a2), (b1, b2) in zip(now, later):
        assert torch.equal(a1, b1) and (a2 is None or torch.equal(a2, b2))
    if njobs == 6:
        with pytest.raises(AssertionError):
            F.pw_tn_reduce(jobs + jobs[:1])


# --------------------------------------------------------------------------------------------------------------------- small members

def _call(fsg, name, *a):
    fsg._lib.call(name, *[x.data_ptr() if torch.is_tensor(x) else x for x in a], torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("tiles", [1, 5])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_bn_finalize_max_is_finalize_then_max_finish(fsg, device, B, tiles):
    """fsg_pw_bn_finalize_max_f32 == fsg_pw_bn_finalize_f32 followed by fsg_pw_max_finish_f32, bitwise, with 1 and 5 tiles per
    cloud; ties across tiles go to the lowest row; the statistics against the oracle (records with means far from each other:
    50 +- 0.1 spread)"""
    g = np.random.default_rng(70 + B + tiles)
    C, c0, ldn = 70, 5, 80
    R = B * tiles
    rec = np.zeros((R, 3, ldn), np.float32)
    rec[:, 0], rec[:, 1] = 64.0, 50.0 + 0.1 * g.standard_normal((R, ldn))
    rec[:, 2] = 64 * 0.01 * g.uniform(0.5, 1.5, (R, ldn))
    sel_val = g.integers(-3, 4, (R, C)).astype(np.float32)     # many ties across the tiles of a cloud
    sel_arg = (np.arange(R)[:, None] % tiles * 64 + g.integers(0, 64, (R, C))).astype(np.int32)
    gamma = (g.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 0, -1, 1)).astype(np.float32)
    beta = g.standard_normal(C).astype(np.float32)
    t = {k: G(v, device) for k, v in dict(rec=rec, sel_val=sel_val, sel_arg=sel_arg, gamma=gamma, beta=beta).items()}
    f32 = dict(dtype=torch.float32, device=device)

    def outs():
        return [torch.zeros(C, **f32) for _ in range(5)] + [torch.full((C,), 1.0, **f32)] + \
            [torch.empty(B, C, **f32), torch.empty(B, C, **f32), torch.empty(B, C, dtype=torch.int32, device=device)]
    mean, inv, al, de, rm, rv, out, ysel, arg = outs()
    _call(fsg, "fsg_pw_bn_finalize_max_f32", t["rec"], R, ldn, c0, C, B, 1, t["gamma"], t["beta"], 1e-5, 1.0 / 3.0, rm, rv, mean, inv, al, de,
          t["sel_val"], t["sel_arg"], t["gamma"], tiles, 0.2, out, ysel, arg)
    mean2, inv2, al2, de2, rm2, rv2, out2, ysel2, arg2 = outs()
    _call(fsg, "fsg_pw_bn_finalize_f32", t["rec"], R, ldn, c0, C, None, B, 1, t["gamma"], t["beta"], 1e-5, 1.0 / 3.0, rm2, rv2, mean2, inv2,
          al2, de2, None, None, None, None, 0, 0, None)
    _call(fsg, "fsg_pw_max_finish_f32", t["sel_val"], t["sel_arg"], t["gamma"], al2, de2, B, tiles, C, 0.2, out2, ysel2, arg2)
    torch.cuda.synchronize()
    for a, b in ((mean, mean2), (inv, inv2), (al, al2), (de, de2), (rm, rm2), (rv, rv2), (out, out2), (ysel, ysel2), (arg, arg2)):
        assert torch.equal(a, b)
    T64 = lambda a: torch.from_numpy(a).double()
    o = po.bn_finalize(T64(rec), c0, C, B, 1, T64(gamma), T64(beta), 1e-5, 1.0 / 3.0, running_mean=torch.zeros(C).double(),
                       running_var=torch.ones(C).double())
    o_out, o_ysel, o_arg = po.max_finish(T64(sel_val), torch.from_numpy(sel_arg), T64(gamma), o["alpha"], o["delta"], B, tiles, 0.2)
    assert torch.equal(arg.cpu(), o_arg) and torch.equal(ysel.cpu().double(), o_ysel)
    for nm, a, b in (("mean", mean, o["mean"]), ("invstd", inv, o["invstd"]), ("alpha", al, o["alpha"]),
                     ("running_mean", rm, o["running_mean"]), ("running_var", rv, o["running_var"])):
        e = float(((a.cpu().double() - b).abs() / b.abs().clamp_min(1e-30)).max())
        print("PWFAM bn_finalize_max B%d %-14s rel %.3g" % (B, nm, e))
        assert e <= 4 * 2.0 ** -24, (nm, e)                  # fp64 inside, one rounding to fp32 (+ one fp32 product for alpha) on the way out
    e = float((de.cpu().double().view(-1) - o["delta"].view(-1)).abs().max() / ((o["alpha"] * o["mean"]).abs() + T64(beta).abs()).max())
    assert e <= 4 * 2.0 ** -24, e


@pytest.mark.parametrize("B,CG", [(1, 64), (32, 1000)])
def test_cloud_linear_vs_fp64(fsg, device, B, CG):
    g = np.random.default_rng(B + CG)
    C0 = 70
    x, Wf = po.wide_range((B, CG), 4, g), po.wide_range((C0, CG + 24), 4, g)
    xt, Wt = G(x, device), G(Wf, device)[:, 24:]               # a strided view, as W0[:, KL:] is
    out = torch.empty(B, C0, dtype=torch.float32, device=device)
    _call(fsg, "fsg_pw_cloud_linear_f32", xt, Wt, Wt.stride(0), B, C0, CG, out)
    x64, W64 = torch.from_numpy(x).double(), torch.from_numpy(Wf[:, 24:].copy()).double()
    judge("cloud_linear B%d CG%d" % (B, CG), out, xt @ Wt.t(), po.cloud_linear(x64, W64), x64.abs() @ W64.abs().t())


@pytest.mark.parametrize("classes,M,C", [(1, 32, 64), (4, 1000, 128), (8, 1000, 64)])
def test_logits_bwd_vs_fp64(fsg, device, classes, M, C):
    g = np.random.default_rng(classes + M + C)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    gr, W3 = f(M, classes), f(classes, C)
    al = (g.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 0, -1, 1)).astype(np.float32)
    de, mu, inv = 0.5 * f(C), 0.3 * f(C), g.uniform(0.5, 2.0, C).astype(np.float32)
    y = po.away_from_kink(f(M, C), al, de, po.KINK_MARGIN)
    assert po.kink_count(y, al, de, po.KINK_MARGIN) == 0
    t = [G(a, device) for a in (gr, W3, y, al, de, mu, inv)]
    R = (M + 31) // 32
    da = torch.empty(M, C, dtype=torch.float32, device=device)
    rec2 = torch.empty(R, 2, C, dtype=torch.float32, device=device)
    _call(fsg, "fsg_pw_logits_bwd_f32", t[0], classes, t[1], t[2], t[3], t[4], t[5], t[6], M, C, 0.2, da, rec2)
    T64 = lambda a: torch.from_numpy(a).double()
    o_da, o_rec2, mag, rmag = po.logits_bwd(T64(gr), T64(W3), T64(y), T64(al), T64(de), T64(mu), T64(inv), 0.2)
    a_da = t[0] @ t[1]
    h = a_da * dl32(t[3] * t[2] + t[4], 0.2)
    pad = lambda v: torch.nn.functional.pad(v, (0, 0, 0, R * 32 - M)).view(R, 32, C).sum(1)
    a_rec2 = torch.stack([pad(h), pad(h * ((t[2] - t[5]) * t[6]))], 1)
    judge("logits_bwd %d/%d/%d da" % (classes, M, C), da, a_da, o_da, mag)
    for i, what in ((0, "sum h"), (1, "sum h yhat")):
        judge("logits_bwd %d/%d/%d %s" % (classes, M, C, what), rec2[:, i], a_rec2[:, i], o_rec2[:, i], rmag[:, i])


@pytest.mark.parametrize("C,kind", [(64, "random"), (4096, "random"), (64, "same-row"), (4096, "ends")])
def test_scatter_rows_vs_fp64(fsg, device, C, kind):
    """dX[b Npts + arg[b,c], :] += coef[b,c] W[c, :]: random selections, every channel of a cloud on one row, selections on the
    first and last row of a cloud; rows outside the selection unchanged bitwise; bitwise reproducible"""
    g = np.random.default_rng(C + len(kind))
    B, K, Npts = 3, 64, 256
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    coef, W, dX = f(B, C), f(C, K + 4), f(B * Npts, K)
    arg = g.integers(0, Npts, (B, C)).astype(np.int32)
    if kind == "same-row":
        arg[:] = np.array([[0], [Npts - 1], [17]], np.int32)
    if kind == "ends":
        arg[:, ::2], arg[:, 1::2] = 0, Npts - 1
    ct, at, Wt = G(coef, device), G(arg, device), G(W, device)[:, :K]
    ws = torch.empty(fsg._lib.lib.fsg_pw_scatter_rows_workspace_bytes(B, C) // 4, dtype=torch.int32, device=device)

    def run():
        x = G(dX, device)
        _call(fsg, "fsg_pw_scatter_rows_f32", ct, at, Wt, Wt.stride(0), B, C, K, Npts, x, K, ws)
        return x
    x1, x2 = run(), run()
    assert torch.equal(x1, x2)
    T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    ref = po.scatter_rows(T64(dX), T64(coef), torch.from_numpy(arg), T64(W[:, :K]), Npts)
    rows = (np.arange(B)[:, None] * Npts + arg).reshape(-1)
    mag = T64(np.abs(dX)).index_add(0, torch.from_numpy(rows).long(), (T64(np.abs(coef))[:, :, None] * T64(np.abs(W[:, :K]))[None]).reshape(B * C, K))
    aten = G(dX, device).index_add(0, G(rows, device).long(), (ct[:, :, None] * Wt[None]).reshape(B * C, K))
    judge("scatter_rows C%d %s" % (C, kind), x1, aten, ref, mag)
    untouched = np.ones(B * Npts, bool)
    untouched[rows] = False
    assert np.array_equal(x1.cpu().numpy()[untouched], dX[untouched])


def _rel(name, got, aten, ref, mag):
    judge(name, got, aten.to(got.device), ref, mag)


# (B, records per cloud, mode, emu, cloud_mean, momentum, a record with n = 0)
BNF_CASES = [(3, 1, "shift", True, True, 0.1, False), (3, 4, "gfeat", True, True, 1.0 / 3.0, False), (3, 37, "shift", False, False, 0.1, False),
             (3, 37, "plain", True, False, 1.0 / 3.0, False), (2, 4, "shift", True, True, 0.1, True), (64, 1, "gfeat", False, True, 0.1, False)]


@pytest.mark.parametrize("B,rpc,mode,want_emu,want_cm,mom,n0", BNF_CASES)
@pytest.mark.parametrize("training", [1, 0])
def test_bn_finalize_vs_fp64(fsg, device, B, rpc, mode, want_emu, want_cm, mom, n0, training):
    """fsg_pw_bn_finalize_f32 on its own: columns [c0, c0 + C) of wider records, shift given / formed from gfeat Wglob^T and
    written back / absent, emu and cloud_mean requested or not, R in {B, 4B, 37B}, records with means of 50 and a spread of 0.1,
    a record with n = 0, the running update at momentum 0.1 and 1/3; training = 0 writes the tables only (mean / invstd bitwise
    untouched, running statistics not given)"""
    g = np.random.default_rng(B * 100 + rpc + len(mode))
    C, c0, ldn, CG = 70, 5, 80, 100
    R = B * rpc
    rec = np.zeros((R, 3, ldn), np.float32)
    rec[:, 0], rec[:, 1] = 64.0, 50.0 + 0.1 * g.standard_normal((R, ldn))
    rec[:, 2] = 64 * 0.01 * g.uniform(0.5, 1.5, (R, ldn))
    if n0:
        rec[1, 0], rec[1, 1], rec[1, 2] = 0.0, 123.0, 0.0
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    gamma = (g.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 0, -1, 1)).astype(np.float32)
    beta, shift, gfeat, Wgl = f(C), f(B, C), f(B, CG), 0.1 * f(C, CG + 8)
    rm0, rv0 = 0.3 * f(C), g.uniform(0.5, 2.0, C).astype(np.float32)
    mean_in, inv_in = (50 + f(C)).astype(np.float32), g.uniform(0.5, 2.0, C).astype(np.float32)
    f32 = dict(dtype=torch.float32, device=device)
    t = {k: G(v, device) for k, v in dict(rec=rec, gamma=gamma, beta=beta, shift=shift, gfeat=gfeat, Wgl=Wgl).items()}
    nb = B if mode != "plain" else 1
    mean, inv = (torch.full((C,), -7.0, **f32), torch.full((C,), -7.0, **f32)) if training else (G(mean_in, device), G(inv_in, device))
    rm, rv = (G(rm0, device), G(rv0, device)) if training else (None, None)
    al, de = torch.empty(C, **f32), torch.full((nb, C), -7.0, **f32)
    emu = torch.full((nb, C), -7.0, **f32) if want_emu else None
    cm = torch.full((B, C), -7.0, **f32) if want_cm else None
    sh = {"plain": None, "shift": t["shift"].clone(), "gfeat": torch.full((B, C), -7.0, **f32)}[mode]
    gf, wg = (t["gfeat"], t["Wgl"][:, :CG]) if mode == "gfeat" else (None, None)
    _call(fsg, "fsg_pw_bn_finalize_f32", t["rec"], R, ldn, c0, C, sh, B, training, t["gamma"], t["beta"], 1e-5, mom, rm, rv, mean, inv, al, de,
          emu, cm, gf, wg, wg.stride(0) if wg is not None else 0, CG if gf is not None else 0, sh if gf is not None else None)
    torch.cuda.synchronize()

    def oracle(cv):
        kw = dict(shift=cv(shift) if mode == "shift" else None, want_emu=want_emu, want_cloud_mean=want_cm)
        if mode == "gfeat":
            kw.update(gfeat=cv(gfeat), Wglob=cv(Wgl[:, :CG].copy()))
        if training:
            kw.update(running_mean=cv(rm0), running_var=cv(rv0))
        else:
            kw.update(mean=cv(mean_in), invstd=cv(inv_in))
        return po.bn_finalize(cv(rec), c0, C, B, training, cv(gamma), cv(beta), 1e-5, mom, **kw)
    o = oracle(lambda a: torch.from_numpy(a).double())
    a32 = oracle(lambda a: G(a, device))
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    name = "bn_finalize B%d R%d %s tr%d" % (B, R, mode, training)
    sh64 = o["shift"].abs() if o["shift"] is not None else torch.zeros(1, C).double()
    if mode == "gfeat":
        _rel(name + " shift", sh, a32["shift"], o["shift"], D(np.abs(gfeat)) @ D(np.abs(Wgl[:, :CG])).t())
    if training:
        n64, mu64 = D(rec[:, 0, c0:c0 + C]), D(rec[:, 1, c0:c0 + C])
        mmag = (n64 * (mu64.abs() + (sh64.repeat_interleave(rpc, 0) if mode != "plain" else 0))).sum(0) / n64.sum(0)
        _rel(name + " mean", mean, a32["mean"], o["mean"], mmag)
        _rel(name + " invstd", inv, a32["invstd"], o["invstd"], o["invstd"])
        _rel(name + " running_mean", rm, a32["running_mean"], o["running_mean"], (1 - mom) * D(np.abs(rm0)) + mom * mmag)
        _rel(name + " running_var", rv, a32["running_var"], o["running_var"], o["running_var"])
    else:
        assert torch.equal(mean.cpu(), torch.from_numpy(mean_in)) and torch.equal(inv.cpu(), torch.from_numpy(inv_in))
    _rel(name + " alpha", al, a32["alpha"], o["alpha"], o["alpha"].abs())
    _rel(name + " delta", de, a32["delta"], o["delta"], o["alpha"].abs() * (sh64 + o["mean"].abs()) + D(np.abs(beta)))
    if want_emu:
        _rel(name + " emu", emu, a32["emu"], o["emu"], sh64 + o["mean"].abs())
    if want_cm:
        if training:
            nr, mr = D(rec[:, 0, c0:c0 + C]).view(B, rpc, C), D(rec[:, 1, c0:c0 + C]).view(B, rpc, C)
            _rel(name + " cloud_mean", cm, a32["cloud_mean"], o["cloud_mean"], (nr * mr.abs()).sum(1) / nr.sum(1))
        else:
            assert bool((cm == -7.0).all())                   # eval: not written


@pytest.mark.parametrize("per_cloud,want_dc,training,rpc", [(0, 0, 1, 4), (1, 1, 1, 4), (1, 0, 1, 37), (1, 1, 0, 4), (0, 0, 0, 1), (1, 1, 1, 1)])
def test_bnbwd_finalize_vs_fp64(fsg, device, per_cloud, want_dc, training, rpc):
    """dbeta, dgamma, P, Q and dc of fsg_pw_bnbwd_finalize_f32: per-cloud emu on and off, dc on and off, training 0 (P = Q = 0
    exactly) and 1"""
    g = np.random.default_rng(per_cloud * 4 + want_dc * 2 + training + rpc)
    B, C = 3, 70
    R, M = B * rpc, B * rpc * 64
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    rec2 = po.wide_range((R, 2, C), 3, g, lo=-1.0)
    alpha = (g.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 0, -1, 1)).astype(np.float32)
    inv, emu, cmn = g.uniform(0.5, 2.0, C).astype(np.float32), f(B if per_cloud else 1, C), f(B, C)
    f32 = dict(dtype=torch.float32, device=device)
    t = [G(a, device) for a in (rec2, alpha, inv, emu, cmn)]
    nb = B if per_cloud else 1
    dbeta, dgamma, P, Q = torch.empty(C, **f32), torch.empty(C, **f32), torch.empty(nb, C, **f32), torch.empty(C, **f32)
    dc = torch.empty(B, C, **f32) if want_dc else None
    _call(fsg, "fsg_pw_bnbwd_finalize_f32", t[0], R, C, B, M, training, t[1], t[2], t[3], per_cloud, t[4] if want_dc else None, dbeta, dgamma,
          P, Q, dc)
    torch.cuda.synchronize()
    D = lambda a: torch.from_numpy(a).double()
    o = po.bnbwd_finalize(D(rec2), B, M, training, D(alpha), D(inv), D(emu), per_cloud, D(cmn), bool(want_dc))
    a = po.bnbwd_finalize(t[0], B, M, training, t[1], t[2], t[3], per_cloud, t[4], bool(want_dc))
    r0, r1 = D(np.abs(rec2[:, 0])), D(np.abs(rec2[:, 1]))
    bm, gm = r0.sum(0), r1.sum(0)
    Qm = D(np.abs(alpha)) * gm / M * D(inv)
    Pm = D(np.abs(alpha)) * (bm / M + D(np.abs(emu)) * gm / M * D(inv))
    name = "bnbwd_finalize pc%d dc%d tr%d R%d" % (per_cloud, want_dc, training, R)
    _rel(name + " dbeta", dbeta, a[0], o[0], bm)
    _rel(name + " dgamma", dgamma, a[1], o[1], gm)
    if training:
        _rel(name + " P", P, a[2], o[2], Pm)
        _rel(name + " Q", Q, a[3], o[3], Qm)
    else:
        assert bool((P == 0).all()) and bool((Q == 0).all())
    if want_dc:
        nbr = M // B
        dcm = D(np.abs(alpha)) * r0.view(B, rpc, C).sum(1) + (nbr * Pm + Qm * nbr * D(np.abs(cmn))) * (1 if training else 0)
        _rel(name + " dc", dc, a[4], o[4], dcm)


@pytest.mark.parametrize("form", ["dc", "dg"])
@pytest.mark.parametrize("B", [1, 8, 9, 32])
def test_gf_prep_vs_fp64(fsg, device, B, form):
    """both forms of fsg_pw_gf_prep_f32 on both sides of the table-size switch at B <= 8; the dc form with dW0g written into a
    wider matrix and Wq rows at ldwq = K + 4 (padding untouched); eval mode for B = 9"""
    g = np.random.default_rng(B + len(form))
    C, C0, K, M = 130, 64, 64, B * 256
    training = 0 if B == 9 else 1
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    alpha = (g.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 0, -1, 1)).astype(np.float32)
    delta, mean, inv = 0.5 * f(C), 0.3 * f(C), g.uniform(0.5, 2.0, C).astype(np.float32)
    ysel = po.away_from_kink(f(B, C), alpha, delta, po.KINK_MARGIN)
    assert po.kink_count(ysel, alpha, delta, po.KINK_MARGIN) == 0
    dcv, W0 = f(B, C0), f(C0, K + C)                          # W0g = W0[:, K:], a strided view
    gfeat, dgv, W = f(B, C), f(B, C), f(C, K)
    f32 = dict(dtype=torch.float32, device=device)
    t = {k: G(v, device) for k, v in dict(alpha=alpha, delta=delta, mean=mean, inv=inv, ysel=ysel, dc=dcv, W0=W0, gfeat=gfeat, dg=dgv, W=W).items()}
    dbeta, dgamma, P, Q = (torch.empty(C, **f32) for _ in range(4))
    coef = torch.empty(B, C, **f32)
    dW0 = torch.full((C0, K + C), -7.0, **f32)
    Wq = torch.full((C, K + 4), -7.0, **f32)
    if form == "dc":
        W0g, dW0g = t["W0"][:, K:], dW0[:, K:]
        _call(fsg, "fsg_pw_gf_prep_f32", t["dc"], W0g, W0g.stride(0), C0, t["gfeat"], dW0g, dW0.stride(0), None, t["ysel"], t["alpha"], t["delta"],
              t["mean"], t["inv"], B, C, M, training, 0.2, dbeta, dgamma, P, Q, coef, t["W"], K, K, Wq, K + 4)
    else:
        _call(fsg, "fsg_pw_gf_prep_f32", None, None, 0, 0, None, None, 0, t["dg"], t["ysel"], t["alpha"], t["delta"], t["mean"], t["inv"], B, C, M,
              training, 0.2, dbeta, dgamma, P, Q, coef, None, 0, 0, None, 0)
    torch.cuda.synchronize()

    def oracle(cv):
        kw = dict(dc=cv(dcv), W0g=cv(W0[:, K:].copy()), gfeat=cv(gfeat), W=cv(W)) if form == "dc" else dict(dg=cv(dgv))
        return po.gf_prep(cv(ysel), cv(alpha), cv(delta), cv(mean), cv(inv), M, training, 0.2, **kw)
    o, a = oracle(lambda x: torch.from_numpy(x).double()), oracle(lambda x: G(x, device))
    name = "gf_prep B%d %s" % (B, form)
    for k, got in (("dbeta", dbeta), ("dgamma", dgamma), ("coef", coef)) + ((("P", P), ("Q", Q)) if training else ()):
        _rel(name + " " + k, got, a[k], o[k], o["mag"][k])
    if not training:
        assert bool((P == 0).all()) and bool((Q == 0).all())
    if form == "dc":
        _rel(name + " dW0g", dW0[:, K:], a["dW0g"], o["dW0g"], o["mag"]["dW0g"])
        assert bool((dW0[:, :K] == -7.0).all())
        if training:
            _rel(name + " Wq", Wq[:, :K + 1], a["Wq"], o["Wq"], o["mag"]["Wq"])
        assert bool((Wq[:, K + 1:] == -7.0).all())


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("B", [1, 32])
def test_gf_dw_vs_fp64(fsg, device, B, K):
    """dW[c, :] = sum_b coef[b,c] X[b Npts + arg[b,c], :] - P[c] s - Q[c] (W G)[c, :] with repeated selections"""
    g = np.random.default_rng(B + K)
    C, Npts = 70, 64
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    coef, X, sv, W, Gm, P, Q = f(B, C), f(B * Npts, K + 4), f(K), f(C, K + 8), f(K, K), 0.1 * f(C), 0.1 * f(C)
    arg = g.choice(np.array([0, 5, Npts - 1]), (B, C)).astype(np.int32)         # few rows: every one selected many times
    t = [G(a, device) for a in (coef, arg, X, sv, W, Gm, P, Q)]
    dW = torch.full((C, K + 4), -7.0, dtype=torch.float32, device=device)
    _call(fsg, "fsg_pw_gf_dw_f32", t[0], t[1], t[2], K + 4, t[3], t[4], K + 8, t[5], t[6], t[7], B, C, K, Npts, dW, K + 4)
    torch.cuda.synchronize()
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    ai = torch.from_numpy(arg)
    o = po.gf_dw(D(coef), ai, D(X[:, :K]), D(sv), D(W[:, :K]), D(Gm), D(P), D(Q), Npts)
    mag = po.gf_dw(D(np.abs(coef)), ai, D(np.abs(X[:, :K])), -D(np.abs(sv)), D(np.abs(W[:, :K])), -D(np.abs(Gm)), D(np.abs(P)), D(np.abs(Q)), Npts)
    a = po.gf_dw(t[0], t[1], t[2][:, :K], t[3], t[4][:, :K], t[5], t[6], t[7], Npts)
    _rel("gf_dw B%d K%d" % (B, K), dW[:, :K], a, o, mag)
    assert bool((dW[:, K:] == -7.0).all())


@pytest.mark.parametrize("dims,B,Npts", [((64, 128, 64, 64, 64, 1), 1, 256), ((128, 256, 128, 64, 64, 8), 5, 512)])
@pytest.mark.parametrize("train", [True, False])
def test_seg_head_other_widths(fsg, device, dims, B, Npts, train):
    """functional._SegHead (what functional.seg_head applies) at widths other than DGCNNSeg's against the fp64 head; the bounds are
    in the module docstring"""
    F = fsg.functional
    KL, CG, C0, C1, C2, CLS = dims
    gen = torch.Generator().manual_seed(sum(dims) + B)
    r = lambda *s: torch.randn(*s, generator=gen)
    P = {"Wg": r(CG, KL) / KL ** 0.5, "W0": r(C0, KL + CG) / (KL + CG) ** 0.5, "W1": r(C1, C0) / C0 ** 0.5, "W2": r(C2, C1) / C1 ** 0.5,
         "W3": r(CLS, C2) / C2 ** 0.5, "b3": r(CLS)}
    for k, C in (("g", CG), ("0", C0), ("1", C1), ("2", C2)):
        P["g" + k] = (0.5 + torch.rand(C, generator=gen)) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
        P["b" + k] = 0.2 * r(C)
        P["rm" + k], P["rv" + k] = 0.3 * r(C), 0.5 + 1.5 * torch.rand(C, generator=gen)
    M = B * Npts
    lv = 0.4 + 0.6 * r(M, KL)
    lv = torch.where(lv < 0, 0.2 * lv, lv)
    gout = r(M, CLS)
    names = ("Wg", "gg", "bg", "W0", "g0", "b0", "W1", "g1", "b1", "W2", "g2", "b2", "W3", "b3")

    def reference(cv):
        Pr = {k: (cv(v).requires_grad_(True) if k in names else cv(v)) for k, v in P.items()}
        x = cv(lv).requires_grad_(True)
        y = po.head_reference_fp64(x, B, Npts, Pr, 0.2, train)
        y.backward(cv(gout))
        return y.detach(), x.grad, {k: Pr[k].grad for k in names}, Pr, x
    y64, gx64, gp64, P64, x64 = reference(lambda v: v.double().to(device))
    y32, gx32, gp32, _, _ = reference(lambda v: v.clone().to(device))
    bns = []
    for k, C in (("g", CG), ("0", C0), ("1", C1), ("2", C2)):
        bn = torch.nn.BatchNorm1d(C).to(device)
        with torch.no_grad():
            bn.weight.copy_(P["g" + k]); bn.bias.copy_(P["b" + k]); bn.running_mean.copy_(P["rm" + k]); bn.running_var.copy_(P["rv" + k])
        bn.train(train)
        bns.append(bn)
    W = {k: P[k].to(device).requires_grad_(True) for k in ("Wg", "W0", "W1", "W2", "W3", "b3")}
    xt = lv.to(device).requires_grad_(True)
    assert F.seg_head_supported(xt, B, Npts, W["Wg"], W["W0"], W["W1"], W["W2"], W["W3"])
    steps = tuple((train, 0.1) for _ in bns)
    y = F._SegHead.apply(xt, B, Npts, 0.2, tuple(bns), steps, W["Wg"], bns[0].weight, bns[0].bias, W["W0"], bns[1].weight, bns[1].bias,
                         W["W1"], bns[2].weight, bns[2].bias, W["W2"], bns[3].weight, bns[3].bias, W["W3"], W["b3"])
    y.backward(gout.to(device))
    got = {"Wg": W["Wg"].grad, "gg": bns[0].weight.grad, "bg": bns[0].bias.grad, "W0": W["W0"].grad, "g0": bns[1].weight.grad,
           "b0": bns[1].bias.grad, "W1": W["W1"].grad, "g1": bns[2].weight.grad, "b1": bns[2].bias.grad, "W2": W["W2"].grad,
           "g2": bns[3].weight.grad, "b2": bns[3].bias.grad, "W3": W["W3"].grad, "b3": W["b3"].grad}
    name = "head %s B%d N%d train%d" % ("x".join(map(str, dims)), B, Npts, train)
    scale = float(y64.abs().max())
    e_y = float((y.detach().double() - y64).abs().max()) / scale
    print("PWFAM %-40s logits %.3g (aten %.3g)" % (name, e_y, float((y32.double() - y64).abs().max()) / scale))
    assert e_y <= 1e-4
    with torch.no_grad():       # rows on a max-pool near-tie (fp64 margin below 8 fp32 roundings of the activation) are left out, at most 16
        yg = x64 @ P64["Wg"].t()
        mu, var = (yg.mean(0), yg.var(0, unbiased=False)) if train else (P64["rmg"], P64["rvg"])
        ag = po.lrelu((yg - mu) / torch.sqrt(var + 1e-5) * P64["gg"] + P64["bg"], 0.2).view(B, Npts, -1)
        top2 = ag.topk(2, dim=1)
        margin = top2.values[:, 0] - top2.values[:, 1]
        tie = margin <= 8 * 2.0 ** -24 * top2.values[:, 0].abs().clamp_min(1e-3 * float(ag.abs().max()))
        keep = torch.ones(M, dtype=torch.bool, device=device)
        bidx = torch.arange(B, device=device).view(B, 1).expand_as(tie)
        for q in range(2):
            keep[(bidx * Npts + top2.indices[:, q])[tie]] = False
    assert int((~keep).sum()) <= 16
    e_k, e_a = eo.row_error(xt.grad, gx64, keep), eo.row_error(gx32, gx64, keep)
    print("PWFAM %-40s dlevels per row kernel %.3g  aten %.3g" % (name, e_k, e_a))
    assert e_k <= max(5e-6, 3 * e_a), (e_k, e_a)
    gmax = max(float(v.norm()) for v in gp64.values())
    for k in names:
        if float(gp64[k].norm()) < 1e-6 * gmax:
            continue                                          # mathematically zero: noise on all sides
        e_k, e_a = eo.norm_error(got[k], gp64[k]), eo.norm_error(gp32[k], gp64[k])
        print("PWFAM %-40s d%s kernel %.3g  aten %.3g" % (name, k, e_k, e_a))
        assert e_k <= max(2e-3, 3 * e_a), (k, e_k, e_a)
