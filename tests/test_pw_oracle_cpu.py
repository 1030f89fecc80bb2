"""Pins tests/pw_oracle.py without a GPU: the oracle members, chained as functional._SegHead chains the kernels, must give the
logits and all 15 gradients of the float64 head by autograd (1e-10 relative); the tie rule; the inputs of every parametrised
random-input rowgemm / tn case of tests/test_pw_family_gpu.py (no element inside the kink margin, selection margins above the fp32 noise); and the
argument checks of fsg_pw_rowgemm_f32 / fsg_pw_tn_f32 / fsg_pw_tn_reduce_f32 that fail before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import pw_oracle as po


def _head_params(KL, CG, C0, C1, C2, CLS, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    P = {"Wg": r(CG, KL) / KL ** 0.5, "W0": r(C0, KL + CG) / (KL + CG) ** 0.5, "W1": r(C1, C0) / C0 ** 0.5, "W2": r(C2, C1) / C1 ** 0.5,
         "W3": r(CLS, C2) / C2 ** 0.5, "b3": r(CLS)}
    for k, C in (("g", CG), ("0", C0), ("1", C1), ("2", C2)):
        P["g" + k] = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
        P["b" + k] = 0.2 * r(C)
        P["rm" + k], P["rv" + k] = 0.3 * r(C), 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    return P


PARAMS = ("Wg", "gg", "bg", "W0", "g0", "b0", "W1", "g1", "b1", "W2", "g2", "b2", "W3", "b3")


@pytest.mark.parametrize("dims,B,Npts", [((64, 128, 64, 64, 32, 3), 3, 128), ((64, 128, 64, 64, 64, 1), 1, 256),
                                         ((128, 256, 128, 64, 64, 8), 5, 512)])
@pytest.mark.parametrize("train", [True, False])
def test_composition_is_the_head(dims, B, Npts, train):
    """oracle members chained as _SegHead.forward / .backward == float64 autograd of the head: logits, d levels, 14 parameter
    gradients and the running statistics to 1e-10 relative (in norm; the statistics of torch's BatchNorm in train mode)"""
    P = _head_params(*dims, seed=7)
    g = torch.Generator().manual_seed(11)
    M = B * Npts
    lv = 0.4 + 0.6 * torch.randn(M, dims[0], generator=g, dtype=torch.float64)
    lv = torch.where(lv < 0, 0.2 * lv, lv)
    gout = torch.randn(M, dims[5], generator=g, dtype=torch.float64)
    Pr = {k: (v.clone().requires_grad_(True) if k in PARAMS else v) for k, v in P.items()}
    x = lv.clone().requires_grad_(True)
    y = po.head_reference_fp64(x, B, Npts, Pr, 0.2, train)
    y.backward(gout)
    mom = 1.0 / 3.0                                          # (not torch's default: pins the oracle's momentum handling)
    out, G, stats = po.head_composed(lv, gout, B, Npts, P, 0.2, train, momentum=mom)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-300))
    assert rel(out, y.detach()) <= 1e-10
    assert rel(G["x"], x.grad) <= 1e-10
    gmax = max(float(Pr[k].grad.norm()) for k in PARAMS)
    for k in PARAMS:
        if float(Pr[k].grad.norm()) < 1e-9 * gmax:          # mathematically zero (e.g. the global-feature layer of a single cloud in
            assert float(G[k].norm()) < 1e-9 * gmax, k      # train mode: a per-batch constant in front of a BatchNorm): rounding on both sides
            continue
        assert rel(G[k], Pr[k].grad) <= 1e-10, (k, rel(G[k], Pr[k].grad))
    if not train:
        return
    # running statistics of all four BatchNorms: torch's update (unbiased variance) on the fp64 pre-BatchNorm activations --
    # layer 0 is the one whose records get the per-cloud shift added
    with torch.no_grad():
        def bn_act(yv, k):
            return po.lrelu((yv - yv.mean(0)) / torch.sqrt(yv.var(0, unbiased=False) + 1e-5) * P["g" + k] + P["b" + k], 0.2)
        pre = {"g": lv @ P["Wg"].t()}
        gf = bn_act(pre["g"], "g").view(B, Npts, -1).max(1)[0]
        pre["0"] = torch.cat([lv, gf.repeat_interleave(Npts, 0)], 1) @ P["W0"].t()
        pre["1"] = bn_act(pre["0"], "0") @ P["W1"].t()
        pre["2"] = bn_act(pre["1"], "1") @ P["W2"].t()
        for k, yv in pre.items():
            assert rel(stats[k][0], (1 - mom) * P["rm" + k] + mom * yv.mean(0)) <= 1e-10, k
            assert rel(stats[k][1], (1 - mom) * P["rv" + k] + mom * yv.var(0, unbiased=True)) <= 1e-10, k


def test_slice_order_is_the_same_value():
    g = np.random.default_rng(3)
    L, R = torch.from_numpy(g.standard_normal((160, 7))), torch.from_numpy(g.standard_normal((160, 5)))
    a, b = po.tn(L, R, ones=1), po.tn(L, R, ones=1, rows_per_slice=64, slice_order=True)
    assert a.shape == (8, 5) and float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    assert torch.allclose(a[7], R.sum(0))


def test_tie_rule_is_lowest_index():
    """rowgemm's sel_arg == argmax with lowest-index ties on an integer-valued input with duplicated rows, both signs"""
    g = np.random.default_rng(5)
    A = g.integers(-8, 9, (256, 32)).astype(np.float64)
    A[5], A[64 + 3], A[200] = A[70], A[70], A[70]            # duplicates inside a tile (64..127) and across tiles
    W = g.integers(-8, 9, (16, 32)).astype(np.float64)
    sgn = np.where(np.arange(16) % 2 == 0, 1.0, -1.0)
    r = po.rowgemm(po.PRO_NONE, po.PW_STORE | po.PW_STATS | po.PW_SEL, 2, torch.from_numpy(A), torch.from_numpy(W), rows_per_cloud=128,
                   sgn=torch.from_numpy(sgn), sel_n=16)
    c = (A @ W.T) * sgn
    for t in range(4):
        blk = c[64 * t:64 * t + 64]
        for n in range(16):
            want = min(i for i in range(64) if blk[i, n] == blk[:, n].max())
            assert int(r["sel_arg"][t, n]) == (64 * t) % 128 + want
            assert float(r["sel_val"][t, n]) == blk[:, n].max()
    assert int((c[64:128] == c[64:128].max(0)).sum(0).max()) >= 2      # the duplicates did make ties
    out, ysel, arg = po.max_finish(r["sel_val"], r["sel_arg"], torch.from_numpy(sgn), torch.ones(16, dtype=torch.float64),
                                   torch.zeros(16, dtype=torch.float64), 2, 2, 0.2)
    cc = torch.from_numpy(c).view(2, 128, 16)
    assert torch.equal(arg.long(), po.argmax_lowest(cc, 1))


def test_the_table_has_the_combinations_the_cases_cover():
    combos = po.instantiated_combinations()
    assert len(combos) == 25 and (0, 7, 1) in combos and (2, 17, 5) in combos
    assert {(c["pro"], c["epi"], c["tile"]) for c in po.rowgemm_cases()} == set(combos)


@pytest.mark.parametrize("case", po.rowgemm_cases(), ids=po.case_id)
def test_rowgemm_case_inputs(case):
    """zero elements inside the kink margin; the random SEL cases have every top-2 margin above the fp32 noise the GPU test
    allows for (a seed that fails is replaced here, not on the GPU)"""
    d = po.rowgemm_inputs(case)
    K1, rpc = case["K1"], case["rpc"]
    if "Y1" in d:
        assert po.kink_count(d["Y1"][:, :K1], d["alpha"], d["delta"], po.KINK_MARGIN, rpc if d["delta"].shape[0] > 1 else 0) == 0
    if "Yp" in d:
        assert po.kink_count(d["Yp"], d["ealpha"], d["edelta"], po.KINK_MARGIN, rpc if d["edelta"].shape[0] > 1 else 0) == 0
    if case["epi"] & po.PW_SEL and case["kind"] in ("a", "b"):      # ('meanshift' rows are near-copies: only sel_val is compared there)
        o = po.rowgemm_oracle(case, d)
        s = torch.where(torch.from_numpy(d["sgn"]) < 0, -1.0, 1.0).double()
        margins = po.selection_margins(o["c"] * s, case["BM"])
        noise = po.SEL_NOISE * o["mag"].view(-1, case["BM"], case["N"]).max(1)[0]
        assert bool((margins > 4 * noise).all()), float((margins / noise).min())


@pytest.mark.parametrize("case", po.tn_cases(), ids=lambda c: c["name"])
def test_tn_case_inputs(case):
    d = po.tn_inputs(case)
    if "LY1" in d:
        assert po.kink_count(d["LY1"][:, :case["N1a"]], d["lalpha"], d["ldelta"], po.KINK_MARGIN,
                             case["rpc"] if d["ldelta"].shape[0] > 1 else 0) == 0
    out, mag = po.tn_oracle(case, d)
    assert out.shape == (case["N1a"] + case["N1b"] + case["ones"], case["N2"]) and bool((mag > 0).all())


def test_builders():
    g = np.random.default_rng(9)
    y = g.standard_normal((300, 40)).astype(np.float32)
    al = (g.uniform(0.5, 1.5, 40) * np.where(np.arange(40) % 2, -1, 1)).astype(np.float32)
    de = g.standard_normal((3, 40)).astype(np.float32)
    assert po.kink_count(y, al, de, 1e-2, 100) > 0
    y2 = po.away_from_kink(y, al, de, 1e-2, 100)
    assert y2.dtype == np.float32 and po.kink_count(y2, al, de, 1e-2, 100) == 0
    assert (y2 != y).sum() < 0.05 * y.size                   # a nudge, not a new input
    w = po.wide_range((4000,), 5, g)
    lg = np.log10(np.abs(w[w != 0]))
    assert w.dtype == np.float32 and lg.max() - np.percentile(lg, 5) > 4
    v = torch.tensor([[1.0, 5.0], [4.0, 5.0], [2.0, -1.0], [0.0, 0.0]], dtype=torch.float64)
    assert torch.equal(po.selection_margins(v, 4), torch.tensor([[2.0, 0.0]], dtype=torch.float64))


def test_entry_points_reject_bad_arguments():
    """the FSG_REQUIREs of check_rowgemm and fsg_pw_tn_f32 that need no device memory: they fail before any launch.  Every pointer
    is the fake address 4096 and is never dereferenced BECAUSE each check fires first -- the pattern of
    test_dgssm_cpu.py::test_ssm_decode_entry_points_reject_bad_arguments; whoever drops or reorders a check in the entry points
    must change the matching case here in the same commit, or it becomes a launch on that address."""
    from fissure_segmentation_amd import _lib
    p = 4096                                                 # 16-byte aligned, never dereferenced
    S, T, SEL, BWD, BIAS = po.PW_STORE, po.PW_STATS, po.PW_SEL, po.PW_BWDSTATS, po.PW_BIAS

    def rg(pro, epi, tile, **kw):
        a = _lib.PWRowGemmArgs()
        base = dict(A1=p, Bimg=p, lda1=32, K1=32, K2=0, M=128, N=64, rows_per_cloud=128, C=p, ldc=64)
        base.update(kw)
        for k, v in base.items():
            setattr(a, k, v)
        _lib.call("fsg_pw_rowgemm_f32", ctypes.byref(a), pro, epi, tile, None)
    with pytest.raises(RuntimeError, match="tile 6 not in 1..5"):
        rg(0, S, 6)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        rg(0, S, 3, A1=None)
    with pytest.raises(RuntimeError, match="bad shape"):
        rg(0, S, 3, K1=48)
    with pytest.raises(RuntimeError, match="bad shape"):
        rg(0, S, 3, lda1=34)
    with pytest.raises(RuntimeError, match="bad segment 2"):
        rg(0, S, 3, K2=32)
    with pytest.raises(RuntimeError, match="prologue tables missing"):
        rg(1, S, 3)
    with pytest.raises(RuntimeError, match="BNBWD needs Y1, P, Q"):
        rg(2, S, 3, alpha=p, delta=p)
    with pytest.raises(RuntimeError, match="STORE needs C"):
        rg(0, S, 3, C=None)
    with pytest.raises(RuntimeError, match="BIAS needs bias"):
        rg(0, S | BIAS, 3)
    with pytest.raises(RuntimeError, match=r"multiples of the tile rows 128"):
        rg(0, S | T, 1, M=192, rec=p)
    with pytest.raises(RuntimeError, match=r"multiples of the tile rows 64"):
        rg(0, S | T, 2, M=128, rows_per_cloud=96, rec=p)
    with pytest.raises(RuntimeError, match="STATS needs rec"):
        rg(0, S | T, 2)
    with pytest.raises(RuntimeError, match="SEL needs"):
        rg(0, S | T | SEL, 2, rec=p, sgn=p, sel_val=p, sel_arg=p, sel_n=0)
    with pytest.raises(RuntimeError, match="BWDSTATS needs"):
        rg(2, S | BWD, 3, alpha=p, delta=p, Y1=p, P=p, Q=p)
    with pytest.raises(RuntimeError, match="per-cloud tables need rows_per_cloud"):
        rg(1, S, 3, alpha=p, delta=p, tstride=32, rows_per_cloud=0)
    with pytest.raises(RuntimeError, match=r"code 3.*prologue 1 / epilogue 9 / tile 3 is not instantiated"):
        rg(1, S | BWD, 3, alpha=p, delta=p, Yp=p, ealpha=p, edelta=p, emu=p, er=p, rec2=p)
    with pytest.raises(RuntimeError, match=r"code 3.*is not instantiated"):
        rg(0, S | T | SEL, 3, rec=p, sgn=p, sel_val=p, sel_arg=p, sel_n=64)

    def tn(tile, ws_short=0, C1=p, C2=None, **kw):
        a = _lib.PWTnArgs()
        base = dict(L1=p, ldl1=64, N1a=64, N1b=0, lpro=0, R=p, ldr=64, N2=64, rpro=0, M=256, rows_per_cloud=128, rows_per_slice=64)
        base.update(kw)
        for k, v in base.items():
            setattr(a, k, v)
        n1 = a.N1a + a.N1b + (1 if a.ones else 0)
        nbytes = _lib.lib.fsg_pw_tn_workspace_bytes(n1, a.N2, a.M, a.rows_per_slice) - ws_short
        _lib.call("fsg_pw_tn_f32", ctypes.byref(a), tile, p, nbytes, C1, 64, C2, 64, None)
    assert _lib.lib.fsg_pw_tn_workspace_bytes(65, 64, 160, 64) == 3 * 65 * 64 * 4
    with pytest.raises(RuntimeError, match="NULL pointer"):
        tn(3, R=None)
    with pytest.raises(RuntimeError, match="bad shape"):
        tn(3, rows_per_slice=48)
    with pytest.raises(RuntimeError, match="two left segments"):
        tn(3, N1a=32, N1b=64, L2=p, C2=p)
    with pytest.raises(RuntimeError, match="two left segments"):
        tn(3, N1b=64, L2=p)                                   # C2 missing
    with pytest.raises(RuntimeError, match="left prologue 2 needs"):
        tn(3, lpro=2)
    with pytest.raises(RuntimeError, match="left prologue 1"):
        tn(3, lpro=1)
    with pytest.raises(RuntimeError, match="right prologue 2"):
        tn(3, rpro=2)
    with pytest.raises(RuntimeError, match=r"per-cloud tables need rows_per_cloud %"):
        tn(3, rpro=1, ralpha=p, rdelta=p, rts=64, rows_per_cloud=96)
    with pytest.raises(RuntimeError, match="workspace too small"):
        tn(3, ws_short=1)
    with pytest.raises(RuntimeError, match="fsg_pw_tn_f32: tile 4"):
        tn(4, rows_per_cloud=0)       # (the tile is looked at last: everything else about this call is valid, nothing is launched)
    jobs = _lib.PWTnReduceJobs()
    jobs.n = 7
    with pytest.raises(RuntimeError, match=r"1\.\.6 jobs"):
        _lib.call("fsg_pw_tn_reduce_f32", ctypes.byref(jobs), None)
    jobs.n = 1
    with pytest.raises(RuntimeError, match="bad job 0"):
        _lib.call("fsg_pw_tn_reduce_f32", ctypes.byref(jobs), None)
