"""CPU tests of tests/pt_oracle.py, the conditions that tests/test_pt_family_gpu.py relies on: the fp64 oracle equals the CPU
restatement of the reference layer, the inputs of every case are settled, the prescribed graph rows are what they claim, every
case reaches the path of csrc/pt_attn.hip it is listed for (computed from constants that are checked against the kernel's
text), and the judge can fail: a reference with one tile's edges left out of the parameter sums and of dq, and one with one
in-edge of the hub left out of dk / dv, both miss the bars of the GPU tests by more than 10 x."""
import os
import re

import numpy as np
import pytest
import torch

import pt_oracle as po
import test_pt_family_gpu as fam
from golden_util import fill_state_dict
from oracle import ref_cpu

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fissure-segmentation_amd", "csrc", "pt_attn.hip")


@pytest.mark.parametrize("c,ns,sizes,train", [(32, 8, (50, 37), True), (64, 16, (61, 9), True), (64, 16, (40,), False)])
def test_oracle_equals_restatement(c, ns, sizes, train):
    """with idx from ref_cpu.knnquery, pt_layer in fp64 == oracle/ref_cpu.PTLayer in fp64 to 1e-12 relative: out, the gradient
    of the input features and of every parameter, the running buffers"""
    rng = np.random.default_rng(c + ns)
    n = sum(sizes)
    ref = fill_state_dict(ref_cpu.PTLayer(c, c, 8, ns), 811 + c).double().train(train)
    p = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(np.float32))
    off = torch.from_numpy(np.cumsum(sizes).astype(np.int32))
    idx, _ = ref_cpu.knnquery(ns, p, p, off, off)
    assert torch.equal(idx, po.knn_graph(p.numpy(), sizes, ns))
    g = torch.from_numpy(rng.standard_normal((n, c)))
    x1, x2 = (torch.from_numpy(rng.standard_normal((n, c))).requires_grad_(True) for _ in range(2))
    with torch.no_grad():
        x2.copy_(x1)
    lp, lw = ref.linear_p, ref.linear_w
    mods = dict(lp1=lp[0], bnp=lp[1], lp2=lp[3], bn1=lw[0], lw1=lw[2], bn2=lw[3], lw2=lw[5])
    get = lambda nm: getattr(mods[nm.split("_")[0]], "weight" if nm[-1] in "wg" else "bias")   # noqa: E731
    params = {nm: get(nm).detach().clone().requires_grad_(True) for nm in po.PARAM_NAMES}
    lin = {nm: [getattr(ref, "linear_" + nm).weight.detach().clone().requires_grad_(True),
                getattr(ref, "linear_" + nm).bias.detach().clone().requires_grad_(True)] for nm in "qkv"}
    running = {t + k: getattr(mods[t], "running_mean" if k == "_rm" else "running_var").clone()
               for t in ("bnp", "bn1", "bn2") for k in ("_rm", "_rv")}
    qkv = torch.cat([x2 @ lin[nm][0].t() + lin[nm][1] for nm in "qkv"], 1)
    r = po.pt_layer(p.double(), idx, qkv, params, running, train)
    r["out"].backward(g)
    y = ref([p.double(), x1, off])
    y.backward(g)

    def close(a, b, what):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), what
    close(r["out"].detach(), y.detach(), "out")
    close(x2.grad, x1.grad, "grad x")
    for nm in po.PARAM_NAMES:
        close(params[nm].grad, get(nm).grad, nm)
    for nm in "qkv":
        close(lin[nm][0].grad, getattr(ref, "linear_" + nm).weight.grad, nm)
        close(lin[nm][1].grad, getattr(ref, "linear_" + nm).bias.grad, nm)
    for t in ("bnp", "bn1", "bn2"):
        close(r[t + "_rm"], mods[t].running_mean, t)
        close(r[t + "_rv"], mods[t].running_var, t)
    if train:
        assert float((r["bn1_rm"] - running["bn1_rm"]).abs().max()) > 1e-3      # the buffers did move


@pytest.mark.parametrize("case", po.CASES, ids=po.case_id)
def test_inputs_are_settled(case):
    """a condition on the INPUTS, evaluated with the fp64 oracle alone: no ReLU argument within KINK_MARGIN of 0"""
    inp, rounds = po.case_inputs(case)
    print("PTORACLE %-24s settle rounds %d" % (case[0], rounds))
    assert rounds < po.SETTLE_ROUNDS
    with torch.no_grad():
        r = po.pt_layer(inp["p"], inp["idx"], inp["qkv"], inp["params"], inp["running"], inp["training"])
    assert po.kinks(r) == 0
    assert inp["p"].dtype == inp["qkv"].dtype == torch.float32 and inp["idx"].dtype == torch.int32
    assert int(inp["idx"].min()) >= 0 and int(inp["idx"].max()) < inp["n"] and inp["idx"].shape == (inp["n"], inp["ns"])
    if case[6] == "offset":
        q = inp["qkv"][:, :inp["c"]].double()
        assert float(q.mean(0).abs().min()) > 29 and float(q.std(0).max()) < 0.2
    if case[6] == "sat":
        u2 = r["u2"] - inp["params"]["lw2_b"].double()
        assert 45 <= float(u2.abs().max()) <= 55
        assert float(r["sm"].max()) > 1 - 1e-6                                   # saturated


@pytest.mark.parametrize("n,ns", [(300, 16), (8300, 3), (37, 3), (137, 2), (50, 15), (8, 2)])
def test_prescribed_rows(n, ns):
    idx = po.prescribed_graph(n, ns)
    a = idx.numpy()
    deg = po.in_degree(idx, n)
    assert (a[:, 0] == np.arange(n)).all()
    assert deg[po.HUB] == n // 2 + 1 and (a[0:2 * (n // 2):2, ns - 1] == po.HUB).all()
    assert (deg[n - po.LONELY:] == 1).all() and po.LONELY >= 3                   # nobody but themselves
    assert (a[po.SELF_ROW] == po.SELF_ROW).all()
    if ns >= 3:
        assert a[po.DUP_ROW, 1] == a[po.DUP_ROW, 2]
    assert torch.equal(idx, po.prescribed_graph(n, ns))                          # the same in every case that uses it
    b = po.prescribed_graph(n, ns, self_loop=False)
    degb = po.in_degree(b, n)
    assert (degb[n - po.LONELY:] == 0).all() and degb[po.HUB] == n // 2
    assert (b.numpy()[po.SELF_ROW] == po.SELF_ROW).all()


def test_noself_graph_with_one_neighbour():
    for n in (20, 37):
        b = po.prescribed_graph(n, 1, self_loop=False)
        deg = po.in_degree(b, n)
        assert deg[po.HUB] == n // 2 and (deg[n - po.LONELY:] == 0).all() and int((deg == 0).sum()) >= po.LONELY


def test_mirrored_constants_match_the_kernel_text():
    src = open(SRC).read()
    assert "constexpr int MAXNS = %d;" % po.MAXNS in src
    m = re.search(r"constexpr int pt_gmax\(int c\) \{ return \(c <= 128 \? (\d+) : \(c == 256 \? (\d+) : (\d+)\)\) \* FSG_PT_GMAX_SCALE; \}", src)
    assert m and [int(v) for v in m.groups()] == [po.pt_gmax(128), po.pt_gmax(256), po.pt_gmax(512)]
    assert po.pt_gmax(32) == po.pt_gmax(64) == po.pt_gmax(128)
    assert "#define FSG_PT_GMAX_SCALE 1\n" in src
    assert "static constexpr int NT = C < 256 ? 256 : C;" in src and "static constexpr int PT = NT / C;" in src
    assert [po.points_per_tile(c) for c in po.PLANES] == [8, 4, 2, 1, 1]
    m = re.search(r"inline int edge_grid\(long M\) \{\s*const long b = \(M \+ 255\) / 256;\s*"
                  r"return \(int\)\(b < 1 \? 1 : \(b > (\d+) \? (\d+) : b\)\);", src)
    assert m and int(m.group(1)) == int(m.group(2)) == po.EDGE_GRID_MAX and po.EDGE_BLOCK == 256
    assert "e += (long)gridDim.x * 256" in src
    assert "for (int r = lane; r < R; r += %d)" % po.FINALIZE_LANES in src
    assert src.count("for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x)") == 6
    assert "bool supported_c(int c) { return c == 32 || c == 64 || c == 128 || c == 256 || c == 512; }" in src


def test_each_case_reaches_its_path():
    by = po.CASE_BY_NAME
    for name in po.MULTI_TILE:
        _, c, n, ns = by[name][:4]
        assert po.tiles(c, n) > po.grid(c, n) == po.pt_gmax(c), name            # some workgroup does a second tile
    assert {c for c in po.PLANES} == {by[name][1] for name in po.MULTI_TILE}     # every instantiation
    t, g = po.tiles(512, 300), po.grid(512, 300)
    assert (t, g, t - g, 2 * g - t) == (300, 256, 44, 212)                       # 44 workgroups do two tiles, 212 one
    assert po.tiles(256, 600) == 600 and po.grid(256, 600) == 512
    assert po.tiles(128, 2101) == 1051 and 2101 % po.points_per_tile(128) == 1   # last tile half filled, in the second round
    assert po.tiles(64, 4201) == 1051 and 4201 % po.points_per_tile(64) == 1
    assert po.tiles(32, 8300) == 1038 and 8300 % po.points_per_tile(32) == 4
    M = 8300 * 16
    assert M > po.EDGE_BLOCK * po.EDGE_GRID_MAX and po.edge_grid(M) == 256 > po.FINALIZE_LANES   # strided; 4 finalize rounds
    assert po.grid(32, 8300) > po.FINALIZE_LANES
    assert not by["c256-n600-ns16-eval"][4] and by["c256-n600-ns16-eval"][0] in po.MULTI_TILE
    for name in po.ODD_E:
        _, c, n, ns = by[name][:4]
        assert (po.points_per_tile(c) * ns) % 16 != 0, name
    assert sorted({c[3] for c in po.CASES}) == [1, 2, 3, 4, 5, 7, 8, 15, 16]
    assert all(1 <= c[3] <= po.MAXNS and c[1] in po.PLANES for c in po.CASES)
    # the kNN cases have a segment shorter than ns; in-degree 0 and the hub exist where listed
    assert by["c64-n9-ns16-knn"][2] < by["c64-n9-ns16-knn"][3] and 7 < by["c32-n137-ns16-knn"][3]
    idx = po.case_inputs(by["c64-n300-ns16-noself"])[0]["idx"]
    assert int((po.in_degree(idx, 300) == 0).sum()) >= 3
    idx = po.case_inputs(by["c32-n8300-ns16"])[0]["idx"]
    assert po.in_degree(idx, 8300)[po.HUB] == 4151                               # hundreds of atomics on one row
    assert [c[0] for c in po.CASES if c[2] == 1] == ["c64-n1-ns4-eval"] and not by["c64-n1-ns4-eval"][4]


@pytest.mark.parametrize("name", ["c512-n300-ns16", "c128-n2101-ns8", "c32-n8300-ns16"])
def test_the_judge_can_fail(name):
    """both mutations must exceed the bars of tests/test_pt_family_gpu.py (max(floor, 3 x the fp32 composition's figure, here
    on the CPU)) by at least 10 x"""
    case = po.CASE_BY_NAME[name]
    inp, _ = po.case_inputs(case)
    c, n = inp["c"], inp["n"]
    r64, g64 = po.run(inp, torch.float64, keep_grads=True)
    _, g32 = po.run(inp, torch.float32)
    mags = po.zero_bias_mags(r64, True)
    e_a = po.param_errors(g32, g64, mags)
    row_a = {nm: po.row_error(g32["qkv"][:, i * c:(i + 1) * c], g64["qkv"][:, i * c:(i + 1) * c]) for i, nm in enumerate(("dq", "dk", "dv"))}
    # 1: the second tile of workgroup 0 is dropped
    mut = po.drop_tile(r64, g64, inp, po.grid(c, n))
    e_m = po.param_errors(mut, g64, mags)
    factors = [e_m[nm] / max(fam.PARAM_FLOOR, fam.MARGIN * e_a[nm]) for nm in po.PARAM_NAMES
               if nm not in mags and not nm.startswith("lp1")]
    factors.append(po.row_error(mut["qkv"][:, :c], g64["qkv"][:, :c]) / max(fam.GRAD_ROW_FLOOR, fam.MARGIN * row_a["dq"]))
    print("PTORACLE %-24s dropped tile: misses the bar by %.3g x" % (name, min(factors)))
    assert len(factors) == 11 and min(factors) >= 10
    # 2: one in-edge of the hub is dropped
    mut = po.drop_hub_edge(r64, g64, inp)
    f = [po.row_error(mut["qkv"][:, i * c:(i + 1) * c], g64["qkv"][:, i * c:(i + 1) * c]) /
         max(fam.GRAD_ROW_FLOOR, fam.MARGIN * row_a[nm]) for i, nm in ((1, "dk"), (2, "dv"))]
    print("PTORACLE %-24s dropped hub edge: misses the bar by %.3g x" % (name, min(f)))
    assert min(f) >= 10
    assert fam.PARAM_FLOOR < 3e-3
