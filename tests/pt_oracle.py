"""Oracle, case list and input conditions of the fused PointTransformerLayer (csrc/pt_attn.hip; functional.pt_attn,
fsg_pt_attn_fwd_f32 / fsg_pt_attn_bwd_f32).  Everything here is plain torch / numpy, device-agnostic; no project kernel runs.
Pinned by tests/test_pt_oracle_cpu.py; used by tests/test_pt_family_gpu.py.

pt_layer() is the layer body of models/pointtransformer/seg_model.py:82-92 as ONE function of (p, idx, qkv, the 14 parameters,
the running buffers, training, dtype): the gather, linear_p, w0 = k_j - q_i + p_r, three BatchNorm -> ReLU stages, the softmax
over the neighbours, the shared-plane aggregate.  The BatchNorm is written out (biased batch variance, eps inside the root,
torch's running-buffer rule with the unbiased variance).  In float64 it is the oracle (gradients: autograd on it); in float32
on the GPU it is the ATen yardstick an fp32 implementation's error is held against (edgeconv_oracle.edgeconv_aten_fp32's role).

The inputs are SETTLED: the three ReLUs make the gradients discontinuous and one fp32 flip moves every row by ~1/(n ns) through
the BatchNorm backward sums, so settle() nudges q / p (fp32, ~2e-2 each, fixed seed) until no ReLU argument of the fp64 run lies
within KINK_MARGIN of 0 -- a condition on the inputs; no element is left out of any comparison because of it.

Graphs: every case runs on prescribed_graph() (a hub named by n / 2 rows, three points named by nobody else, a row of self
loops, a duplicated neighbour; the same rows in every case), but the two kNN cases (oracle/c_api.knn_segment on clouds with a
segment shorter than ns) and three that take its variant without the self-loop column: the one listed for in-degree 0, and both
ns = 1 cases -- with one column the self-loop graph is the identity, every d = p_j - p_i is 0 and the first BatchNorm has
zero variance in training.

The mirrored constants below are checked against the text of csrc/pt_attn.hip by tests/test_pt_oracle_cpu.py, and that test
computes from them that every case reaches the path it is listed for.
"""
import zlib

import numpy as np
import torch

from oracle import c_api

PARAM_NAMES = ("lp1_w", "lp1_b", "bnp_g", "bnp_b", "lp2_w", "lp2_b", "bn1_g", "bn1_b", "lw1_w", "lw1_b", "bn2_g", "bn2_b",
               "lw2_w", "lw2_b")
ZERO_BIASES = ("lp1_b", "lw1_b", "lw2_b")     # in front of a train-mode BatchNorm / the softmax: mathematically zero gradient
EPS, MOMENTUM = 1e-5, 0.1
KINK_MARGIN = 1e-4
NUDGE = 2e-2
SETTLE_ROUNDS = 30

# ---- mirrored from csrc/pt_attn.hip
MAXNS = 16                      # :31  constexpr int MAXNS = 16;
EDGE_BLOCK, EDGE_GRID_MAX = 256, 256      # :795-798 edge_grid(): 256-thread blocks, at most 256 of them (pt_stats_p, pt_b4)
FINALIZE_LANES = 64             # :129 pt_bn_finalize_kernel: for (r = lane; r < R; r += 64)
PLANES = (32, 64, 128, 256, 512)


def pt_gmax(c):
    """:36  workgroups per launch at most"""
    return 1024 if c <= 128 else (512 if c == 256 else 256)


def points_per_tile(c):
    """:40-41  Geo<C>::PT = max(256, C) / C"""
    return max(256, c) // c


def tiles(c, n):
    pt = points_per_tile(c)
    return (n + pt - 1) // pt


def grid(c, n):
    """:791-794 grid_for<C>(n)"""
    return min(tiles(c, n), pt_gmax(c))


def edge_grid(M):
    return max(1, min(EDGE_GRID_MAX, (M + EDGE_BLOCK - 1) // EDGE_BLOCK))


# ------------------------------------------------------------------------------------------------------------ the layer
def _bn(x, gamma, beta, rm, rv, training, momentum):
    """BatchNorm over the rows of x (M, L), written out.  -> (z, xhat, mean, invstd, new rm, new rv)"""
    if training:
        M = x.shape[0]
        mean = x.mean(0)
        var = (x - mean).square().mean(0)
        with torch.no_grad():
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * var * (M / (M - 1) if M > 1 else 1.0)
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (x - mean) * invstd
    return xhat * gamma + beta, xhat, mean, invstd, rm, rv


def pt_layer(p, idx, qkv, params, running, training, dtype=torch.float64, momentum=MOMENTUM, keep_grads=False):
    """p (n,3), idx (n,ns) integer, qkv (n,3c) = [q | k | v]; params: dict of the 14 tensors (PARAM_NAMES); running: dict
    bnp_rm, bnp_rv, bn1_rm, ... (not modified); momentum: a number or one per BatchNorm (bnp, bn1, bn2).  All converted to
    `dtype` unless they already have it (leaves that require grad are used as they are).  -> dict of out (n,c) and every
    intermediate: d, a, zp, t, pr, w0, z1, h1, u1, z2, h2, u2, sm (edge tensors (n,ns,.)), stats = (mp, rp, m1, r1, m2, r2),
    hats = (ahat, w0hat, u1hat) and the updated running buffers under their names.  keep_grads: retain_grad() on the edge
    tensors that the mutation tests and the zero-gradient biases need."""
    cv = lambda t: t if t.dtype == dtype else t.to(dtype)   # noqa: E731
    p, qkv = cv(p), cv(qkv)
    P = {k: cv(v) for k, v in params.items()}
    R = {k: cv(v) for k, v in running.items()}
    mom = (momentum,) * 3 if np.isscalar(momentum) else tuple(momentum)
    n, ns = idx.shape
    c = qkv.shape[1] // 3
    cs = c // 8
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    j = idx.long().reshape(-1)
    d = (p[j].view(n, ns, 3) - p.unsqueeze(1)).reshape(n * ns, 3)
    a = d @ P["lp1_w"].t() + P["lp1_b"]
    zp, ahat, mp, rp, rmp, rvp = _bn(a, P["bnp_g"], P["bnp_b"], R["bnp_rm"], R["bnp_rv"], training, mom[0])
    t = torch.relu(zp)
    pr = t @ P["lp2_w"].t() + P["lp2_b"]                                           # (n ns, c)
    w0 = (k[j].view(n, ns, c) - q.unsqueeze(1)).reshape(n * ns, c) + pr
    z1, w0hat, m1, r1, rm1, rv1 = _bn(w0, P["bn1_g"], P["bn1_b"], R["bn1_rm"], R["bn1_rv"], training, mom[1])
    h1 = torch.relu(z1)
    u1 = h1 @ P["lw1_w"].t() + P["lw1_b"]                                          # (n ns, cs)
    z2, u1hat, m2, r2, rm2, rv2 = _bn(u1, P["bn2_g"], P["bn2_b"], R["bn2_rm"], R["bn2_rv"], training, mom[2])
    h2 = torch.relu(z2)
    u2 = h2 @ P["lw2_w"].t() + P["lw2_b"]
    sm = torch.softmax(u2.view(n, ns, cs), 1)
    gv = v[j].view(n, ns, c)
    vp = gv + pr.view(n, ns, c)
    out = (vp.view(n, ns, 8, cs) * sm.unsqueeze(2)).sum(1).reshape(n, c)
    r = dict(out=out, d=d, a=a, zp=zp, t=t, pr=pr, w0=w0, z1=z1, h1=h1, u1=u1, z2=z2, h2=h2, u2=u2, sm=sm, gv=gv,
             stats=(mp, rp, m1, r1, m2, r2), hats=(ahat, w0hat, u1hat),
             bnp_rm=rmp, bnp_rv=rvp, bn1_rm=rm1, bn1_rv=rv1, bn2_rm=rm2, bn2_rv=rv2)
    if keep_grads:
        for name in ("d", "a", "zp", "pr", "w0", "z1", "u1", "z2", "u2", "gv"):
            if r[name].requires_grad:
                r[name].retain_grad()
    return r


def leaves(t, device=None, dtype=None):
    """detached copies of a dict of tensors that require grad"""
    return {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in t.items()}


def run(inp, dtype, device="cpu", momentum=MOMENTUM, keep_grads=False, grad_p=True):
    """forward + backward of pt_layer on a case's inputs -> (result dict, grads dict: p, qkv and the 14 parameters)"""
    L = leaves(dict(p=inp["p"], qkv=inp["qkv"], **inp["params"]), device, dtype)
    p = L["p"] if grad_p else L["p"].detach()
    running = {k: v.to(device) for k, v in inp["running"].items()}
    r = pt_layer(p, inp["idx"].to(device), L["qkv"], {k: L[k] for k in PARAM_NAMES}, running, inp["training"], dtype,
                 momentum, keep_grads)
    r["out"].backward(inp["g"].to(device=device, dtype=dtype))
    grads = {k: v.grad for k, v in L.items() if v.grad is not None}
    return r, grads


# ------------------------------------------------------------------------------------------------------------ graphs
HUB, SELF_ROW, DUP_ROW, LONELY = 1, 3, 5, 3


def knn_graph(p, sizes, ns):
    """the exact kNN graph of the packed clouds (segments of `sizes` points) through oracle/c_api.knn_segment; a segment
    shorter than ns is padded by its rule"""
    off = np.cumsum(np.asarray(sizes)).astype(np.int32)
    idx, _ = c_api.knn_segment(np.asarray(p, np.float32), np.asarray(p, np.float32), off, off, ns)
    return torch.from_numpy(idx.astype(np.int32))


def prescribed_graph(n, ns, self_loop=True, seed=0):
    """int32 (n, ns) graph with prescribed rows (n >= 8; below that a ring, column s names point (i + s) mod n: uniform columns
    may name one of two points three times out of four, which leaves the first BatchNorm three identical samples):
      * column 0 is the point itself (self_loop=False: uniform like the other columns, so some points have in-degree 0);
      * the LONELY = 3 last points are named by no row but, with self_loop, their own;
      * point HUB = 1 is named by the last column of the n // 2 even rows and by nothing else (but its own self loop);
      * row SELF_ROW = 3 lists itself ns times;
      * row DUP_ROW = 5 repeats its column 1 in column 2 (ns >= 3).
    With ns == 1 and self_loop the hub column IS column 0 of the even rows: the self loop gives way there."""
    rng = np.random.default_rng([seed, n, ns])
    if n < 8:
        return torch.from_numpy(((np.arange(n)[:, None] + np.arange(ns)[None, :]) % n).astype(np.int32))
    idx = rng.integers(0, n - LONELY, (n, ns))
    idx[idx == HUB] = HUB + 1
    if self_loop:
        idx[:, 0] = np.arange(n)
    idx[0:2 * (n // 2):2, ns - 1] = HUB
    idx[SELF_ROW, :] = SELF_ROW
    if ns >= 3:
        idx[DUP_ROW, 2] = idx[DUP_ROW, 1]
    return torch.from_numpy(idx.astype(np.int32))


def in_degree(idx, n):
    return np.bincount(idx.numpy().reshape(-1), minlength=n)


# ------------------------------------------------------------------------------------------------------------ the cases
# (name, C, n, ns, training, graph, numeric, what it is for)
CASES = [
    ("c512-n300-ns16", 512, 300, 16, True, "prescribed", None, "300 tiles on 256 workgroups: 44 do two tiles, 212 one"),
    ("c256-n600-ns16", 256, 600, 16, True, "prescribed", None, "600 tiles on 512 workgroups"),
    ("c128-n2101-ns8", 128, 2101, 8, True, "prescribed", None, "1051 tiles on 1024 workgroups, the last one half filled"),
    ("c64-n4201-ns5", 64, 4201, 5, True, "prescribed", None, "1051 tiles, the last has 1 of 4 points, ns odd"),
    ("c32-n8300-ns16", 32, 8300, 16, True, "prescribed", None, "1038 tiles; 132800 edges stride pt_stats_p / pt_b4; 256 records"),
    ("c32-n8300-ns3", 32, 8300, 3, True, "prescribed", None, "the same tiling with E = 24"),
    ("c256-n600-ns16-eval", 256, 600, 16, False, "prescribed", None, "two tiles per workgroup in eval mode (invM = 0)"),
    ("c256-n37-ns3", 256, 37, 3, True, "prescribed", None, "E = 3"),
    ("c512-n20-ns1", 512, 20, 1, True, "noself", None, "ns = 1, PT = 1"),
    ("c64-n37-ns1", 64, 37, 1, True, "noself", None, "ns = 1, E = 4"),
    ("c32-n137-ns2", 32, 137, 2, True, "prescribed", None, "E = 16 from ns = 2"),
    ("c32-n61-ns7", 32, 61, 7, True, "prescribed", None, "E = 56"),
    ("c128-n50-ns15", 128, 50, 15, True, "prescribed", None, "E = 30"),
    ("c64-n9-ns16-knn", 64, 9, 16, True, "knn:9", None, "kNN graph of a segment shorter than ns (padding rule)"),
    ("c32-n137-ns16-knn", 32, 137, 16, True, "knn:130,7", None, "kNN graph, one segment of 7 < ns"),
    ("c64-n300-ns16-noself", 64, 300, 16, True, "noself", None, "column 0 not the self loop: points with in-degree 0"),
    ("c32-n2-ns2", 32, 2, 2, True, "prescribed", None, "two points"),
    ("c64-n1-ns4-eval", 64, 1, 4, False, "prescribed", None, "one point (eval only: in training every variance is zero)"),
    ("c64-n300-ns16-offset", 64, 300, 16, True, "prescribed", "offset", "k, q with a per-channel offset of +-30 on a spread of 0.1"),
    ("c64-n300-ns16-sat", 64, 300, 16, True, "prescribed", "sat", "lw2 scaled until u2 spans +-50: saturated softmax"),
]
MULTI_TILE = ("c512-n300-ns16", "c256-n600-ns16", "c128-n2101-ns8", "c64-n4201-ns5", "c32-n8300-ns16", "c32-n8300-ns3",
              "c256-n600-ns16-eval")
ODD_E = ("c64-n4201-ns5", "c32-n8300-ns3", "c256-n37-ns3", "c512-n20-ns1", "c64-n37-ns1", "c32-n61-ns7", "c128-n50-ns15")
CASE_BY_NAME = {c[0]: c for c in CASES}
SEEDS = {}                       # case name -> seed other than 0 (a case that does not settle gets another seed, not a wider margin)


def case_id(case):
    return case[0]


def raw_inputs(case, seed=None):
    """the unsettled fp32 inputs of a case: dict(p, idx, qkv, params, running, g, training, ...)"""
    name, c, n, ns, training, graph, numeric, _ = case
    seed = SEEDS.get(name, 0) if seed is None else seed
    rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
    cs = c // 8
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    p = f(rng.uniform(-1, 1, (n, 3)))
    qkv = rng.standard_normal((n, 3 * c))
    if numeric == "offset":
        off = 30.0 * rng.choice([-1.0, 1.0], 2 * c)
        qkv[:, :2 * c] = 0.1 * qkv[:, :2 * c] + off
    shapes = dict(lp1_w=(3, 3), lp1_b=(3,), bnp_g=(3,), bnp_b=(3,), lp2_w=(c, 3), lp2_b=(c,), bn1_g=(c,), bn1_b=(c,),
                  lw1_w=(cs, c), lw1_b=(cs,), bn2_g=(cs,), bn2_b=(cs,), lw2_w=(cs, cs), lw2_b=(cs,))
    params = {}
    for k in PARAM_NAMES:                     # golden_util.fill_state_dict's distributions
        sh = shapes[k]
        if k.endswith("_g"):
            v = 0.5 + rng.random(sh)
            v[::5] *= -1.0
        elif len(sh) == 1:
            v = 0.1 * rng.standard_normal(sh)
        else:
            v = rng.standard_normal(sh) / np.sqrt(sh[1])
        params[k] = f(v)
    running = {}
    for tag, L in (("bnp", 3), ("bn1", c), ("bn2", cs)):
        running[tag + "_rm"] = f(0.1 * rng.standard_normal(L))
        running[tag + "_rv"] = f(0.5 + rng.random(L))
    g = f(rng.standard_normal((n, c)))
    if graph.startswith("knn:"):
        idx = knn_graph(p.numpy(), [int(s) for s in graph[4:].split(",")], ns)
    else:
        idx = prescribed_graph(n, ns, self_loop=graph == "prescribed")
    inp = dict(name=name, c=c, n=n, ns=ns, p=p, idx=idx, qkv=f(qkv), params=params, running=running, g=g, training=training)
    if numeric == "sat":
        with torch.no_grad():
            u2 = pt_layer(p, idx, inp["qkv"], params, running, training)["u2"]
        params["lw2_w"] = (params["lw2_w"].double() * (50.0 / float((u2 - params["lw2_b"].double()).abs().max()))).float()
    return inp


def kinks(r, margin=KINK_MARGIN):
    """number of ReLU arguments (zp, z1, z2) of a pt_layer() result within `margin` of 0"""
    return sum(int((r[k].abs() < margin).sum()) for k in ("zp", "z1", "z2"))


def settle(inp, device="cpu"):
    """Move the fp32 inputs off the kinks (in place on copies) -> (inputs, rounds).  Per round, with the fp64 run of the
    current inputs:  a near-kink z1[i,s,ch] nudges q[i,ch];  a near-kink z2[i,s,o] nudges ONE channel of q[i], the open one
    (h1[i,s,ch] > 0) with the largest |Wa[o,ch]| (nudging the whole row would move c ns elements of z1 and make new near-kinks
    as fast as it removes them);  a near-kink zp[i,s,:] nudges p[i].  Near: within 2 KINK_MARGIN; done: none within it."""
    inp = dict(inp, p=inp["p"].clone(), qkv=inp["qkv"].clone())
    ns = inp["ns"]
    rng = np.random.default_rng(12345)
    step = lambda k: torch.from_numpy((NUDGE * (0.5 + rng.random(k)) * rng.choice([-1.0, 1.0], k)).astype(np.float32))  # noqa: E731
    for rounds in range(SETTLE_ROUNDS):
        with torch.no_grad():
            r = pt_layer(inp["p"].to(device), inp["idx"].to(device), inp["qkv"].to(device),
                         {k: v.to(device) for k, v in inp["params"].items()},
                         {k: v.to(device) for k, v in inp["running"].items()}, inp["training"])
        near = {k: (r[k].abs() < 2 * KINK_MARGIN) for k in ("zp", "z1", "z2")}
        if not any(bool(v.any()) for v in near.values()):
            assert kinks(r) == 0
            return inp, rounds
        e, ch = torch.nonzero(near["z1"], as_tuple=True)
        if e.numel():
            pairs = torch.unique(torch.stack([e // ns, ch], 1), dim=0).cpu()
            inp["qkv"][pairs[:, 0], pairs[:, 1]] += step(pairs.shape[0])
        e, o = torch.nonzero(near["z2"], as_tuple=True)
        if e.numel():
            score = inp["params"]["lw1_w"].to(device).double().abs()[o] * (r["h1"][e] > 0)       # (K, c)
            pairs = torch.unique(torch.stack([e // ns, score.argmax(1)], 1), dim=0).cpu()
            inp["qkv"][pairs[:, 0], pairs[:, 1]] += step(pairs.shape[0])
        e = torch.nonzero(near["zp"].any(1), as_tuple=True)[0]
        if e.numel():
            pts = torch.unique(e // ns).cpu()
            inp["p"][pts] += step(pts.numel() * 3).view(-1, 3)
    raise AssertionError("the inputs of %s did not settle within %d rounds: another seed, not a wider margin"
                         % (inp["name"], SETTLE_ROUNDS))


_cache = {}


def case_inputs(case, device="cpu"):
    """the settled inputs of a case (computed once per process) -> (inputs, settle rounds)"""
    if case[0] not in _cache:
        _cache[case[0]] = settle(raw_inputs(case), device)
    return _cache[case[0]]


# ------------------------------------------------------------------------------------------------------------ statistics
def row_error(got, want):
    """edgeconv_oracle.row_error: max over the rows of |got_r - want_r| / (|want_r| + rms row norm of want)"""
    want = want.double()
    rn = want.norm(dim=1)
    return float(((got.double() - want).norm(dim=1) / (rn + rn.pow(2).mean().sqrt()).clamp_min(1e-300)).max())


def norm_error(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300))


def rel_error(got, want):
    """max |got - want| / |want| (stats, running buffers: the kernels carry those sums in double and round once)"""
    want = want.double()
    return float(((got.double() - want).abs() / want.abs().clamp_min(1e-300)).max())


def dp_mags(r, idx):
    """(n,) sum of the absolute summands of each row of dp, from an oracle run with keep_grads (p required grad): every edge
    (i, j) adds +dd to row j and -dd to row i"""
    n, ns = idx.shape
    dd = r["d"].grad.abs().sum(1)
    mag = dd.view(n, ns).sum(1)
    return mag.index_add(0, idx.long().reshape(-1).to(dd.device), dd)


def zero_bias_mags(r, training=True):
    """sum of the absolute summands of the mathematically-zero bias gradients, from an oracle run with keep_grads: lp1_b and
    lw1_b in front of a train-mode BatchNorm, lw2_b in front of the softmax (in eval mode too: the softmax over the neighbours
    does not see a per-channel shift)"""
    mags = {"lw2_b": r["u2"].grad.abs().sum(0)}
    if training:
        mags.update({"lp1_b": r["a"].grad.abs().sum(0), "lw1_b": r["u1"].grad.abs().sum(0)})
    return mags


def param_errors(got, want, mags):
    """figure per parameter gradient: norm_error; the biases in `mags` as max |got - want| / sum |summands|"""
    out = {}
    for k in PARAM_NAMES:
        if k in mags:
            out[k] = float(((got[k].double() - want[k].double()).abs() / mags[k].to(got[k].device).clamp_min(1e-300)).max())
        else:
            out[k] = norm_error(got[k], want[k])
    return out


# ------------------------------------------------------------------------------------------------------------ mutations
def drop_tile(r, grads, inp, tile):
    """the parameter gradients and dq of an oracle run (keep_grads) with the edges of ONE tile (PT consecutive points) left out
    of the sums: what a workgroup that skips its second tile would leave.  -> dict like `grads` (lp1_*: pt_b4 is not tiled)"""
    c, ns = inp["c"], inp["ns"]
    pt = points_per_tile(c)
    lo, hi = tile * pt * ns, min(inp["n"], (tile + 1) * pt) * ns
    e = slice(lo, hi)
    ahat, w0hat, u1hat = r["hats"]
    g = {k: v.clone() for k, v in grads.items()}
    g["lw2_w"] -= r["u2"].grad[e].t() @ r["h2"][e].detach()
    g["lw2_b"] -= r["u2"].grad[e].sum(0)
    g["bn2_g"] -= (r["z2"].grad[e] * u1hat[e].detach()).sum(0)
    g["bn2_b"] -= r["z2"].grad[e].sum(0)
    g["lw1_w"] -= r["u1"].grad[e].t() @ r["h1"][e].detach()
    g["lw1_b"] -= r["u1"].grad[e].sum(0)
    g["bn1_g"] -= (r["z1"].grad[e] * w0hat[e].detach()).sum(0)
    g["bn1_b"] -= r["z1"].grad[e].sum(0)
    g["lp2_w"] -= r["pr"].grad[e].t() @ r["t"][e].detach()
    g["lp2_b"] -= r["pr"].grad[e].sum(0)
    g["bnp_g"] -= (r["zp"].grad[e] * ahat[e].detach()).sum(0)
    g["bnp_b"] -= r["zp"].grad[e].sum(0)
    g["qkv"][tile * pt:(tile + 1) * pt, :c] = 0
    return g


def drop_hub_edge(r, grads, inp):
    """dk / dv with ONE in-edge of the hub (row 0, last column) left out"""
    c, ns = inp["c"], inp["ns"]
    assert int(inp["idx"][0, ns - 1]) == HUB
    g = {k: v.clone() for k, v in grads.items()}
    g["qkv"][HUB, c:2 * c] -= r["w0"].grad[ns - 1]
    g["qkv"][HUB, 2 * c:] -= r["gv"].grad[0, ns - 1]
    return g
