"""Plain float64 statements of every member of the point-wise head family (csrc/pointwise.hip), written from the contract in
include/fsg_hip.h (the block "The members of the family behind the fused DGCNN head") and not from the kernel source: torch
ops only, no kernels.  tests/test_pw_oracle_cpu.py chains them the way functional._SegHead does and compares with float64
autograd of the head, which is what makes them a reference; tests/test_pw_family_gpu.py compares the kernels with them.

Conventions: all tensors float64 unless they are indices; `alpha`, `Q`, `er`, `ealpha` are per-channel vectors; `delta`, `P`,
`edelta`, `emu` are (nb, K) tables with one row per cloud when the matching stride argument is non-zero and one row otherwise
(a 1-D vector is accepted for the one-row form).  Operands with a prologue also return `mag`, the sum of the absolute operand
magnitudes a product is measured against (|alpha A1| + |delta| for prologue 1, |alpha A1| + |P| + |Q Y1| for prologue 2).
"""
import os
import re

import numpy as np
import torch

PW_STORE, PW_STATS, PW_SEL, PW_BWDSTATS, PW_BIAS = 1, 2, 4, 8, 16
PRO_NONE, PRO_BNACT, PRO_BNBWD = 0, 1, 2
MAX_REDUCE_JOBS = 6

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fissure-segmentation_amd", "csrc", "pointwise.hip")


def tile_rows(tile):
    """fsg_pw_tile_rows: rows of C per workgroup"""
    return 128 if tile in (1, 4) else 64


def tile_cols(tile):
    """columns of C per workgroup (tile codes of fsg_pw_rowgemm_f32)"""
    return {1: 128, 2: 128, 3: 64, 4: 64, 5: 192}[tile]


def instantiated_combinations():
    """every (prologue, epilogue, tile) that fsg_pw_rowgemm_f32 dispatches: the PW_CASE table of csrc/pointwise.hip plus the
    one combination written out as a plain `case` (the single-buffered 128 x 128 STORE | STATS | SEL product)"""
    names = {"PRO_NONE": 0, "PRO_BNACT": 1, "PRO_BNBWD": 2, "PW_STORE": 1, "PW_STATS": 2, "PW_SEL": 4, "PW_BWDSTATS": 8, "PW_BIAS": 16}
    text = open(_SRC).read()
    body = text[text.index('extern "C" int fsg_pw_rowgemm_f32'):text.index("#undef PW_CASE")]

    def epi_of(s):
        return sum(names[t.strip()] for t in s.strip("() ").split("|"))
    out = []
    for m in re.finditer(r"^\s*PW_CASE\((PRO_\w+),\s*([^,]+),\s*(\d),\s*\d,\s*\d\);", body, re.M):
        out.append((names[m.group(1)], epi_of(m.group(2)), int(m.group(3))))
    for m in re.finditer(r"^\s*case (PRO_\w+) \* 1000 \+ (\([^)]*\)|\w+) \* 10 \+ (\d):", body, re.M):
        out.append((names[m.group(1)], epi_of(m.group(2)), int(m.group(3))))
    assert len(set(out)) == len(out)
    return sorted(out)


# --------------------------------------------------------------------------------------------------------------------- prologues

def lrelu(u, slope):
    return torch.where(u > 0, u, u * slope)


def dlrelu(u, slope):
    return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))


def table_rows(tab, M, rows_per_cloud, stride):
    """the row of a per-cloud table that every one of the M rows reads: cloud(m) = m / rows_per_cloud; stride 0 = row 0 for all"""
    tab = tab.reshape(1, -1) if tab.dim() == 1 else tab
    if stride == 0:
        return tab[:1]
    assert rows_per_cloud > 0
    return tab[torch.arange(M, device=tab.device) // rows_per_cloud]


def pro_none(A1, Y1=None, alpha=None, delta=None, P=None, Q=None, tstride=0, rows_per_cloud=0, slope=0.0):
    return A1, A1.abs()


def pro_bnact(A1, Y1=None, alpha=None, delta=None, P=None, Q=None, tstride=0, rows_per_cloud=0, slope=0.0):
    """a = lrelu(alpha[k] A1[m,k] + delta[cloud(m)][k])"""
    d = table_rows(delta, A1.shape[0], rows_per_cloud, tstride)
    return lrelu(alpha * A1 + d, slope), (alpha * A1).abs() + d.abs()


def pro_bnbwd(A1, Y1, alpha, delta, P, Q, tstride=0, rows_per_cloud=0, slope=0.0):
    """a = alpha[k] A1[m,k] f'(alpha[k] Y1[m,k] + delta[cloud][k]) - P[cloud][k] - Q[k] Y1[m,k]"""
    M = A1.shape[0]
    d, p = table_rows(delta, M, rows_per_cloud, tstride), table_rows(P, M, rows_per_cloud, tstride)
    a = alpha * A1 * dlrelu(alpha * Y1 + d, slope) - p - Q * Y1
    return a, (alpha * A1).abs() + p.abs() + (Q * Y1).abs()


PROLOGUES = {PRO_NONE: pro_none, PRO_BNACT: pro_bnact, PRO_BNBWD: pro_bnbwd}


def argmax_lowest(v, dim):
    """argmax along `dim`, the lowest index among equal maxima (stated explicitly: torch.argmax makes no promise)"""
    mx = v.max(dim, keepdim=True)[0]
    n = v.shape[dim]
    shape = [1] * v.dim()
    shape[dim] = n
    idx = torch.arange(n, device=v.device).view(shape).expand_as(v)
    return torch.where(v == mx, idx, torch.full_like(idx, n)).min(dim)[0]


# --------------------------------------------------------------------------------------------------------------------- products

def rowgemm(pro, epi, tile, A1, W, Y1=None, A2=None, alpha=None, delta=None, P=None, Q=None, tstride=0, rows_per_cloud=0, slope=0.0,
            store_n0=0, bias=None, sgn=None, sel_n=0, Yp=None, ealpha=None, edelta=None, emu=None, er=None, etstride=0):
    """fsg_pw_rowgemm_f32 with the weight W (N, K1 + K2) instead of its image.  Returns a dict:
    c (M, N) the product before the epilogue and mag (M, N) its sum of absolute operand magnitudes (+ |bias|);
    C (M, N - store_n0) what is stored; rec (R, 3, N) = (n, mean, M2) per tile of tile_rows(tile) rows; sel_val / sel_arg
    (R, sel_n): max of sgn * c over the tile and its row inside the cloud, lowest row on ties; rec2 (R, 2, N): sums over the tile
    of h = c f'(ealpha Yp + edelta[cloud]) and h (Yp - emu[cloud]) er, with rec2_mag the sums of their absolute summands."""
    M, K1 = A1.shape
    a, amag = PROLOGUES[pro](A1, Y1, alpha, delta, P, Q, tstride, rows_per_cloud, slope)
    if A2 is not None:
        a, amag = torch.cat([a, A2], 1), torch.cat([amag, A2.abs()], 1)
    c, mag = a @ W.t(), amag @ W.abs().t()
    N = W.shape[0]
    out = {"c": c}
    BM = tile_rows(tile)
    if epi & PW_STORE:
        st = c + bias if epi & PW_BIAS else c
        out["C"] = st[:, store_n0:]
        if epi & PW_BIAS:
            mag = mag + bias.abs()
    out["mag"] = mag
    if epi & (PW_STATS | PW_SEL | PW_BWDSTATS):
        assert M % BM == 0
        R = M // BM
        ct = c.view(R, BM, N)
    if epi & PW_STATS:
        mean = ct.mean(1)
        d = ct - mean[:, None]
        out["rec"] = torch.stack([torch.full_like(mean, BM), mean, d.pow(2).sum(1)], 1)
        mt = mag.view(R, BM, N)
        out["rec_mag"] = torch.stack([torch.ones_like(mean), mt.mean(1), (d.pow(2) + 2 * d.abs() * mt).sum(1)], 1)
    if epi & PW_SEL:
        s = torch.where(sgn[:sel_n] < 0, -1.0, 1.0).to(c.dtype)
        v = ct[:, :, :sel_n] * s
        row = argmax_lowest(v, 1)
        out["sel_val"] = v.max(1)[0]
        first = torch.arange(R, device=c.device)[:, None] * BM
        out["sel_arg"] = (first % rows_per_cloud + row).to(torch.int32)
    if epi & PW_BWDSTATS:
        de, mu = table_rows(edelta, M, rows_per_cloud, etstride), table_rows(emu, M, rows_per_cloud, etstride)
        fp = dlrelu(ealpha * Yp + de, slope)
        yh = (Yp - mu) * er
        h = c * fp
        out["rec2"] = torch.stack([h.view(R, BM, N).sum(1), (h * yh).view(R, BM, N).sum(1)], 1)
        hm = mag * fp.abs()
        out["rec2_mag"] = torch.stack([hm.view(R, BM, N).sum(1), (hm * yh.abs()).view(R, BM, N).sum(1)], 1)
    return out


def tn(L1, R, LY1=None, L2=None, lpro=PRO_NONE, lalpha=None, ldelta=None, lP=None, lQ=None, lts=0, rpro=PRO_NONE, ralpha=None,
       rdelta=None, rts=0, slope=0.0, rows_per_cloud=0, rows_per_slice=0, ones=0, slice_order=False, with_mag=False):
    """fsg_pw_tn_f32: [C1 ; C2] (N1a + N1b + ones, N2) = sum_m L'(m, :)^T R'(m, :) with L' = [pro(L1) | L2 | 1].
    slice_order=True: the partial products of the row slices, summed slice by slice (the same value in float64; kept because it
    is how the contract states the sum)."""
    left, lmag = PROLOGUES[lpro](L1, LY1, lalpha, ldelta, lP, lQ, lts, rows_per_cloud, slope)
    right, rmag = PROLOGUES[rpro](R, None, ralpha, rdelta, None, None, rts, rows_per_cloud, slope)
    if L2 is not None:
        left, lmag = torch.cat([left, L2], 1), torch.cat([lmag, L2.abs()], 1)
    if ones:
        o = torch.ones(left.shape[0], 1, dtype=left.dtype, device=left.device)
        left, lmag = torch.cat([left, o], 1), torch.cat([lmag, o], 1)
    if slice_order:
        assert rows_per_slice > 0
        out = torch.zeros(left.shape[1], right.shape[1], dtype=left.dtype, device=left.device)
        for m0 in range(0, left.shape[0], rows_per_slice):
            out = out + left[m0:m0 + rows_per_slice].t() @ right[m0:m0 + rows_per_slice]
    else:
        out = left.t() @ right
    return (out, lmag.t() @ rmag) if with_mag else out


# --------------------------------------------------------------------------------------------------------------------- tables

def bn_finalize(rec, c0, C, B, training, gamma, beta, eps, momentum=0.1, shift=None, running_mean=None, running_var=None, mean=None,
                invstd=None, gfeat=None, Wglob=None, want_emu=False, want_cloud_mean=False):
    """fsg_pw_bn_finalize_f32 on STATS records rec (R, 3, ldn), columns [c0, c0 + C).  gfeat (B, CG) + Wglob (C, CG): the shift
    is gfeat Wglob^T, formed here.  training == 0: `mean` / `invstd` are inputs.  Returns a dict with mean, invstd, running_mean,
    running_var (None when not given), alpha, delta (B or 1, C), emu, cloud_mean, shift."""
    out = {"shift": shift, "running_mean": running_mean, "running_var": running_var, "emu": None, "cloud_mean": None}
    if gfeat is not None:
        shift = gfeat @ Wglob.t()
        out["shift"] = shift
    if training:
        R = rec.shape[0]
        n, mu, M2 = (rec[:, i, c0:c0 + C] for i in range(3))
        if shift is not None:
            mu = mu + shift.repeat_interleave(R // B, 0)
        tot = n.sum(0)
        mean = (n * mu).sum(0) / tot
        var = ((M2 + n * (mu - mean).pow(2)).sum(0) / tot).clamp_min(0)
        invstd = 1.0 / torch.sqrt(var + eps)
        if running_mean is not None:
            unbiased = var * tot / (tot - 1)
            out["running_mean"] = (1 - momentum) * running_mean + momentum * mean
            out["running_var"] = (1 - momentum) * running_var + momentum * unbiased
        if want_cloud_mean:
            nr, mr = rec[:, 0, c0:c0 + C].reshape(B, R // B, C), rec[:, 1, c0:c0 + C].reshape(B, R // B, C)
            out["cloud_mean"] = (nr * mr).sum(1) / nr.sum(1)
    alpha = gamma * invstd
    sh = shift if shift is not None else torch.zeros(1, C, dtype=alpha.dtype, device=alpha.device)
    out.update(mean=mean, invstd=invstd, alpha=alpha, delta=alpha * (sh - mean) + beta)
    if want_emu:
        out["emu"] = mean - sh
    return out


def max_finish(sel_val, sel_arg, sgn, alpha, delta, B, tiles, slope):
    """fsg_pw_max_finish_f32: SEL records (B * tiles, C) -> out (B, C) = lrelu(alpha ysel + delta), ysel, arg (lowest row on ties)"""
    C = sel_val.shape[1]
    v, a = sel_val.view(B, tiles, C), sel_arg.view(B, tiles, C).long()
    best = v.max(1)[0]
    arg = torch.where(v == best[:, None], a, torch.full_like(a, 2 ** 31 - 1)).min(1)[0]
    ysel = torch.where(sgn < 0, -1.0, 1.0).to(v.dtype) * best
    return lrelu(alpha * ysel + delta.reshape(1, C), slope), ysel, arg.to(torch.int32)


def cloud_linear(x, W):
    """fsg_pw_cloud_linear_f32: out (B, C0) = x (B, CG) W^T"""
    return x @ W.t()


def bnbwd_finalize(rec2, B, M, training, alpha, invstd, emu, emu_per_cloud, cloud_mean=None, want_dc=False):
    """fsg_pw_bnbwd_finalize_f32: BWDSTATS records (R, 2, C) -> dbeta, dgamma, P (B or 1, C), Q (C) of prologue 2 (so that
    dy = alpha h - P - Q y is the BatchNorm backward: Q = alpha r dgamma / M, P = alpha (dbeta / M - emu r dgamma / M); all zero
    in eval mode), dc (B, C) = per-cloud column sums of dy."""
    R, _, C = rec2.shape
    dbeta, dgamma = rec2[:, 0].sum(0), rec2[:, 1].sum(0)
    db, dg = (dbeta / M, dgamma / M * invstd) if training else (torch.zeros_like(dbeta), torch.zeros_like(dgamma))
    Q = alpha * dg
    e = emu.reshape(-1, C)[:B if emu_per_cloud else 1]
    P = alpha * (db - e * dg)
    dc = None
    if want_dc:
        nb = M // B
        dc = alpha * rec2[:, 0].reshape(B, R // B, C).sum(1) - nb * P - Q * nb * cloud_mean
    return dbeta, dgamma, P, Q, dc


def logits_bwd(g, W3, y, alpha, delta, mean, invstd, slope):
    """fsg_pw_logits_bwd_f32: da (M, C) = g (M, classes) W3 and the BWDSTATS records (ceil(M / 32), 2, C) of the BatchNorm in front;
    also returns the sums of absolute summands of da and of the records"""
    M, C = y.shape
    da, mag = g @ W3, g.abs() @ W3.abs()
    fp = dlrelu(alpha * y + delta.reshape(1, C), slope)
    yh = (y - mean) * invstd
    R = (M + 31) // 32
    pad = R * 32 - M

    def blocks(t):
        return torch.nn.functional.pad(t, (0, 0, 0, pad)).view(R, 32, C).sum(1)
    h, hm = da * fp, mag * fp.abs()
    return da, torch.stack([blocks(h), blocks(h * yh)], 1), mag, torch.stack([blocks(hm), blocks(hm * yh.abs())], 1)


def gf_prep(ysel, alpha, delta, mean, invstd, M, training, slope, dg=None, dc=None, W0g=None, gfeat=None, W=None):
    """fsg_pw_gf_prep_f32.  Either dg (B, C) is given, or dc (B, C0) with W0g (C0, C) and gfeat (B, C): dg = dc W0g and
    dW0g = dc^T gfeat.  W (C, K) given: also Wq = [Q o W | -P] (C, K + 1).  Returns a dict."""
    out = {"dW0g": None, "Wq": None}
    if dc is not None:
        dg = dc @ W0g
        out["dW0g"] = dc.t() @ gfeat
    h = dg * dlrelu(alpha * ysel + delta.reshape(1, -1), slope)
    dbeta, dgamma = h.sum(0), (h * (ysel - mean) * invstd).sum(0)
    db, dgm = (dbeta / M, dgamma / M * invstd) if training else (torch.zeros_like(dbeta), torch.zeros_like(dgamma))
    Q, P = alpha * dgm, alpha * (db - mean * dgm)
    out.update(dg=dg, dbeta=dbeta, dgamma=dgamma, P=P, Q=Q, coef=alpha * h)
    if W is not None:
        out["Wq"] = torch.cat([Q[:, None] * W, -P[:, None]], 1)
    # sums of absolute summands of every output (what an error of it is measured against)
    dgm = dc.abs() @ W0g.abs() if dc is not None else dg.abs()
    hm = dgm * dlrelu(alpha * ysel + delta.reshape(1, -1), slope).abs()
    bm, gm = hm.sum(0), (hm * (ysel - mean).abs() * invstd).sum(0)
    Qm, Pm = alpha.abs() * gm / M * invstd, alpha.abs() * (bm / M + mean.abs() * gm / M * invstd)
    mag = dict(dg=dgm, dbeta=bm, dgamma=gm, Q=Qm, P=Pm, coef=alpha.abs() * hm)
    if dc is not None:
        mag["dW0g"] = dc.abs().t() @ gfeat.abs()
    if W is not None:
        mag["Wq"] = torch.cat([Qm[:, None] * W.abs(), Pm[:, None]], 1)
    out["mag"] = mag
    return out


def scatter_rows(dX, coef, arg, W, Npts):
    """fsg_pw_scatter_rows_f32: dX[b Npts + arg[b,c], :] += coef[b,c] W[c, :]"""
    B, C = coef.shape
    rows = (torch.arange(B, device=dX.device)[:, None] * Npts + arg.long()).reshape(-1)
    return dX.index_add(0, rows, (coef[:, :, None] * W[None]).reshape(B * C, -1))


def gf_dw(coef, arg, X, s, W, G, P, Q, Npts):
    """fsg_pw_gf_dw_f32: dW[c, :] = sum_b coef[b,c] X[b Npts + arg[b,c], :] - P[c] s - Q[c] (W G)[c, :]"""
    B, C = coef.shape
    rows = torch.arange(B, device=X.device)[:, None] * Npts + arg.long()
    return (coef[:, :, None] * X[rows]).sum(0) - P[:, None] * s[None] - Q[:, None] * (W @ G)


# --------------------------------------------------------------------------------------------------------------------- the head

def head_reference_fp64(levels, B, Npts, P, slope, train, eps=1e-5):
    """models/dgcnn.py:123-162 of the reference on point-major rows in float64 torch ops (the same statement as
    test_gpu_parity._head_reference_fp64, restated here so that the CPU tests need nothing from a GPU module)"""
    def bn(y, g, b, rm, rv):
        mu, var = (y.mean(0), y.var(0, unbiased=False)) if train else (rm, rv)
        return (y - mu) / torch.sqrt(var + eps) * g + b
    yg = lrelu(bn(levels @ P["Wg"].t(), P["gg"], P["bg"], P["rmg"], P["rvg"]), slope)
    g = yg.view(B, Npts, -1).max(1)[0]
    x = torch.cat([levels, g.repeat_interleave(Npts, 0)], 1)
    y = lrelu(bn(x @ P["W0"].t(), P["g0"], P["b0"], P["rm0"], P["rv0"]), slope)
    y = lrelu(bn(y @ P["W1"].t(), P["g1"], P["b1"], P["rm1"], P["rv1"]), slope)
    y = lrelu(bn(y @ P["W2"].t(), P["g2"], P["b2"], P["rm2"], P["rv2"]), slope)
    return y @ P["W3"].t() + P["b3"]


def head_composed(levels, gout, B, Npts, P, slope, train, eps=1e-5, momentum=0.1):
    """The oracle members chained exactly as functional._SegHead.forward / .backward chain the kernels (same tiles, same
    tables, same Gram form of the global-feature backward).  P as for head_reference_fp64.  Returns (logits, grads dict with
    'x' and the 14 parameter names, running statistics dict)."""
    M, KL = levels.shape
    Wg, W0, W1, W2, W3 = P["Wg"], P["W0"], P["W1"], P["W2"], P["W3"]
    CG, C0, C1, C2 = Wg.shape[0], W0.shape[0], W1.shape[0], W2.shape[0]
    S, T, SEL, BWD, BIAS = PW_STORE, PW_STATS, PW_SEL, PW_BWDSTATS, PW_BIAS

    def stats_in(k):
        return dict(mean=P["rm" + k], invstd=1.0 / torch.sqrt(P["rv" + k] + eps)) if not train else \
            dict(running_mean=P["rm" + k], running_var=P["rv" + k])
    r0 = rowgemm(PRO_NONE, S | T | SEL, 1, levels, torch.cat([Wg, W0[:, :KL]], 0), rows_per_cloud=Npts, store_n0=CG, sgn=P["gg"], sel_n=CG)
    y0, rec0 = r0["C"], r0["rec"]
    fg = bn_finalize(rec0, 0, CG, B, train, P["gg"], P["bg"], eps, momentum, **stats_in("g"))
    g, ysel, arg = max_finish(r0["sel_val"], r0["sel_arg"], P["gg"], fg["alpha"], fg["delta"], B, Npts // 128, slope)
    c = cloud_linear(g, W0[:, KL:])
    f0 = bn_finalize(rec0, CG, C0, B, train, P["g0"], P["b0"], eps, momentum, shift=c, want_emu=True, want_cloud_mean=True, **stats_in("0"))
    r1 = rowgemm(PRO_BNACT, S | T, 2, y0, W1, alpha=f0["alpha"], delta=f0["delta"], tstride=C0, rows_per_cloud=Npts, slope=slope)
    y1 = r1["C"]
    f1 = bn_finalize(r1["rec"], 0, C1, B, train, P["g1"], P["b1"], eps, momentum, **stats_in("1"))
    r2 = rowgemm(PRO_BNACT, S | T, 3, y1, W2, alpha=f1["alpha"], delta=f1["delta"], rows_per_cloud=Npts, slope=slope)
    y2 = r2["C"]
    f2 = bn_finalize(r2["rec"], 0, C2, B, train, P["g2"], P["b2"], eps, momentum, **stats_in("2"))
    out = rowgemm(PRO_BNACT, S | BIAS, 3, y2, W3, alpha=f2["alpha"], delta=f2["delta"], rows_per_cloud=Npts, slope=slope, bias=P["b3"])["C"]
    cm_0 = f0["cloud_mean"] if f0["cloud_mean"] is not None else torch.zeros(B, C0, dtype=levels.dtype)
    # ---- backward
    G = {"b3": gout.sum(0)}
    G["W3"] = tn(gout, y2, rpro=PRO_BNACT, ralpha=f2["alpha"], rdelta=f2["delta"], slope=slope, rows_per_cloud=Npts, rows_per_slice=128)
    da2, r2b, _, _ = logits_bwd(gout, W3, y2, f2["alpha"], f2["delta"], f2["mean"], f2["invstd"], slope)
    G["b2"], G["g2"], P2, Q2, _ = bnbwd_finalize(r2b, B, M, train, f2["alpha"], f2["invstd"], f2["mean"], False)
    bw2 = dict(lpro=PRO_BNBWD, lalpha=f2["alpha"], ldelta=f2["delta"], lP=P2, lQ=Q2)
    G["W2"] = tn(da2, y1, LY1=y2, rpro=PRO_BNACT, ralpha=f1["alpha"], rdelta=f1["delta"], slope=slope, rows_per_cloud=Npts, **bw2)
    q1 = rowgemm(PRO_BNBWD, S | BWD, 2, da2, W2.t(), Y1=y2, alpha=f2["alpha"], delta=f2["delta"], P=P2, Q=Q2, rows_per_cloud=Npts,
                 slope=slope, Yp=y1, ealpha=f1["alpha"], edelta=f1["delta"], emu=f1["mean"], er=f1["invstd"])
    da1 = q1["C"]
    G["b1"], G["g1"], P1, Q1, _ = bnbwd_finalize(q1["rec2"], B, M, train, f1["alpha"], f1["invstd"], f1["mean"], False)
    bw1 = dict(lpro=PRO_BNBWD, lalpha=f1["alpha"], ldelta=f1["delta"], lP=P1, lQ=Q1)
    G["W1"] = tn(da1, y0, LY1=y1, rpro=PRO_BNACT, ralpha=f0["alpha"], rdelta=f0["delta"], rts=C0, slope=slope, rows_per_cloud=Npts, **bw1)
    q0 = rowgemm(PRO_BNBWD, S | BWD, 2, da1, W1.t(), Y1=y1, alpha=f1["alpha"], delta=f1["delta"], P=P1, Q=Q1, rows_per_cloud=Npts,
                 slope=slope, Yp=y0, ealpha=f0["alpha"], edelta=f0["delta"], emu=f0["emu"], er=f0["invstd"], etstride=C0)
    da0 = q0["C"]
    G["b0"], G["g0"], P0, Q0, dc = bnbwd_finalize(q0["rec2"], B, M, train, f0["alpha"], f0["invstd"], f0["emu"], True, cm_0, True)
    pg = gf_prep(ysel, fg["alpha"], fg["delta"], fg["mean"], fg["invstd"], M, train, slope, dc=dc, W0g=W0[:, KL:], gfeat=g, W=Wg)
    G["bg"], G["gg"] = pg["dbeta"], pg["dgamma"]
    m1n = tn(pg["Wq"], Wg)                                       # [M1 ; npvec] = [Q o Wg | -P]^T Wg
    M1, npvec = m1n[:KL], m1n[KL]
    bw0 = dict(lpro=PRO_BNBWD, lalpha=f0["alpha"], ldelta=f0["delta"], lP=P0, lQ=Q0, lts=C0)
    big = tn(da0, levels, LY1=y0, L2=levels, ones=1, slope=slope, rows_per_cloud=Npts, **bw0)   # [dW0_levels ; G ; s]
    G["W0"] = torch.cat([big[:C0], pg["dW0g"]], 1)
    Gram, s = big[C0:C0 + KL], big[C0 + KL]
    dlv = rowgemm(PRO_BNBWD, S | BIAS, 4, da0, torch.cat([W0[:, :KL].t(), -M1], 1), Y1=y0, A2=levels, alpha=f0["alpha"], delta=f0["delta"],
                  P=P0, Q=Q0, tstride=C0, rows_per_cloud=Npts, slope=slope, bias=npvec)["C"]
    G["x"] = scatter_rows(dlv, pg["coef"], arg, Wg, Npts)
    G["Wg"] = gf_dw(pg["coef"], arg, levels, s, Wg, Gram, pg["P"], pg["Q"], Npts)
    stats = {k: (f["running_mean"], f["running_var"]) for k, f in (("g", fg), ("0", f0), ("1", f1), ("2", f2))}
    return out, G, stats


# --------------------------------------------------------------------------------------------------------------------- inputs

def wide_range(shape, decades, rng, lo=-3.0):
    """float32 values with log-uniform magnitudes over `decades` decades starting at 10^lo and normal mantissas (what
    test_pw_linear_is_fp32_grade uses: all three bf16 pieces of an operand carry weight)"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(lo, lo + decades, shape)).astype(np.float32)


def away_from_kink(Y, alpha, delta, margin, rows_per_cloud=0):
    """float32 copy of Y with the pre-BatchNorm values nudged so that no |alpha y + delta[cloud]| lies within `margin` of 0 (the
    derivative of LeakyReLU jumps there: an fp32 evaluation may legitimately land on the other side).  alpha must be non-zero.
    delta: (K,) or one row per cloud of rows_per_cloud rows."""
    Y = np.array(Y, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    d = np.asarray(delta, dtype=np.float64).reshape(-1, Y.shape[1])
    d = d[np.arange(Y.shape[0]) // rows_per_cloud] if d.shape[0] > 1 else d
    u = alpha * Y + d
    near = np.abs(u) < 2 * margin
    target = np.where(u >= 0, 3.0 * margin, -3.0 * margin)
    Y = np.where(near, (target - d) / alpha, Y).astype(np.float32)
    return Y


def kink_count(Y, alpha, delta, margin, rows_per_cloud=0):
    """number of elements of (float32) Y with |alpha y + delta[cloud]| < margin, evaluated in float64"""
    Y, alpha = np.asarray(Y, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    d = np.asarray(delta, dtype=np.float64).reshape(-1, Y.shape[1])
    d = d[np.arange(Y.shape[0]) // rows_per_cloud] if d.shape[0] > 1 else d
    return int((np.abs(alpha * Y + d) < margin).sum())


def selection_margins(v, group_rows):
    """v (M, N) float64 (already multiplied by the sign): the top-2 gap of every (group of `group_rows` rows, column) -> (M / group_rows, N)"""
    t = v.view(-1, group_rows, v.shape[1]).topk(2, dim=1).values
    return t[:, 0] - t[:, 1]


# --------------------------------------------------------------------------------------------------------------------- cases
# The random-input rowgemm and tn cases of tests/test_pw_family_gpu.py are generated here, so that tests/test_pw_oracle_cpu.py can pin their
# inputs (no element inside the kink margin, selection margins above the fp32 noise) without a GPU.

KINK_MARGIN = 1e-3        # |alpha y + delta| of every element whose LeakyReLU derivative is taken; the inputs are O(1)
SEL_NOISE = 8 * 2.0 ** -24  # x the sum of absolute summands of the winner: the fp32 noise a selection margin must exceed
                            # (the head test's "8 roundings of its magnitude")


def rowgemm_cases():
    """dicts (pro, epi, tile, kind, rpc (rows per cloud), M, K1, K2, N, per_cloud, slope, seed) for every instantiated combination:
    kind 'a': rows_per_cloud = 2 BM, K1 = 32, N = 64 + 13, one-row tables, slope 0.2, second segment of 64 where there is one;
    kind 'b': rows_per_cloud = BM, K1 = 96, N = 128 + 64, per-cloud tables (three different rows), slope 0, K2 = 0;
    kind 'ragged' (no reducing epilogue): M = BM + 37, N = 77;  kind 'meanshift' (STATS): per-column mean 100 x the spread.
    Tile 5 always has N = 192."""
    out = []
    for i, (pro, epi, tile) in enumerate(instantiated_combinations()):
        BM = tile_rows(tile)
        two_seg = pro == PRO_BNBWD and epi == (PW_STORE | PW_BIAS)
        base = dict(pro=pro, epi=epi, tile=tile, BM=BM)
        out.append(dict(base, kind="a", rpc=2 * BM, M=6 * BM, K1=32, K2=64 if two_seg else 0, N=192 if tile == 5 else 77,
                        per_cloud=False, slope=0.2, seed=1000 + i))
        out.append(dict(base, kind="b", rpc=BM, M=3 * BM, K1=96, K2=0, N=192, per_cloud=True, slope=0.0, seed=2000 + i))
        if not epi & (PW_STATS | PW_SEL | PW_BWDSTATS):
            out.append(dict(base, kind="ragged", rpc=0 if pro == PRO_NONE else BM, M=BM + 37, K1=32, K2=64 if two_seg else 0,
                            N=192 if tile == 5 else 77, per_cloud=False, slope=0.2, seed=3000 + i))
        if epi & PW_STATS:
            out.append(dict(base, kind="meanshift", rpc=2 * BM, M=6 * BM, K1=96, K2=0, N=77, per_cloud=False, slope=0.2, seed=4000 + i))
    return out


def case_id(c):
    return "pro%d-epi%d-tile%d-%s" % (c["pro"], c["epi"], c["tile"], c["kind"])


def rowgemm_inputs(c):
    """float32 numpy inputs of a rowgemm case (padded row strides: lda1 = K1 + 8, A2 a view at column 4 of a (M, K2 + 12) array)"""
    g = np.random.default_rng(c["seed"])
    M, K1, K2, N, rpc = c["M"], c["K1"], c["K2"], c["N"], c["rpc"]
    nb = max(1, (M + rpc - 1) // rpc) if (c["per_cloud"] and rpc) else 1
    pro, epi = c["pro"], c["epi"]
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    d = {}
    if c["kind"] == "meanshift":
        d["A1"] = (f(1, K1 + 8) + 0.01 * f(M, K1 + 8)).astype(np.float32)
        d["W"] = 0.3 * f(N, K1 + K2)
    elif pro == PRO_NONE:
        d["A1"] = wide_range((M, K1 + 8), 5, g)
        d["W"] = wide_range((N, K1 + K2), 4, g)
    else:
        d["A1"] = f(M, K1 + 8)
        d["W"] = wide_range((N, K1 + K2), 3, g, lo=-2.0)
    if K2:
        d["A2"] = f(M, K2 + 12)
    sign = lambda n: np.where(np.arange(n) % 3 == 0, -1.0, 1.0).astype(np.float32)
    if pro != PRO_NONE:
        d["alpha"] = (g.uniform(0.5, 1.5, K1) * sign(K1)).astype(np.float32)
        d["delta"] = 0.5 * f(nb, K1)
    if pro == PRO_BNBWD:
        d["P"], d["Q"] = 0.1 * f(nb, K1), 0.1 * f(K1)
        d["Y1"] = away_from_kink(f(M, K1 + 8), np.pad(d["alpha"], (0, 8), constant_values=1.0), np.pad(d["delta"], ((0, 0), (0, 8))),
                                 KINK_MARGIN, rpc if nb > 1 else 0)
    if epi & PW_BIAS:
        d["bias"] = f(N)
    if epi & PW_SEL:
        d["sgn"] = (g.uniform(0.5, 1.5, N) * sign(N)).astype(np.float32)
    if epi & PW_BWDSTATS:
        d["ealpha"] = (g.uniform(0.5, 1.5, N) * sign(N)).astype(np.float32)
        d["edelta"], d["emu"] = 0.5 * f(nb, N), 0.3 * f(nb, N)
        d["er"] = g.uniform(0.5, 2.0, N).astype(np.float32)
        d["Yp"] = away_from_kink(f(M, N), d["ealpha"], d["edelta"], KINK_MARGIN, rpc if nb > 1 else 0)
    return d


def rowgemm_oracle(c, d, store_n0=0, sel_n=None):
    """the fp64 oracle of a case on its inputs `d` (numpy float32) -> rowgemm()'s dict"""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(d[k])).double() if k in d else None
    K1, K2 = c["K1"], c["K2"]
    A2 = t("A2")[:, 4:4 + K2] if K2 else None
    Y1 = t("Y1")[:, :K1] if "Y1" in d else None
    ts = K1 if c["per_cloud"] else 0
    return rowgemm(c["pro"], c["epi"], c["tile"], t("A1")[:, :K1], t("W"), Y1=Y1, A2=A2, alpha=t("alpha"), delta=t("delta"), P=t("P"),
                   Q=t("Q"), tstride=ts, rows_per_cloud=c["rpc"], slope=c["slope"], store_n0=store_n0, bias=t("bias"), sgn=t("sgn"),
                   sel_n=(c["N"] if sel_n is None else sel_n), Yp=t("Yp"), ealpha=t("ealpha"), edelta=t("edelta"), emu=t("emu"),
                   er=t("er"), etstride=c["N"] if c["per_cloud"] else 0)


def tn_cases():
    """the row contractions of _SegHead.backward at reduced size and the row counts of the contract (name, tile, N1a, N1b, ones,
    lpro, rpro, N2, M, rows_per_slice, rows_per_cloud, per-cloud left / right tables, seed)"""
    k = ("name", "tile", "N1a", "N1b", "ones", "lpro", "rpro", "N2", "M", "rps", "rpc", "lpc", "rpc_tab", "seed")
    rows = [("logits", 3, 4, 0, 0, 0, 1, 32, 3 * 128, 128, 128, False, False, 1),
            ("qw", 3, 65, 0, 0, 0, 0, 64, 128, 64, 0, False, False, 2),
            ("gram", 5, 64, 64, 1, 2, 0, 64, 2 * 64 + 32, 64, 128, True, False, 3),
            ("layer2", 2, 32, 0, 0, 2, 1, 64, 3 * 32, 32, 96, False, False, 4),
            ("layer1", 1, 64, 0, 0, 2, 1, 64, 3 * 128, 64, 128, False, True, 5),
            ("one-slice", 3, 64, 0, 0, 2, 1, 64, 128, 128, 128, False, False, 6),
            ("short-slice", 1, 64, 0, 0, 2, 1, 128, 2 * 128 + 32, 128, 256, True, True, 7),
            ("odd-rows", 2, 77, 0, 0, 0, 0, 130, 2 * 32 + 13, 32, 0, False, False, 8)]
    return [dict(zip(k, r)) for r in rows]


def tn_inputs(c):
    g = np.random.default_rng(100 + c["seed"])
    M, N1a, N1b, N2 = c["M"], c["N1a"], c["N1b"], c["N2"]
    nb = (M + c["rpc"] - 1) // c["rpc"] if c["rpc"] else 1
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    sign = lambda n: np.where(np.arange(n) % 3 == 0, -1.0, 1.0).astype(np.float32)
    d = {"R": f(M, N2 + 4)}
    d["L1"] = f(M, N1a + 3 + (-(N1a + 3)) % 4) if c["lpro"] else wide_range((M, N1a + 3 + (-(N1a + 3)) % 4), 4, g)
    if N1b:
        d["L2"] = f(M, N1b)
    if c["lpro"]:
        ln = nb if c["lpc"] else 1
        d["lalpha"] = (g.uniform(0.5, 1.5, N1a) * sign(N1a)).astype(np.float32)
        d["ldelta"], d["lP"], d["lQ"] = 0.5 * f(ln, N1a), 0.1 * f(ln, N1a), 0.1 * f(N1a)
        pad = d["L1"].shape[1] - N1a
        d["LY1"] = away_from_kink(f(*d["L1"].shape), np.pad(d["lalpha"], (0, pad), constant_values=1.0),
                                  np.pad(d["ldelta"], ((0, 0), (0, pad))), KINK_MARGIN, c["rpc"] if ln > 1 else 0)
    if c["rpro"]:
        d["ralpha"] = (g.uniform(0.5, 1.5, N2) * sign(N2)).astype(np.float32)
        d["rdelta"] = 0.5 * f(nb if c["rpc_tab"] else 1, N2)
    return d


def tn_oracle(c, d):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(d[k])).double() if k in d else None
    N1a, N2 = c["N1a"], c["N2"]
    return tn(t("L1")[:, :N1a], t("R")[:, :N2], LY1=t("LY1")[:, :N1a] if "LY1" in d else None, L2=t("L2"), lpro=c["lpro"],
              lalpha=t("lalpha"), ldelta=t("ldelta"), lP=t("lP"), lQ=t("lQ"), lts=N1a if c["lpc"] else 0, rpro=c["rpro"], ralpha=t("ralpha"),
              rdelta=t("rdelta"), rts=N2 if c["rpc_tab"] else 0, slope=0.2, rows_per_cloud=c["rpc"], rows_per_slice=c["rps"], ones=c["ones"],
              with_mag=True)
