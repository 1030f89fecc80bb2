"""GPU tests of the folded tail of the head's backward (csrc/pointwise.hip, include/fsg_hip.h: fsg_pw_rowgemm_scatter_f32,
fsg_pw_gf_prep_sort_f32, fsg_pw_tn_reduce_image_f32, fsg_pw_logits_bwd_bias_f32, and the deeper load pipeline of
fsg_pw_tn_reduce_f32).  The folded entries promise the BITS of the launch sequences they replace -- same operations in the same
order -- so every comparison is torch.equal and the oracle is the existing entry sequence on the same inputs (for the slice fold:
a numpy float32 emulation of its stated association, exact because it is adds only).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRO_BNBWD, PW_STORE, PW_BIAS = 2, 1, 16


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def G(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _call(fsg, name, *a):
    fsg._lib.call(name, *[x.data_ptr() if torch.is_tensor(x) else x for x in a], torch.cuda.current_stream().cuda_stream)


def _eq(a, b):
    """bitwise equality (torch.equal on the raw words: a NaN or a -0.0 would count too)"""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ row-GEMM + scatter
def _make_arg(kind, g, B, C, Npts):
    if kind == "random" or kind == "zero_coef":
        arg = g.integers(0, Npts, (B, C))
    elif kind == "same_row":            # all channels of a cloud on one row (a different one per cloud)
        arg = np.repeat(np.array([[70], [5], [127]])[:B], C, 1)
    elif kind == "one_tile":            # the rows of one tile, each many times
        arg = np.stack([64 * (b % 2) + g.permutation(C) % 64 for b in range(B)])
    elif kind == "edges":               # rows 0, 63, 64, 127; cloud 1 has an empty first tile, cloud 2 an empty second one
        arg = g.choice(np.array([0, 63, 64, 127]), (B, C))
        arg[1] = g.choice(np.array([64, 127]), C)
        arg[2] = g.choice(np.array([0, 63]), C)
    return arg.astype(np.int32)


@pytest.mark.parametrize("kind", ["random", "same_row", "one_tile", "edges", "zero_coef"])
@pytest.mark.parametrize("C", [640, 1000, 1024])
def test_rowgemm_scatter_is_rowgemm_then_scatter(fsg, device, C, kind):
    F = fsg.functional
    B, Npts, K1, K2, N = 3, 128, 32, 64, 192
    M = B * Npts
    g = np.random.default_rng(C + len(kind))
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    da, y, lv = G(f(M, K1), device), G(f(M, K1), device), G(f(M, K2 + 4), device)
    W = G(f(N, K1 + K2) / 8, device)
    alpha, delta, P, Q = G(0.5 + np.abs(f(K1)), device), G(f(B, K1), device), G(0.1 * f(B, K1), device), G(0.1 * f(K1), device)
    bias = G(f(N), device)
    Wg = G(f(C, N + 8), device)
    coef = f(B, C)
    if kind == "zero_coef":
        coef[1] = 0.0
    coef = G(coef, device)
    arg_np = _make_arg(kind, g, B, C, Npts)
    arg = G(arg_np, device)
    img = F.pw_weight_image(W)

    def product(out):
        return dict(A1=da, Y1=y, A2=lv, lda1=K1, lda2=lv.stride(0), K1=K1, K2=K2, Bimg=img, M=M, N=N, rows_per_cloud=Npts,
                    alpha=alpha, delta=delta, P=P, Q=Q, tstride=K1, slope=0.2, C=out, ldc=N, store_n0=0, bias=bias)
    plain = torch.full((M, N), -7.0, dtype=torch.float32, device=device)
    F.pw_rowgemm(PRO_BNBWD, PW_STORE | PW_BIAS, 5, **product(plain))
    want = plain.clone()
    ws = fsg._lib.workspace("fsg_pw_scatter_rows", B, C, device=device)
    _call(fsg, "fsg_pw_scatter_rows_f32", coef, arg, Wg, Wg.stride(0), B, C, N, Npts, want, N, ws)
    torch.cuda.synchronize()
    keys = ws.view(torch.int32).view(B, 1024)                    # the existing sort's keys
    rows = np.sort(arg_np, 1)
    first = np.stack([np.searchsorted(rows[b], 64 * np.arange(Npts // 64 + 1), "left") for b in range(B)]).astype(np.int32)
    got = torch.full((M, N), -7.0, dtype=torch.float32, device=device)
    F.pw_rowgemm_scatter(keys, G(first, device), coef, Wg, **product(got))
    torch.cuda.synchronize()
    sel = np.zeros(M, bool)
    sel[(np.arange(B)[:, None] * Npts + arg_np).ravel()] = True
    sel = torch.from_numpy(sel).to(device)
    assert _eq(got[~sel], plain[~sel]), "rows that no channel selected differ from the plain product"
    assert bool((want[sel] != plain[sel]).any()) or kind == "zero_coef"
    assert _eq(got, want)


# ------------------------------------------------------------------------------------------------ sort + tile table
@pytest.mark.parametrize("B,Npts,C", [(3, 128, 640), (9, 128, 1024), (3, 64 * 300, 1024), (9, 64 * 300, 1000)])
def test_gf_prep_sort_is_gf_prep_then_sort(fsg, device, B, Npts, C):
    g = np.random.default_rng(B + Npts + C)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    C0, K, M = 64, 64, B * Npts
    ldq = (K + 4) & ~3
    t = {k: G(v, device) for k, v in dict(dc=f(B, C0), W0=f(C0, K + C), gfeat=f(B, C), ysel=f(B, C), alpha=0.5 + np.abs(f(C)),
                                          delta=f(1, C), mean=f(C), inv=0.5 + np.abs(f(C)), W=f(C, K + 8)).items()}
    arg_np = g.integers(0, Npts, (B, C)).astype(np.int32)
    arg_np[0, : C // 2] = Npts - 1                    # a long run on the last row; the other tiles of cloud 0 are thin
    arg = G(arg_np, device)
    W0g = t["W0"][:, K:]
    outs = []
    for fused in (False, True):
        f32 = dict(dtype=torch.float32, device=device)
        dW0 = torch.full((C0, K + C), -7.0, **f32)
        Wq = torch.full((C, ldq), -7.0, **f32)
        dbeta, dgamma, P, Q, coef = (torch.full(s, -7.0, **f32) for s in ((C,), (C,), (C,), (C,), (B, C)))
        head = (t["dc"], W0g, K + C, C0, t["gfeat"], dW0[:, K:], K + C)
        tail = (t["ysel"], t["alpha"], t["delta"], t["mean"], t["inv"], B, C, M, 1, 0.2, dbeta, dgamma, P, Q, coef, t["W"], K + 8, K, Wq, ldq)
        if fused:
            keys = torch.full((B, 1024), -7, dtype=torch.int32, device=device)
            first = torch.full((B, Npts // 64 + 1), -7, dtype=torch.int32, device=device)
            _call(fsg, "fsg_pw_gf_prep_sort_f32", *head, *tail, arg, Npts, keys, first)
        else:
            _call(fsg, "fsg_pw_gf_prep_f32", *head, None, *tail)
            ws = fsg._lib.workspace("fsg_pw_scatter_rows", B, C, device=device)
            dX = torch.zeros(M, 4, **f32)
            _call(fsg, "fsg_pw_scatter_rows_f32", coef, arg, t["W"], K + 8, B, C, 4, Npts, dX, 4, ws)
            keys, first = ws.view(torch.int32).view(B, 1024), None
        torch.cuda.synchronize()
        outs.append((dW0, Wq, dbeta, dgamma, P, Q, coef, keys, first))
    for a, b in zip(outs[0][:8], outs[1][:8]):
        assert _eq(a, b)
    rows = np.sort(arg_np, 1)
    want = np.stack([np.searchsorted(rows[b], 64 * np.arange(Npts // 64 + 1), "left") for b in range(B)]).astype(np.int32)
    assert np.array_equal(outs[1][8].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ reduce + image
@pytest.mark.parametrize("S", [1, 5, 13, 16])       # (13: three rounds of four slices and the remainder)
@pytest.mark.parametrize("KL", [64, 192])
def test_tn_reduce_image_is_reduce_then_image(fsg, device, KL, S):
    F = fsg.functional
    g = np.random.default_rng(KL + S)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    Mr, ldq = 64 * S, (KL + 4) & ~3
    Wq, Wg = G(f(Mr, ldq), device), G(f(Mr, KL + 8), device)
    kw = dict(L1=Wq, ldl1=ldq, N1a=KL + 1, N1b=0, lpro=0, R=Wg, ldr=Wg.stride(0), N2=KL, rpro=0, slope=0.2, M=Mr, rows_per_cloud=0,
              rows_per_slice=64)
    ks0, KS = 3, 3 + KL // 16 + 2
    nbytes = (KL // 32) * KS * 3 * 1024
    img_a = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=device)
    img_b = img_a.clone()
    m1n = torch.empty(KL + 1, KL, dtype=torch.float32, device=device)
    F.pw_tn(3, m1n, KL, **kw)
    F.pw_weight_image(m1n[:KL], scale=-1.0, out=img_a, ks0=ks0, KS=KS)
    npvec = torch.full((KL,), -7.0, dtype=torch.float32, device=device)
    part = []
    F.pw_tn(3, npvec, KL, defer=part, **kw)
    assert part[0][5] == S
    _call(fsg, "fsg_pw_tn_reduce_image_f32", part[0][0], S, KL + 1, KL, KL, -1.0, ks0, KS, img_b, npvec, KL)
    torch.cuda.synchronize()
    assert _eq(npvec, m1n[KL])
    assert torch.equal(img_a, img_b)
    assert bool((img_a != 0x5A).any())


@pytest.mark.parametrize("S", [6, 21])               # (21: a round of sixteen slices, one of four and the remainder)
@pytest.mark.parametrize("N1,N2,NI", [(53, 50, 45), (49, 48, 48), (70, 128, 40)])
def test_tn_reduce_image_other_shapes(fsg, device, N1, N2, NI, S):
    """the kernel's other paths (N2 not a multiple of 64 / of 4, a ragged last row block, several fp32 rows) on given slices,
    against fsg_pw_tn_reduce_f32 + fsg_pw_weight_image_f32"""
    F = fsg.functional
    g = np.random.default_rng(N1 + N2 + NI + S)
    part = (g.standard_normal((S, N1, N2)) * 10.0 ** g.integers(-3, 4, (S, 1, 1))).astype(np.float32)
    ws = G(part, device).view(-1).view(torch.uint8)
    f32 = dict(dtype=torch.float32, device=device)
    C1, C2 = torch.empty(NI, N2, **f32), torch.full((max(N1 - NI, 1), N2 + 1), -7.0, **f32)
    F.pw_tn_reduce([(ws, C1, N2, C2, N2 + 1, S, N1, N2, NI)])
    ks0, KS = 2, 2 + (N2 + 15) // 16 + 1
    img_a = torch.full((((NI + 31) // 32) * KS * 3 * 1024,), 0x5A, dtype=torch.uint8, device=device)
    img_b = img_a.clone()
    F.pw_weight_image(C1, scale=-1.0, out=img_a, ks0=ks0, KS=KS)
    D2 = torch.full_like(C2, -7.0)
    _call(fsg, "fsg_pw_tn_reduce_image_f32", ws, S, N1, N2, NI, -1.0, ks0, KS, img_b, D2, N2 + 1)
    torch.cuda.synchronize()
    assert torch.equal(img_a, img_b) and bool((img_a != 0x5A).any())
    assert _eq(C2, D2)


# ------------------------------------------------------------------------------------------------ logits + bias
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", [33, 1027, 4100])
@pytest.mark.parametrize("classes", [1, 2, 4, 8])
def test_logits_bwd_bias_is_logits_bwd_then_colsum(fsg, device, classes, M, C):
    g = np.random.default_rng(classes + M + C)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    t = [G(a, device) for a in (f(M, classes), f(classes, C), f(M, C), 0.5 + np.abs(f(C)), f(C), f(C), 0.5 + np.abs(f(C)))]
    Rb = (M + 31) // 32
    outs = []
    for fused in (False, True):
        f32 = dict(dtype=torch.float32, device=device)
        da, rec2, db = torch.full((M, C), -7.0, **f32), torch.full((Rb, 2, C), -7.0, **f32), torch.full((classes + 3,), -7.0, **f32)
        if fused:
            _call(fsg, "fsg_pw_logits_bwd_bias_f32", t[0], classes, *t[1:], M, C, 0.2, da, rec2, db)
        else:
            _call(fsg, "fsg_pw_logits_bwd_f32", t[0], classes, *t[1:], M, C, 0.2, da, rec2)
            _call(fsg, "fsg_colsum_narrow_f32", t[0], M, classes, db)
        torch.cuda.synchronize()
        outs.append((da, rec2, db))
    for a, b in zip(*outs):
        assert _eq(a, b)
    assert bool((outs[1][2][classes:] == -7.0).all()) and bool((outs[1][2][:classes] != -7.0).all())


# ------------------------------------------------------------------------------------------------ the slice fold
def _fold_np(part):
    """pw_tn_reduce's association: four interleaved accumulators over the slices, the remainder into the first, (a0+a1)+(a2+a3)"""
    S = part.shape[0]
    a = [np.zeros(part.shape[1:], np.float32) for _ in range(4)]
    q = 0
    while q + 4 <= S:
        for u in range(4):
            a[u] = a[u] + part[q + u]
        q += 4
    while q < S:
        a[0] = a[0] + part[q]
        q += 1
    return (a[0] + a[1]) + (a[2] + a[3])


@pytest.mark.parametrize("S", [1, 3, 4, 17, 33])
def test_tn_reduce_many_keeps_the_association(fsg, device, S):
    F = fsg.functional
    g = np.random.default_rng(S)
    shapes = [(70, 33, 70), (65, 48, 64)]           # (N1, N2, N1a): one matrix; rows behind N1a to a second matrix
    jobs, wants, outs = [], [], []
    for N1, N2, N1a in shapes:
        part = (g.standard_normal((S, N1, N2)) * 10.0 ** g.integers(-3, 4, (S, 1, 1))).astype(np.float32)
        ws = G(part, device).view(-1).view(torch.uint8)
        C1 = torch.full((N1a, N2 + 2), -7.0, dtype=torch.float32, device=device)
        C2 = torch.full((max(N1 - N1a, 1), N2 + 1), -7.0, dtype=torch.float32, device=device)
        jobs.append((ws, C1, N2 + 2, C2, N2 + 1, S, N1, N2, N1a))
        wants.append(_fold_np(part))
        outs.append((C1, C2))
    F.pw_tn_reduce(jobs)
    torch.cuda.synchronize()
    for (N1, N2, N1a), want, (C1, C2) in zip(shapes, wants, outs):
        assert _eq(C1[:, :N2], G(want[:N1a], device))
        assert bool((C1[:, N2:] == -7.0).all())
        if N1 > N1a:
            assert _eq(C2[:, :N2], G(want[N1a:], device))
            assert bool((C2[:, N2:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ the whole head
def _run_head(fsg, device, dims, B, Npts, fused_tail, names):
    F = fsg.functional
    KL, CG, C0, C1, C2, CLS = dims
    gen = torch.Generator().manual_seed(sum(dims) + B)
    r = lambda *s: torch.randn(*s, generator=gen)
    P = {"Wg": r(CG, KL) / KL ** 0.5, "W0": r(C0, KL + CG) / (KL + CG) ** 0.5, "W1": r(C1, C0) / C0 ** 0.5, "W2": r(C2, C1) / C1 ** 0.5,
         "W3": r(CLS, C2) / C2 ** 0.5, "b3": r(CLS)}
    bns = []
    for C in (CG, C0, C1, C2):
        bn = torch.nn.BatchNorm1d(C).to(device).train()
        with torch.no_grad():
            bn.weight.copy_((0.5 + torch.rand(C, generator=gen)) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0))
            bn.bias.copy_(0.2 * r(C))
        bns.append(bn)
    M = B * Npts
    lv = 0.4 + 0.6 * r(M, KL)
    lv = torch.where(lv < 0, 0.2 * lv, lv)
    gout = r(M, CLS)
    W = {k: v.to(device).requires_grad_(True) for k, v in P.items()}
    xt = lv.to(device).requires_grad_(True)
    assert F.seg_head_supported(xt, B, Npts, W["Wg"], W["W0"], W["W1"], W["W2"], W["W3"])
    steps = tuple((True, 0.1) for _ in bns)
    old = F.set_fused_head_tail(fused_tail)
    real = fsg._lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    fsg._lib.call = spy
    try:
        y = F._SegHead.apply(xt, B, Npts, 0.2, tuple(bns), steps, W["Wg"], bns[0].weight, bns[0].bias, W["W0"], bns[1].weight,
                             bns[1].bias, W["W1"], bns[2].weight, bns[2].bias, W["W2"], bns[3].weight, bns[3].bias, W["W3"], W["b3"])
        y.backward(gout.to(device))
        torch.cuda.synchronize()
    finally:
        fsg._lib.call = real
        F.set_fused_head_tail(old)
    grads = [xt.grad] + [W[k].grad for k in ("Wg", "W0", "W1", "W2", "W3", "b3")]
    for bn in bns:
        grads += [bn.weight.grad, bn.bias.grad]
    return [y.detach()] + grads


@pytest.mark.parametrize("dims,B,Npts,inside", [((192, 1024, 64, 64, 64, 4), 2, 256, True), ((64, 128, 64, 64, 64, 4), 2, 256, False)])
def test_seg_head_tail_fused_equals_unfused(fsg, device, dims, B, Npts, inside):
    """_SegHead forward + backward, every returned gradient, with the tail folded and not; outside the envelope of the scatter
    epilogue (levels narrower than 192, fewer than 513 global channels) the folded setting keeps the separate sort + scatter"""
    n_on, n_off = [], []
    on = _run_head(fsg, device, dims, B, Npts, True, n_on)
    off = _run_head(fsg, device, dims, B, Npts, False, n_off)
    assert len(on) == len(off) == 16 and all(t is not None for t in on)
    for a, b in zip(on, off):
        assert _eq(a, b)
    assert "fsg_pw_scatter_rows_f32" in n_off and "fsg_pw_rowgemm_scatter_f32" not in n_off and "fsg_pw_weight_image_f32" in n_off
    assert ("fsg_pw_rowgemm_scatter_f32" in n_on) == inside and ("fsg_pw_gf_prep_sort_f32" in n_on) == inside
    assert ("fsg_pw_scatter_rows_f32" in n_on) == (not inside)
    assert "fsg_pw_tn_reduce_image_f32" in n_on and "fsg_pw_weight_image_f32" not in n_on
