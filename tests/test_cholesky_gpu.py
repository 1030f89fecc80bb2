"""GPU tests of fsg_cholesky_f64, fsg_cholesky_solve_f64 and fsg_cpd_spd_system_f64 (csrc/cholesky.hip).

The yardstick is LAPACK's own residual on the same matrix (torch on the CPU, fp64): the kernel may have at most 4 x that, with a
floor of 4 fp64 ulps (8.9e-16) -- another blocking changes the summation order and nothing else.  Residuals are evaluated in
np.longdouble up to n = 257 and in fp64 above (tests/chol_oracle.py).  Every measured pair is printed and, when
FSG_CHOL_PARITY names a file, appended to it (profiles/cholesky_parity.txt is such a record)."""
import os

import pytest
import torch

import chol_oracle as co
import cpd_oracle

pytestmark = pytest.mark.gpu
NB = 64                       # FSG_CHOL_BLOCK (asserted below)
FLOOR = 4 * 2.0 ** -52        # 8.9e-16
SIZES = [1, 2, 15, 16, 17, NB - 1, NB, NB + 1, 2 * NB + 3, 257]
KINDS = ["cond1e2", "cond1e6", "cond1e10", "diagonal"]


def record(line):
    print(line)
    path = os.environ.get("FSG_CHOL_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def F():
    from fissure_segmentation_amd import functional
    assert functional.CHOL_BLOCK == NB
    return functional


def matrices(kind, n, B, seed):
    if kind == "diagonal":
        g = torch.Generator().manual_seed(seed)
        return torch.diag_embed(torch.rand(B, n, generator=g, dtype=torch.float64) * 9 + 0.5)
    return co.random_spd(n, float(kind[4:]), seed, B)


def rhs_of(B, n, r, seed):
    return torch.randn(B, n, r, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def check_against_lapack(what, A, b, L, X, info):
    """A (B,n,n), b (B,n,r) on the CPU; L, X, info from the kernels"""
    assert info.dtype == torch.int32 and info.is_cuda and not info.any(), info
    L, X = L.cpu(), X.cpu()
    Lr = torch.linalg.cholesky(co.lower_symmetric(A))
    Xr = torch.cholesky_solve(b, Lr)
    for i in range(A.shape[0]):
        f_got, f_yard = co.factor_residual(A[i], L[i]), co.factor_residual(A[i], Lr[i])
        s_got, s_yard = co.solve_residual(A[i], X[i], b[i]), co.solve_residual(A[i], Xr[i], b[i])
        record(f"{what} item {i}: factor kernel {f_got:.3e} lapack {f_yard:.3e} | solve kernel {s_got:.3e} lapack {s_yard:.3e}")
        assert f_got <= max(4 * f_yard, FLOOR), (what, i, f_got, f_yard)
        assert s_got <= max(4 * s_yard, FLOOR), (what, i, s_got, s_yard)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_factor_and_solve_against_lapack(device, n, B):
    f = F()
    for k, kind in enumerate(KINDS):
        r = (1, 3, 8)[(k + n + B) % 3]
        A, b = matrices(kind, n, B, 100 * n + k), rhs_of(B, n, r, 7 * n + k)
        Ad, bd = A.to(device), b.to(device)
        keep_a, keep_b = Ad.clone(), bd.clone()
        L, info = f.cholesky_factor(Ad)
        X = f.cholesky_solve(L, bd)
        assert torch.equal(Ad, keep_a) and torch.equal(bd, keep_b), "the inputs were modified"
        assert torch.equal(torch.triu(L, 1), torch.triu(keep_a, 1)), "the strict upper triangle was written"
        check_against_lapack(f"{kind} n={n} B={B} r={r}", A, b, L, X, info)
        X2, info2 = f.spd_solve(Ad, bd)
        assert torch.equal(X2, X) and torch.equal(info2, info) and torch.equal(Ad, keep_a)


@pytest.mark.parametrize("r", [1, 3, 8])
def test_every_rhs_count_and_the_in_place_forms(device, r):
    f = F()
    n, B = 2 * NB + 3, 3
    A, b = matrices("cond1e6", n, B, 5), rhs_of(B, n, r, 6)
    Ad, bd = A.to(device), b.to(device)
    L, info = f.cholesky_factor(Ad)
    X = f.cholesky_solve(L, bd)
    check_against_lapack(f"cond1e6 n={n} B={B} r={r}", A, b, L, X, info)
    for c in range(r):     # a column does not depend on its neighbours; a vector is a single column
        assert torch.equal(f.cholesky_solve(L, bd[:, :, c]), X[:, :, c])
    A2, b2 = Ad.clone(), bd.clone()
    L2, _ = f.cholesky_factor(A2, overwrite=True)
    assert L2.data_ptr() == A2.data_ptr() and torch.equal(L2, L)
    X2 = f.cholesky_solve(L2, b2, overwrite=True)
    assert X2.data_ptr() == b2.data_ptr() and torch.equal(X2, X)
    out = torch.empty_like(Ad)
    L3, _ = f.cholesky_factor(Ad, out=out)
    assert L3.data_ptr() == out.data_ptr() and torch.equal(torch.tril(L3), torch.tril(L))
    L1, info1 = f.cholesky_factor(Ad[1])                       # without the batch axis
    assert L1.shape == (n, n) and info1.shape == (1,) and torch.equal(L1, L[1])
    assert torch.equal(f.cholesky_solve(L1, bd[1]), X[1])
    with pytest.raises(ValueError):
        f.cholesky_solve(L, torch.zeros(B, n, 9, dtype=torch.float64, device=device))


def test_n_1023(device):
    f = F()
    n, B, r = 1023, 2, 3
    A, b = matrices("cond1e6", n, B, 11), rhs_of(B, n, r, 12)
    L, info = f.cholesky_factor(A.to(device))
    X = f.cholesky_solve(L, b.to(device))
    check_against_lapack(f"cond1e6 n={n} B={B} r={r}", A, b, L, X, info)


@pytest.fixture(scope="module")
def cpd_systems():
    """(G, P1, PX, Y, sigma2) of the first and the last iteration of the 193 x 161 run with two far-away moving points"""
    X, Y = co.case_pair(193, 161, True)
    run = co.deformable_spd(X, Y, keep_systems=True)
    assert int((run["systems"][-1][1] == 0).sum()) > 0
    return run["systems"]


def test_cpd_systems_first_and_last_iteration(device, cpd_systems):
    f = F()
    for which, (G, P1, PX, Y, sigma2) in zip(("first", "last"), cpd_systems):
        S, rhs, d = f.cpd_spd_system(*(t[None].to(device) for t in (G, P1, PX, Y)), sigma2.reshape(1).to(device), co.ALPHA)
        L, info = f.cholesky_factor(S)
        V = f.cholesky_solve(L, rhs)
        check_against_lapack(f"cpd system {which} iteration n={G.shape[0]} zero rows={int((P1 == 0).sum())}", S.cpu(), rhs.cpu(), L, V,
                             info)
        W = (d[:, :, None] * V)[0].cpu()
        A, b = co.lu_system(G, P1, PX, Y, sigma2, co.ALPHA)
        Wr = torch.linalg.solve(A, b)
        err, cond = float((W - Wr).abs().max() / Wr.abs().max()), float(torch.linalg.cond(A))
        record(f"cpd system {which} iteration: |W_chol - W_lu| / |W| = {err:.3e}, cond(A) = {cond:.3e}")
        # two backward-stable solves of one system: each within about n eps cond of the solution (n = 161: 100 to be generous)
        assert err <= 100 * cond * 2.0 ** -53 and not W[P1 == 0].any()


def test_assembly_kernel(device, cpd_systems):
    f = F()
    ts = [torch.stack([s[i] for s in cpd_systems]) for i in range(4)]
    sigma2 = torch.stack([s[4].reshape(()) for s in cpd_systems])
    S, rhs, d = f.cpd_spd_system(*(t.to(device) for t in ts), sigma2.to(device), co.ALPHA)
    assert S.shape == ts[0].shape and rhs.shape == ts[2].shape and d.shape == ts[1].shape
    for i, (G, P1, PX, Y, s2) in enumerate(cpd_systems):
        Sr, rr, dr = co.spd_system(G, P1, PX, Y, s2, co.ALPHA)
        for name, got, ref in (("S", torch.tril(S[i].cpu()), torch.tril(Sr)), ("rhs", rhs[i].cpu(), rr), ("d", d[i].cpu(), dr)):
            ulps = float(((got - ref).abs() / (ref.abs() * 2.0 ** -52).clamp(min=1e-300)).max())
            record(f"assembly item {i} {name}: {ulps:.2f} ulps at most")
            assert ulps <= 4, (name, ulps)
        zero = P1 == 0
        if zero.any():
            assert torch.equal(S[i].cpu().diagonal()[zero], (co.ALPHA * s2).expand(int(zero.sum())))
            assert not rhs[i].cpu()[zero].any() and not d[i].cpu()[zero].any()
            assert not torch.tril(S[i].cpu(), -1)[zero].any() and not torch.tril(S[i].cpu(), -1)[:, zero].any()


def test_only_the_lower_triangle_is_read(device):
    f = F()
    n, B = 2 * NB + 3, 2
    A, b = matrices("cond1e6", n, B, 21).to(device), rhs_of(B, n, 3, 22).to(device)
    L, info = f.cholesky_factor(A)
    X = f.cholesky_solve(L, b)
    nan = torch.triu(torch.full_like(A, float("nan")), 1)
    Ln, infon = f.cholesky_factor(torch.tril(A) + nan)
    Xn = f.cholesky_solve(Ln, b)
    assert torch.equal(torch.tril(Ln), torch.tril(L)) and torch.equal(infon, info) and torch.equal(Xn, X)
    assert torch.isnan(torch.triu(Ln, 1)[torch.triu(torch.ones(n, n, dtype=torch.bool, device=device), 1).expand(B, n, n)]).all()
    assert torch.isfinite(X).all()


@pytest.mark.parametrize("bad", [-1.0, float("nan")], ids=["negative", "nan"])
@pytest.mark.parametrize("index", [0, 5, NB, 2 * NB + 2], ids=["first", "in_block_0", "block_1", "tail"])
def test_not_positive_definite_is_a_status(device, index, bad):
    """a status path: the call returns, the item reports its column, the other items do not notice"""
    f = F()
    n = 2 * NB + 3
    good = matrices("cond1e2", n, 2, 31).to(device)
    A = torch.stack([good[0], torch.eye(n, dtype=torch.float64, device=device), good[1]])
    A[1, index, index] = bad
    L, info = f.cholesky_factor(A)
    b = rhs_of(3, n, 3, 32).to(device)
    X = f.cholesky_solve(L, b)
    torch.cuda.synchronize()
    assert info.tolist() == [0, index + 1, 0]
    for i, g in ((0, 0), (2, 1)):
        La, ia = f.cholesky_factor(good[g])
        assert torch.equal(L[i], La) and int(ia) == 0 and torch.equal(X[i], f.cholesky_solve(La, b[i]))
    assert torch.equal(L[1, :index, :index], torch.eye(n, dtype=torch.float64, device=device)[:index, :index])


def test_same_bits_twice_alone_in_a_batch_and_from_a_graph(device):
    f = F()
    n, B, r = 2 * NB + 3, 3, 3
    A, b = matrices("cond1e6", n, B, 41).to(device), rhs_of(B, n, r, 42).to(device)
    L, info = f.cholesky_factor(A)
    X = f.cholesky_solve(L, b)
    L2, _ = f.cholesky_factor(A)
    assert torch.equal(L2, L) and torch.equal(f.cholesky_solve(L2, b), X)
    for i in range(B):
        Li, _ = f.cholesky_factor(A[i:i + 1])
        assert torch.equal(Li[0], L[i]) and torch.equal(f.cholesky_solve(Li, b[i:i + 1])[0], X[i])
    # captured: the static inputs are refilled between the replays
    As, bs = torch.zeros_like(A), torch.zeros_like(b)
    As.copy_(torch.eye(n, dtype=torch.float64, device=device))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        f.spd_solve(As, bs)                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Lg, ig = f.cholesky_factor(As)
        Xg = f.cholesky_solve(Lg, bs)
    for _ in range(2):
        As.copy_(A)
        bs.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Lg, L) and torch.equal(Xg, X) and torch.equal(ig, info)
        As.zero_()
        Lg.zero_()
        Xg.zero_()
