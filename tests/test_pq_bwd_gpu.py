"""GPU tests of the tail of the EdgeConv [P | Q] Linears' backward and of the optimizer behind it (include/fsg_hip.h:
fsg_gemm_small_many_deferred_f32 -- the weight-gradient products of all blocks in one launch --,
fsg_edge_weights_bwd_folded_f32 -- their split sums inside the edge-weights backward -- and
fsg_adam_flat_segments_f32 -- Adam reading the gradients where autograd left them).  All promise the BITS of the launch sequences
they replace (the same adds in the same order, the same per-element update), so every comparison is torch.equal on the raw words
and the oracle is the earlier entry sequence on the same inputs.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def _eq(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Spy:
    """records the names of the C-ABI entries called inside the `with` block"""

    def __init__(self, fsg):
        self.lib, self.names = fsg._lib, []

    def __enter__(self):
        self.real = self.lib.call

        def call(name, *a):
            self.names.append(name)
            return self.real(name, *a)
        self.lib.call = call
        return self.names

    def __exit__(self, *exc):
        self.lib.call = self.real


# ------------------------------------------------------------------------------------------------ A: folded split sums
def _expected_splits(M):
    """what fsg_gemm_small_deferred_f32 reports for a (128, C <= 64) product behind M rows (csrc/small_gemm.hip: splits_for, two
    output tiles): no split below 128 rows, else M / 64 splits up to 128"""
    return 0 if M < 128 else min(M // 64, 128)


def _fold_jobs(fsg, device, shapes, seed):
    """shapes: [(Co, C, M)] -> (folded outputs, reference outputs): dW = g^T x (2Co, C) behind M rows per job; reference = the
    product reduced at once (fsg_gemm_small_f32: the same product kernel, then its own split sum) + fsg_edge_weights_many_f32"""
    F, lib = fsg.functional, fsg._lib
    gen = torch.Generator().manual_seed(seed)
    fold, ref = lib.EdgeWeightFoldJobs(), lib.EdgeWeightJobs()
    fold.n = ref.n = len(shapes)
    keep, outs, refs = [], [], []
    for j, (Co, C, M) in enumerate(shapes):
        g = (torch.randn(M, 2 * Co, generator=gen) * torch.logspace(-2, 2, M).unsqueeze(1)).to(device)
        x = torch.randn(M, C, generator=gen).to(device)
        N = 2 * Co
        dw_ref = F.gemm_small(g, 1, N, x, C, 1, None, N, C, M)
        dw = torch.full((N, C), float("nan"), device=device)
        ws = lib.workspace("fsg_gemm_small", N, C, M, device=device)
        S = ctypes.c_int(-1)
        lib.call("fsg_gemm_small_deferred_f32", g.data_ptr(), 1, N, x.data_ptr(), C, 1, dw.data_ptr(), C, N, C, M, None,
                 ws.data_ptr() if ws is not None else None, ctypes.byref(S), _stream())
        assert S.value == _expected_splits(M), (M, S.value)
        if S.value > 1:     # the partials the folded entry gets are what the reduce-at-once path sums: check one split sum here
            part = ws.view(torch.float32)[:S.value * N * C].view(S.value, N * C)
            assert torch.allclose(part.double().sum(0).float().view(N, C), dw_ref, rtol=1e-4, atol=1e-3 * float(dw_ref.abs().max()))
        else:
            assert _eq(dw, dw_ref)
        out = torch.full((Co, 2 * C), float("nan"), device=device)
        out_ref = torch.full((Co, 2 * C), float("nan"), device=device)
        src = ws if S.value > 1 else dw
        fold.src[j], fold.dst[j], fold.Co[j], fold.C[j], fold.S[j] = src.data_ptr(), out.data_ptr(), Co, C, S.value
        ref.src[j], ref.dst[j], ref.Co[j], ref.C[j] = dw_ref.data_ptr(), out_ref.data_ptr(), Co, C
        keep += [g, x, dw, dw_ref, ws]
        outs.append(out), refs.append(out_ref)
    lib.call("fsg_edge_weights_bwd_folded_f32", ctypes.byref(fold), _stream())
    lib.call("fsg_edge_weights_many_f32", ctypes.byref(ref), 1, _stream())
    torch.cuda.synchronize()
    return outs, refs


@pytest.mark.parametrize("shapes", [
    [(64, 3, 64)], [(64, 64, 64)],                  # S = 1: the job reads a finished gradient
    [(64, 64, 256)],                                # a 256-row product: 4 splits, the flat order
    [(64, 64, 16384)], [(64, 3, 16384)],            # 128 splits: sixteen slices, then the slice sums
    [(64, 3, 16384), (64, 64, 256), (64, 64, 64)],  # one mixed table
    [(64, 64, 1024), (64, 5, 1088)],                # 16 and 17 splits: the sliced order's first sizes, uneven slices
], ids=lambda s: "+".join("%dx%d@%d" % t for t in s))
def test_folded_edge_weights_backward_is_reduce_then_transform(fsg, device, shapes):
    outs, refs = _fold_jobs(fsg, device, shapes, 11 + len(shapes))
    for (Co, C, M), a, b in zip(shapes, outs, refs):
        assert not torch.isnan(b).any()
        assert _eq(a, b), (Co, C, M, float((a - b).abs().max()))


def test_grouped_products_equal_the_products_alone(fsg, device):
    """fsg_gemm_small_many_deferred_f32: split counts, partials (or the finished product where there is no split) of every job
    against fsg_gemm_small_deferred_f32 on the same operands; dW = g^T x shapes (I, J, M): the EdgeConv ones, one whose X rows
    have stride 192, one without a split, one with ragged tiles and a ragged last split"""
    lib = fsg._lib
    gen = torch.Generator().manual_seed(23)
    shapes = [(128, 64, 16384, 64), (128, 3, 16384, 3), (128, 64, 256, 192), (128, 64, 64, 64), (100, 37, 1000, 37)]
    jobs = lib.GemmSmallJobs()
    jobs.n = len(shapes)
    alone, grouped, keep = [], [], []
    for j, (I, J, M, ldx) in enumerate(shapes):
        g = torch.randn(M, I, generator=gen).to(device)
        x = torch.randn(M, ldx, generator=gen).to(device)[:, :J]
        nbytes = lib.lib.fsg_gemm_small_workspace_bytes(I, J, M)
        outs = []
        for _ in range(2):
            c = torch.full((I, J), float("nan"), device=device)
            ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=device)
            outs.append((c, ws))
        S = ctypes.c_int(-1)
        c, ws = outs[0]
        lib.call("fsg_gemm_small_deferred_f32", g.data_ptr(), 1, I, x.data_ptr(), ldx, 1, c.data_ptr(), J, I, J, M, None,
                 ws.data_ptr(), ctypes.byref(S), _stream())
        alone.append((c, ws, S.value))
        c, ws = outs[1]
        jobs.A[j], jobs.sa_i[j], jobs.sa_k[j], jobs.B[j], jobs.sb_k[j], jobs.sb_j[j] = g.data_ptr(), 1, I, x.data_ptr(), ldx, 1
        jobs.C[j], jobs.ldc[j], jobs.I[j], jobs.J[j], jobs.K[j], jobs.workspace[j] = c.data_ptr(), J, I, J, M, ws.data_ptr()
        jobs.splits[j] = -1
        grouped.append((c, ws))
        keep += [g, x]
    lib.call("fsg_gemm_small_many_deferred_f32", ctypes.byref(jobs), _stream())
    torch.cuda.synchronize()
    assert [a[2] for a in alone] == [128, 128, 4, 0, 11]
    for j, ((I, J, M, _), (c0, ws0, S), (c1, ws1)) in enumerate(zip(shapes, alone, grouped)):
        assert jobs.splits[j] == S, (j, jobs.splits[j], S)
        if S > 1:
            assert not torch.isnan(ws0[:S * I * J]).any() and _eq(ws0[:S * I * J], ws1[:S * I * J]), j
        else:
            assert not torch.isnan(c0).any() and _eq(c0, c1), j


def _graph_case(fsg, device, case, on):
    """two weights of edge_weights_many behind [P | Q] products of 256 rows (4 splits) and 16384 rows (128), every gradient returned"""
    F = fsg.functional
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen).to(device)
    W = r(64, 128).requires_grad_(True)
    W3 = r(64, 6).requires_grad_(True)
    xs = [r(256, 64).requires_grad_(True) for _ in range(2)]
    x3 = r(16384, 3)      # (the K = 3 product is one fsg_gemm_small_f32 takes from about 5500 rows on)
    gs = [r(256, 128), r(256, 128), r(16384, 128)]
    old = F.set_fused_pq_tail(on)
    try:
        with _Spy(fsg) as names:
            w, w3 = F.edge_weights_many([W, W3])
            if case == "retain_grad":
                w.retain_grad()
            loss = (F._LinearPMGiven.apply(xs[0], w, (xs[0] @ w.t()).detach()) * gs[0]).sum()
            if case == "two_uses":
                loss = loss + (F._LinearPMGiven.apply(xs[1], w, (xs[1] @ w.t()).detach()) * gs[1]).sum()
            loss = loss + (F.linear_pm(x3, w3) * gs[2]).sum()       # the K = 3 product through the ordinary Linear
            if case == "create_graph":
                grads = torch.autograd.grad(loss, [W, W3, xs[0]], create_graph=True)
            else:
                loss.backward()
                grads = [W.grad, W3.grad, xs[0].grad] + ([xs[1].grad] if case == "two_uses" else [])
                grads += [w.grad] if case == "retain_grad" else []
            torch.cuda.synchronize()
    finally:
        F.set_fused_pq_tail(old)
    return [g.detach() for g in grads], names


@pytest.mark.parametrize("case", ["one_use", "two_uses", "create_graph", "retain_grad"])
def test_unreduced_weight_gradients_only_where_sound(fsg, device, case):
    """switch on == switch off in every gradient; the unreduced route is taken by a weight with ONE product outside create_graph
    and by nothing else (a second use would have autograd add bytes that are not there yet, create_graph may read the gradient, and
    a [P | Q] weight that retains its gradient must find the finished product in it)"""
    on, n_on = _graph_case(fsg, device, case, True)
    off, n_off = _graph_case(fsg, device, case, False)
    assert len(on) == len(off) and all(_eq(a, b) for a, b in zip(on, off))
    assert "fsg_edge_weights_bwd_folded_f32" not in n_off and "fsg_gemm_small_many_deferred_f32" not in n_off
    products = lambda n: sum(x in ("fsg_gemm_small_rowsum_f32", "fsg_gemm_small_many_deferred_f32") for x in n)
    if case == "create_graph":
        assert "fsg_edge_weights_bwd_folded_f32" not in n_on and "fsg_gemm_small_many_deferred_f32" not in n_on
    else:       # (two_uses, retain_grad: the products of W run and reduce at once, W3 -- one product -- is still left to the tail)
        assert n_on.count("fsg_edge_weights_bwd_folded_f32") == 1 and n_on.count("fsg_gemm_small_many_deferred_f32") == 1
        assert products(n_off) - products(n_on) == (1 if case == "one_use" else 0)


def test_dgcnn_step_gradients_equal_with_and_without_the_folded_tail(fsg, device):
    """DGCNN-seg, 2 x 256 points, k = 20: every parameter gradient with the tail folded and not (the three [P | Q] weights go
    through _LinearPMGiven, the first behind K = 3 input channels)"""
    from fissure_segmentation_amd.models.dgcnn import DGCNNSeg
    F = fsg.functional
    torch.manual_seed(3)
    net = DGCNNSeg(k=20, in_features=3, num_classes=4).to(device).train()
    x = torch.randn(2, 3, 256, device=device)
    res = []
    for on in (True, False):
        old = F.set_fused_pq_tail(on)
        try:
            net.zero_grad(set_to_none=True)
            with _Spy(fsg) as names:
                net(x).square().mean().backward()
            torch.cuda.synchronize()
        finally:
            F.set_fused_pq_tail(old)
        res.append(([p.grad.clone() for p in net.parameters()], names))
    (g_on, n_on), (g_off, n_off) = res
    assert ("fsg_edge_weights_bwd_folded_f32" in n_on) and ("fsg_edge_weights_bwd_folded_f32" not in n_off)
    assert all(_eq(a, b) for a, b in zip(g_on, g_off))


# ------------------------------------------------------------------------------------------------ C: Adam without the copy
def _adam_pair(fsg, device, shapes, wd, missing=(), lr_tensor=False, steps=20):
    """`steps` steps of FlatAdam.step() and of gather_grads() + step_flat() from the same parameters and gradients ->
    (optimizer, optimizer, entries called by step())"""
    from fissure_segmentation_amd.optim import FlatAdam
    gen = torch.Generator().manual_seed(len(shapes) + 17)
    init = [torch.randn(*s, generator=gen) for s in shapes]
    opts = []
    for _ in range(2):
        ps = [torch.nn.Parameter(t.clone().to(device)) for t in init]
        lr = torch.tensor([1e-2], device=device) if lr_tensor else 1e-2
        opts.append(FlatAdam(ps, lr=lr, weight_decay=wd))
    names = []
    for step in range(steps):
        grads = [torch.randn(*s, generator=gen) * 10.0 ** (step % 5 - 2) for s in shapes]
        for o in opts:
            for i, (p, g) in enumerate(zip(o.params, grads)):
                p.grad = None if i in missing else g.clone().to(device)
        with _Spy(fsg) as n:
            opts[0].step()
        names += n
        if missing:     # the reference for a missing gradient is the step's own fallback (value and moments kept)
            opts[1].step()
        else:
            opts[1].gather_grads()
            opts[1].step_flat()
    torch.cuda.synchronize()
    return opts[0], opts[1], names


def _same_state(a, b):
    return (_eq(a.flat.data, b.flat.data) and _eq(a.exp_avg, b.exp_avg) and _eq(a.exp_avg_sq, b.exp_avg_sq) and
            _eq(a.flat.grad, b.flat.grad) and _eq(a._state, b._state))


@pytest.mark.parametrize("wd,lr_tensor", [(0.0, False), (1e-2, True)])
def test_adam_reads_gradients_in_place(fsg, device, wd, lr_tensor):
    """small and large parameters (the large ones span many chunks of the kernel's table, the largest more than one stride of a
    chunk's workgroups): parameters, both moments, the flat gradient buffer and the step counter, bit for bit"""
    shapes = [(16, 8), (16,), (4, 16), (4,), (300, 1000), (1024, 1024), (64,)]
    a, b, names = _adam_pair(fsg, device, shapes, wd, lr_tensor=lr_tensor)
    assert names.count("fsg_adam_flat_segments_f32") == 20 and "fsg_adam_flat_f32" not in names
    assert float(a._state[0]) == 20.0 and _same_state(a, b)
    assert _eq(a.flat.grad, torch.cat([p.grad.reshape(-1) for p in a.params]))


def test_adam_falls_back_on_a_three_element_parameter(fsg, device):
    a, b, names = _adam_pair(fsg, device, [(16, 8), (3,), (4, 16)], 0.0)
    assert names.count("fsg_adam_flat_f32") == 20 and "fsg_adam_flat_segments_f32" not in names
    assert _same_state(a, b)


def test_adam_falls_back_on_a_missing_gradient(fsg, device):
    shapes = [(16, 8), (16,), (4, 16)]
    a, b, names = _adam_pair(fsg, device, shapes, 0.0, missing=(1,))
    assert names.count("fsg_adam_flat_f32") == 20 and "fsg_adam_flat_segments_f32" not in names
    assert _same_state(a, b)
    full, _, _ = _adam_pair(fsg, device, shapes, 0.0)          # same seed, same gradients, none missing
    lo, hi = a._spans[1]
    assert _eq(a.flat.data[:lo], full.flat.data[:lo]) and _eq(a.flat.data[hi:], full.flat.data[hi:])
    assert not a.exp_avg[lo:hi].any() and not a.exp_avg_sq[lo:hi].any() and not a.flat.grad[lo:hi].any()
