"""GPU tests of the last two stages of a training step one by one against tests/loss_oracle.py (float64): fsg_nnu_loss_f32
(csrc/seg_loss.hip: cross-entropy + generalised Dice, value and gradient), fsg_chamfer_nn_f32 / _bwd_f32 (csrc/chamfer.hip: the
atomic and the ordered backward, the latter through fsg_csr_bipartite_launch of csrc/edgeconv.hip with NS != N) and
fsg_adam_flat_f32 / fsg_adam_flat_segments_f32 (csrc/adam.hip), at the grid, tile, tie and label edges listed in loss_oracle's
case tables (pinned by tests/test_loss_oracle_cpu.py).

How a value is judged (`judge`, the rule of tests/test_bn_family_gpu.py with FLOOR and MARGIN of tests/test_pw_family_gpu.py):
max |got - fp64| / mag, mag the sum of the absolute summands of that value (loss_oracle's `mag`), against max(1e-6, 2 x the same
figure of an fp32 yardstick on the GPU): ATen's F.cross_entropy(weight=w) + the Dice closed form under autograd on the valid points
for the segmentation loss, the oracle's own statement in fp32 torch ops (gather / scatter_add_ from the same arg) for the Chamfer
gradients, torch.optim.Adam in fp32 over the same tensors for Adam (the oracle's fp32 run where the step count does not start at
0).  The scalars total, ce and gdl are judged relative to their fp64 value with the floor 4 x 2^-24 (the kernel sums in fp64 and
rounds once).  An element without summands (mag == 0: the gradient row of an invalid label, a Chamfer target nobody selects or
whose queries all carry g == 0) must be exactly 0.  Every figure is printed before it is asserted (`LOSSFAM <case> <quantity>
kernel ... yardstick ...`); profiles/loss_family_parity.txt holds one run.  Chamfer's arg is compared bit for bit with
oracle/c_api.chamfer_nn and then handed to the oracle, so no fp32 / fp64 near-tie can make the two disagree and no row is left out.

One assertion of this module is about torch and not about the kernels: a leaf that is a SLICE of a larger tensor gets a contiguous
.grad from autograd's accumulation (its layout contract keeps the strides of dense tensors only), whatever the backward returns.
The strided-input test therefore asserts the strides of the buffer the kernel wrote (the autograd node's `grad`) for all three
views and x.grad.stride() == x.stride() for the dense point-major one.

MEASURED on an MI355X (profiles/loss_family_parity.txt, 404 figures, all under their bars).
  seg loss  99 scalar figures, the largest 8.9e-8 (total at w_ce 0.3, w_dice 2; ATen 9.2e-8), 0.37 of the bar 2.4e-7.  Gradient: 35
            of 36 under the floor, the largest of those 8.1e-7 at C = 32 (ATen 1.0e-6); past the grid cap 5.3e-7 at 3 x 5462 and
            6.1e-7 at 7 x 7033 (ATen 7.0e-7, 7.7e-7).  The one above the floor is logits of scale 40, 3.6e-6 against ATen's 5.9e-6:
            z - max of two fp32 logits 90 apart rounds to half an ulp of 64 .. 128 = 3.8e-6, which exp() turns into a relative
            error of p.
  Chamfer   all 36 under the floor; the largest 1.3e-7 (grad_y of the accumulate call, atomic path; torch 6.7e-8), 0.13 of the
            bar.  Ordered grad_y with 1365 in-edges per target (4096 -> 3, the `tmp` sort branch): 5.4e-8 (torch's atomics
            9.5e-9).  The fall-back above 16384 targets (300 -> 16400): 9.2e-8, as the atomic path.
  Adam      all 233 under the floor; the largest 4.9e-7 (exp_avg_sq of the segments kernel, weight decay 0.01, step 2;
            torch.optim.Adam 4.2e-7), 0.49 of the bar.  Tail-only sizes 1, 2, 3: at most 1.1e-7.
One finding, in load_softmax of csrc/seg_loss.hip: log p_y was z_y - (max + log s); with +1e4 on every logit max + log s rounds to
an ulp of 1e4 = 9.8e-4 per point and `total` was 7.75e-7 off its float64 value (bar 2.4e-7, ATen 9.3e-8).  It is now
(z_y - max) - log s: 8.1e-9.  The gradient never used log p_y.  What stays as it is and is documented instead: the ordered Chamfer
backward above 16384 targets runs the atomics (functional.set_deterministic's docstring).
Two things the older tests of these kernels did not do although their text says so: test_flat_adam_matches_torch_adam's shapes hold
4684 elements, a multiple of 4, so the tail branch of adam_flat_kernel never ran; and no label outside [0, C) was ever passed.
Mutants tried on the GPU, each failing here while the older tests of the same kernels pass: g indexed without the cloud in
chamfer_bwd_kernel (chamfer 700to450); nnu_grad_kernel stopped after one grid-stride iteration (pts-3x5462, pts-3x5462-now,
pts-7x7033); `yl >= 0 && yl < C` weakened to `yl < C` (lab-wrap32 only: a negative label still reads as negative after the
conversion to int, so -1 and -100 stay skipped; -2^32 + 1 reads as class 1); the tail branch of adam_flat_kernel removed (every
size but 4).
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_oracle as lo
from oracle import c_api

pytestmark = pytest.mark.gpu

FLOOR, MARGIN = 1e-6, 2.0          # tests/test_pw_family_gpu.py
REL_FLOOR = 4 * 2.0 ** -24         # fp64 inside, one rounding to fp32 on the way out
SENTINEL = -777.25


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def G(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)          # a copy: the shared case inputs are read-only


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def judge(name, got, yard, ref, mag, floor=FLOOR):
    """max |got - ref| / mag against max(floor, MARGIN x the yardstick's); yard None: the floor alone.  An element without summands
    (mag == 0) must equal the reference, which is 0 there, exactly, and takes no part in either figure."""
    ref, mag = ref.to(got.device), mag.to(got.device)
    assert got.shape == ref.shape == mag.shape, (name, got.shape, ref.shape, mag.shape)
    assert bool(torch.isfinite(got).all()), name
    none = mag == 0
    assert bool((got.double()[none] == ref[none]).all()), (name, "a value without summands must be exact")
    safe = torch.where(none, torch.ones_like(mag), mag)

    def figure(x):
        return float(((x.double() - ref).abs() / safe).masked_fill(none, 0.0).max()) if ref.numel() else 0.0
    e_k = figure(got)
    e_y = None if yard is None else figure(yard)
    print("LOSSFAM %-52s kernel %.3g  yardstick %s" % (name, e_k, "-" if e_y is None else "%.3g" % e_y))
    assert e_y is None or e_y < 1.0, (name, "the yardstick itself is off", e_y)
    assert e_k <= max(floor, MARGIN * (e_y or 0.0)), (name, e_k, e_y)
    return e_k


def judge_rel(name, got, yard, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
    judge(name, got.reshape(-1), None if yard is None else yard.reshape(-1), ref, ref.abs(), floor=REL_FLOOR)


_refs = {}


def shared(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


# --------------------------------------------------------------------------------------------------------------------- seg loss

def seg_tensors(d, device):
    return G(d["logits"], device), G(d["labels"], device), (G(d["w"], device) if d["w"] is not None else None)


def seg_kernel(fsg, x, y, w, w_ce=1.0, w_dice=1.0, smooth=1.0):
    """functional.nnu_loss forward + backward on the leaf made of x (its strides kept)"""
    x = x.detach().requires_grad_(True)
    total, ce, gdl = fsg.functional.nnu_loss(x, y, w, w_ce, w_dice, smooth)
    wrote = total.grad_fn.grad.stride()
    total.backward()
    torch.cuda.synchronize()
    return dict(total=total.detach(), ce=ce.detach(), gdl=gdl.detach(), grad=x.grad, wrote=wrote, leaf=x)


def seg_aten(x, y, w, w_ce=1.0, w_dice=1.0, smooth=1.0):
    """the fp32 yardstick: ATen on the GPU over the valid points, autograd, the rows of the others zero"""
    B, C, N = x.shape
    yf = y.reshape(-1)
    valid = (yf >= 0) & (yf < C)
    zv = x.permute(0, 2, 1).reshape(-1, C)[valid].clone().requires_grad_(True)
    total, ce, gdl = lo.nnu_autograd(zv, yf[valid], w, w_ce, w_dice, smooth)
    total.backward()
    rows = torch.zeros(B * N, C, dtype=torch.float32, device=x.device)
    rows[valid] = zv.grad
    return dict(total=total.detach(), ce=ce.detach(), gdl=gdl.detach(), grad=rows.view(B, N, C).permute(0, 2, 1))


def seg_direct(fsg, x, y, w, grad, w_ce=1.0, w_dice=1.0, smooth=1.0):
    """one call of the C entry point -> loss_out (4,); grad None or a (B, C, N) tensor written through its own strides"""
    B, C, N = x.shape
    vals = torch.full((4,), SENTINEL, dtype=torch.float32, device=x.device)
    ws = fsg._lib.workspace("fsg_nnu_loss", C, device=x.device)
    gs = grad.stride() if grad is not None else (0, 0, 0)
    fsg._lib.call("fsg_nnu_loss_f32", P(x), x.stride(0), x.stride(1), x.stride(2), P(y), P(w), B, C, N, float(w_ce), float(w_dice),
                  float(smooth), P(vals), P(grad), gs[0], gs[1], gs[2], P(ws), _stream())
    torch.cuda.synchronize()
    return vals


def check_seg(name, got, aten, ref):
    for k in ("total", "ce", "gdl"):
        judge_rel("%s %s" % (name, k), got[k], aten[k], ref[k])
    judge("%s grad" % name, got["grad"], aten["grad"], ref["grad"], ref["mag"])


@pytest.mark.parametrize("case", lo.SEG_CASES, ids=lo.seg_id)
def test_nnu_loss_vs_fp64(fsg, device, case):
    """every SEG_CASES entry through functional.nnu_loss: total, ce, gdl and the gradient against the masked float64 oracle; through
    the C entry point: loss_out[3] == the number of labels outside [0, C), their gradient rows exactly 0.0, and with grad == NULL
    (one workgroup instead of up to 64) the same bits in loss_out[0..2]"""
    d = lo.seg_inputs(case)
    ref = shared(("seg", case[0]), lambda: lo.seg_oracle(case))
    x, y, w = seg_tensors(d, device)
    got, aten = seg_kernel(fsg, x, y, w), seg_aten(x, y, w)
    check_seg("seg " + case[0], got, aten, ref)
    B, C, N = x.shape
    bad = ((y < 0) | (y >= C))
    assert bool((got["grad"].permute(0, 2, 1)[bad] == 0).all())
    grad = torch.full_like(x, SENTINEL)
    vals = seg_direct(fsg, x, y, w, grad)
    assert float(vals[3]) == float(ref["n_bad"]) == float(bad.sum())
    assert torch.equal(grad, got["grad"]) and torch.equal(vals[:3], torch.stack((got["total"], got["ce"], got["gdl"])))
    no_grad = seg_direct(fsg, x, y, w, None)
    assert torch.equal(no_grad.view(torch.int32), vals.view(torch.int32)), "grad == NULL must not change the values"


@pytest.mark.parametrize("smooth", lo.SEG_SMOOTH)
@pytest.mark.parametrize("w_ce,w_dice", lo.SEG_PARAMS)
def test_nnu_loss_weights_and_smooth(fsg, device, w_ce, w_dice, smooth):
    case = lo.seg_case("C-5")
    ref = lo.seg_oracle(case, w_ce, w_dice, smooth)
    x, y, w = seg_tensors(lo.seg_inputs(case), device)
    got, aten = seg_kernel(fsg, x, y, w, w_ce, w_dice, smooth), seg_aten(x, y, w, w_ce, w_dice, smooth)
    check_seg("seg w_ce %g w_dice %g smooth %g" % (w_ce, w_dice, smooth), got, aten, ref)


@pytest.mark.parametrize("view", ["channel_slice", "point_slice", "point_major"])
def test_nnu_loss_strided_views(fsg, device, view):
    """logits that are a channel slice big[:, 1:1 + C, :], a point slice big[:, :, 5:5 + N] or the point-major view of (B, N, C)
    memory: the same bits as the contiguous tensor, the gradient written with the input's strides, nothing outside the view touched"""
    case = lo.seg_case("C-5")
    ref = shared(("seg", case[0]), lambda: lo.seg_oracle(case))
    x, y, w = seg_tensors(lo.seg_inputs(case), device)
    B, C, N = x.shape

    def carve(fill):
        if view == "channel_slice":
            big = torch.full((B, C + 3, N), fill, dtype=torch.float32, device=device)
            return big, big[:, 1:1 + C, :]
        if view == "point_slice":
            big = torch.full((B, C, N + 9), fill, dtype=torch.float32, device=device)
            return big, big[:, :, 5:5 + N]
        big = torch.full((B, N, C), fill, dtype=torch.float32, device=device)
        return big, big.transpose(1, 2)
    big, xv = carve(3.0)
    xv.copy_(x)
    assert not xv.is_contiguous() and xv.stride() != x.stride()
    base = seg_kernel(fsg, x, y, w)
    got = seg_kernel(fsg, xv, y, w)
    assert got["leaf"].stride() == xv.stride()
    assert got["wrote"] == xv.stride(), "the kernel's gradient buffer has the strides of the logits"
    dense = view == "point_major"
    assert got["grad"].stride() == (xv.stride() if dense else x.stride())       # autograd's layout contract, see the module docstring
    for k in ("total", "ce", "gdl", "grad"):
        assert torch.equal(got[k], base[k]), k
    judge("seg view %s grad" % view, got["grad"], seg_aten(x, y, w)["grad"], ref["grad"], ref["mag"])
    gbig, gv = carve(SENTINEL)
    vals = seg_direct(fsg, xv, y, w, gv)
    assert torch.equal(gv, base["grad"]) and torch.equal(vals[:3], torch.stack((base["total"], base["ce"], base["gdl"])))
    inside = torch.zeros_like(gbig, dtype=torch.bool)
    {"channel_slice": lambda: inside[:, 1:1 + C, :], "point_slice": lambda: inside[:, :, 5:5 + N],
     "point_major": lambda: inside}[view]().fill_(True)
    assert bool((gbig[~inside] == SENTINEL).all()), "memory outside the view must stay as it was"
    assert bool((big[~inside] == 3.0).all())


def test_nnu_loss_is_reproducible_past_the_grid_cap(fsg, device):
    """49231 points (three to four grid-stride iterations per thread): a second run gives the same bits, value and gradient"""
    x, y, w = seg_tensors(lo.seg_inputs(lo.seg_case("pts-7x7033")), device)
    a, b = seg_kernel(fsg, x, y, w), seg_kernel(fsg, x, y, w)
    for k in ("total", "ce", "gdl", "grad"):
        assert torch.equal(a[k], b[k]), k


# --------------------------------------------------------------------------------------------------------------------- Chamfer

def chamfer_fwd_exact(fsg, device, x, y):
    dist, arg = fsg.functional.chamfer_nn(G(x, device), G(y, device))
    rd, ra = c_api.chamfer_nn(x, y)
    assert np.array_equal(arg.cpu().numpy(), ra), "arg"
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), rd.view(np.uint32)), "dist bits"
    return dist, arg


@pytest.mark.parametrize("case", lo.CH_FWD, ids=lo.ch_fwd_id)
def test_chamfer_nn_tile_edges_exact(fsg, device, case):
    """dist and arg bit for bit against the C oracle around the query tile (128, two per lane) and the candidate tile (1024 over
    eight waves of 128)"""
    d = lo.ch_fwd_inputs(case)
    chamfer_fwd_exact(fsg, device, d["x"], d["y"])


def test_chamfer_nn_ties_take_the_lowest_index(fsg, device):
    """duplicated targets in two wave slices of a tile, in the last slice of tile 0 and the first of tile 1, in the same wave of two
    tiles, and a triple over three tiles: queries exactly on the point get distance 0 and the LOWEST of the indices; a lattice
    block (coordinates rounded to 1 / 4) with many exactly equal distances equals the sequential scan of the C oracle"""
    d = lo.tie_inputs()
    dist, arg = chamfer_fwd_exact(fsg, device, d["x"], d["y"])
    for k, grp in enumerate(lo.TIE_GROUPS):
        q = slice(lo.TIE_Q * k, lo.TIE_Q * (k + 1))
        assert bool((arg[:, q] == grp[0]).all()) and bool((dist[:, q] == 0).all()), grp
    assert not bool(torch.isin(arg, torch.tensor([j for grp in lo.TIE_GROUPS for j in grp[1:]], device=device, dtype=arg.dtype)).any())
    lat = lo.lattice_inputs()
    chamfer_fwd_exact(fsg, device, lat["x"], lat["y"])


def chamfer_backward(fsg, x, y, g, deterministic):
    F = fsg.functional
    was = F._deterministic
    F.set_deterministic(deterministic)
    try:
        xt, yt = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
        dist, arg = F.chamfer_nn(xt, yt)
        dist.backward(g)
        torch.cuda.synchronize()
    finally:
        F.set_deterministic(was)
    return xt.grad, yt.grad, arg


@pytest.mark.parametrize("case", lo.CH_BWD, ids=lo.ch_bwd_id)
def test_chamfer_backward_vs_fp64(fsg, device, case):
    """functional.chamfer_nn(x, y)[0] under a random incoming gradient (mixed signs, exact zeros, another scale per cloud), the
    atomic and the ordered path against the float64 gradient from the kernel's own arg; ordered: two runs and cloud 0 alone give the
    same bits (up to the 16384 targets the reverse-graph builder takes; above it falls back to atomics and is judged like them);
    the higher-index copy of a duplicated target receives exactly zero"""
    N, M, dup, _ = case
    d = lo.ch_bwd_inputs(case)
    x, y, g = G(d["x"], device), G(d["y"], device), G(d["g"], device)
    name = "chamfer " + lo.ch_bwd_id(case)
    gx_a, gy_a, arg = chamfer_backward(fsg, x, y, g, False)
    _, ra = c_api.chamfer_nn(d["x"], d["y"])
    assert np.array_equal(arg.cpu().numpy(), ra)
    ref = lo.chamfer_bwd(lo.T(d["x"]), lo.T(d["y"]), arg.cpu(), lo.T(d["g"]))
    yard = lo.chamfer_bwd(x, y, arg, g, dtype=torch.float32)
    gx_o, gy_o, arg_o = chamfer_backward(fsg, x, y, g, True)
    assert torch.equal(arg_o, arg)
    for path, gx, gy in (("atomic", gx_a, gy_a), ("ordered", gx_o, gy_o)):
        judge("%s %s grad_x" % (name, path), gx, yard["grad_x"], ref["grad_x"], ref["mag_x"])
        judge("%s %s grad_y" % (name, path), gy, yard["grad_y"], ref["grad_y"], ref["mag_y"])
        if dup:
            assert bool((gy[:, dup[1]] == 0).all()) and bool((gy[:, dup[0]] != 0).any())
    assert torch.equal(gx_a, gx_o)                     # one writer per query point on both paths
    if M <= lo.CH_ORDERED_MAX_M:
        gx_2, gy_2, _ = chamfer_backward(fsg, x, y, g, True)
        assert torch.equal(gx_2, gx_o) and torch.equal(gy_2, gy_o), "the ordered path must be reproducible"
        gx_0, gy_0, _ = chamfer_backward(fsg, x[:1], y[:1], g[:1], True)
        assert torch.equal(gx_0, gx_o[:1]) and torch.equal(gy_0, gy_o[:1]), "a cloud must not depend on its batch"


@pytest.mark.parametrize("ordered", [False, True])
def test_chamfer_backward_accumulates(fsg, device, ordered):
    """the header's contract: _bwd ACCUMULATES into grad_x and grad_y (the caller zero-fills).  One call of the C entry point on
    buffers that hold random values, without and with workspace: pre-fill + gradient."""
    case = lo.CH_BWD[0]
    d = lo.ch_bwd_inputs(case)
    B, (N, M) = 2, case[:2]
    x, y, g = (G(d[k][:B], device) for k in ("x", "y", "g"))
    _, arg = fsg.functional.chamfer_nn(x, y)
    rng = np.random.default_rng(5)
    fx, fy = rng.standard_normal((B, N, 3)).astype(np.float32), rng.standard_normal((B, M, 3)).astype(np.float32)
    gx, gy = G(fx, device), G(fy, device)
    ws = fsg._lib.workspace("fsg_chamfer_nn_bwd", B, N, M, device=device) if ordered else None
    fsg._lib.call("fsg_chamfer_nn_bwd_f32", P(x), P(y), P(arg), P(g), B, N, M, P(gx), P(gy), P(ws), _stream())
    torch.cuda.synchronize()
    ref = lo.chamfer_bwd(lo.T(d["x"][:B]), lo.T(d["y"][:B]), arg.cpu(), lo.T(d["g"][:B]))
    yard = lo.chamfer_bwd(x, y, arg, g, dtype=torch.float32)
    name = "chamfer accumulate %s" % ("ordered" if ordered else "atomic")
    judge(name + " grad_x", gx, G(fx, device) + yard["grad_x"], lo.T(fx) + ref["grad_x"], lo.T(fx).abs() + ref["mag_x"])
    judge(name + " grad_y", gy, G(fy, device) + yard["grad_y"], lo.T(fy) + ref["grad_y"], lo.T(fy).abs() + ref["mag_y"])


# --------------------------------------------------------------------------------------------------------------------- Adam

HP32 = {k: lo.f32(v) for k, v in lo.ADAM_HP.items()}


def flat_adam(fsg, params, lr, wd):
    from fissure_segmentation_amd.optim import FlatAdam
    return FlatAdam(params, lr=lr, betas=(lo.ADAM_HP["b1"], lo.ADAM_HP["b2"]), eps=lo.ADAM_HP["eps"], weight_decay=wd)


def torch_adam(params, wd):
    return torch.optim.Adam(params, lr=lo.f32(lo.ADAM_LR[0]), betas=(HP32["b1"], HP32["b2"]), eps=HP32["eps"], weight_decay=lo.f32(wd))


def state_of(opt):
    """(step, ticket) of a FlatAdam's device state block"""
    torch.cuda.synchronize()
    return float(opt._state[0]), int(opt._state.view(torch.int32)[1])


def yard_moments(yopt, params):
    return (torch.cat([yopt.state[p]["exp_avg"].reshape(-1) for p in params]),
            torch.cat([yopt.state[p]["exp_avg_sq"].reshape(-1) for p in params]))


def check_adam_step(name, opt, yparams, yopt, ref):
    ym, yv = yard_moments(yopt, yparams)
    yp = torch.cat([p.detach().reshape(-1) for p in yparams])
    judge(name + " p", opt.flat.data, yp, ref["p"], ref["mag_p"])
    judge(name + " m", opt.exp_avg, ym, ref["m"], ref["mag_m"])
    judge(name + " v", opt.exp_avg_sq, yv, ref["v"], ref["mag_v"])


def check_adam_blocks(n, wd, s, p0, prev, opt):
    """the element blocks of a fixture after step s (prev: exp_avg, exp_avg_sq before it)"""
    b = lo.adam_blocks(n)
    p, m, v = opt.flat.data, opt.exp_avg, opt.exp_avg_sq
    if wd == 0:
        z = b["zero"]
        assert torch.equal(p[z], p0[z]), "g == 0 and no weight decay: the parameter must not move"
        assert bool((m[z] == 0).all()) and bool((v[z] == 0).all())
        t = b["tiny"]
        assert bool((v[t] < lo.TINY32).all()), "v of |g| = 1e-20 lies below fp32's normal range"
        if s >= 2:                                     # g == 0 from step 3 on: v decays by exactly b2, m shrinks
            lz = b["late_zero"]
            assert torch.equal(v[lz], prev[1][lz] * HP32["b2"]) and bool((v[lz] > 0).all())
            assert bool((m[lz].abs() < prev[0][lz].abs()).all())
    assert bool(torch.isfinite(p).all())


ADAM_FLAT_CASES = [(n, wd, "device" if wd else "host") for n in lo.ADAM_FLAT_N for wd in lo.ADAM_WD] + \
                  [(1023, 0.0, "device"), (1023, 1e-2, "host")]


@pytest.mark.parametrize("n,wd,lr_kind", ADAM_FLAT_CASES)
def test_adam_flat_vs_fp64(fsg, device, n, wd, lr_kind):
    """fsg_adam_flat_f32 through optim.FlatAdam (gather_grads + step_flat), four steps with a learning rate changed before step 3 (a
    device tensor or the host value) and another gradient scale per step: p, exp_avg, exp_avg_sq after every step against float64;
    the device step count equals the number of calls and the ticket is back at 0; the g == 0, |g| = 1e-20 and +-1e3 blocks; first
    step without weight decay: |dp| = lr |g| / (|g| + eps) (m / (1 - b1) = g and sqrt(v / (1 - b2)) = |g| at t = 1; eps is added
    AFTER the bias correction in this rule, so it is not scaled by sqrt(1 - b2): with |g| = 1e-6 that variant is 1e-4 lr off)"""
    d = lo.adam_inputs(n)
    ref = shared(("adam", n, wd), lambda: lo.adam_oracle(n, wd))
    p = torch.nn.Parameter(G(d["p"], device))
    lr = torch.tensor([lo.ADAM_LR[0]], dtype=torch.float32, device=device) if lr_kind == "device" else lo.ADAM_LR[0]
    opt = flat_adam(fsg, [p], lr, wd)
    yp = torch.nn.Parameter(G(d["p"], device))
    yopt = torch_adam([yp], wd)
    p0 = G(d["p"], device)
    name = "adam flat n %d wd %g lr %s" % (n, wd, lr_kind)
    for s in range(lo.ADAM_STEPS):
        if lr_kind == "device":
            lr.fill_(lo.ADAM_LR[s])
        else:
            opt.param_groups[0]["lr"] = lo.ADAM_LR[s]
        yopt.param_groups[0]["lr"] = lo.f32(lo.ADAM_LR[s])
        prev = (opt.exp_avg.clone(), opt.exp_avg_sq.clone())
        p.grad, yp.grad = G(d["g"][s], device), G(d["g"][s], device)
        opt.gather_grads()
        opt.step_flat()
        yopt.step()
        assert state_of(opt) == (s + 1.0, 0)
        check_adam_step("%s step %d" % (name, s + 1), opt, [yp], yopt, ref[s])
        if n >= lo.ADAM_BLOCK_MIN_N:
            check_adam_blocks(n, wd, s, p0, prev, opt)
        if s == 0 and wd == 0:
            g64 = lo.T(d["g"][0])
            want = -lo.f32(lo.ADAM_LR[0]) * g64 / (g64.abs() + HP32["eps"])
            judge("%s first step dp" % name, opt.flat.data.double() - p0.double(), yp.detach().double() - p0.double(), want,
                  ref[0]["mag_p"])


@pytest.mark.parametrize("wd", lo.ADAM_WD)
def test_adam_segments_vs_fp64_and_flat_kernel(fsg, device, wd):
    """fsg_adam_flat_segments_f32 (optim.FlatAdam.step with every gradient in place) on five parameters of 1 049 132 elements: chunks
    of 1198 float4 for workgroups of 1024 threads, a short last chunk per parameter.  Against float64 directly, bit-equal to the
    flat kernel, and the flat gradient buffer holds the concatenation afterwards."""
    sizes = [int(np.prod(s)) for s in lo.ADAM_SEG_SHAPES]
    n = sum(sizes)
    d = lo.adam_inputs(n)
    ref = shared(("adam", n, wd), lambda: lo.adam_oracle(n, wd))
    cuts = np.cumsum([0] + sizes)

    def split(a):
        return [G(a[cuts[i]:cuts[i + 1]].reshape(shape), device) for i, shape in enumerate(lo.ADAM_SEG_SHAPES)]
    pa, pb, py = ([torch.nn.Parameter(t) for t in split(d["p"])] for _ in range(3))
    seg, flat, yopt = flat_adam(fsg, pa, lo.ADAM_LR[0], wd), flat_adam(fsg, pb, lo.ADAM_LR[0], wd), torch_adam(py, wd)
    p0 = G(d["p"], device)
    for s in range(lo.ADAM_STEPS):
        for o in (seg, flat, yopt):
            o.param_groups[0]["lr"] = lo.ADAM_LR[s] if o is not yopt else lo.f32(lo.ADAM_LR[s])
        prev = (seg.exp_avg.clone(), seg.exp_avg_sq.clone())
        for params in (pa, pb, py):
            for q, t in zip(params, split(d["g"][s])):
                q.grad = t
        assert seg._grad_segments() is not None, "the in-place path must be the one that runs"
        seg.flat.grad.fill_(SENTINEL)
        seg.step()
        flat.gather_grads()
        flat.step_flat()
        yopt.step()
        assert state_of(seg) == (s + 1.0, 0) and state_of(flat) == (s + 1.0, 0)
        assert torch.equal(seg.flat.grad, G(d["g"][s], device))
        for a, b in ((seg.flat.data, flat.flat.data), (seg.exp_avg, flat.exp_avg), (seg.exp_avg_sq, flat.exp_avg_sq)):
            assert torch.equal(a, b), "segments kernel == flat kernel, bit for bit"
        check_adam_step("adam segments wd %g step %d" % (wd, s + 1), seg, py, yopt, ref[s])
        check_adam_blocks(n, wd, s, p0, prev, seg)


def test_adam_ticket_is_reused_across_grid_sizes(fsg, device):
    """ONE state block through three calls of the C entry point with 1024, 1 and 5 workgroups: the step reads 1, 2, 3, the ticket 0
    after each, and each result is the rule at t = 1, 2, 3 (yardstick: the oracle's fp32 run)"""
    state = torch.zeros(2, dtype=torch.float32, device=device)
    lr, wd = 1e-2, 1e-2
    for k, n in enumerate(lo.ADAM_TICKET_N):
        d = lo.adam_inputs(n)
        p, g = G(d["p"], device), G(d["g"][0], device)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        fsg._lib.call("fsg_adam_flat_f32", P(p), P(g), P(m), P(v), P(state), n, lr, None, lo.ADAM_HP["b1"], lo.ADAM_HP["b2"],
                      lo.ADAM_HP["eps"], wd, _stream())
        torch.cuda.synchronize()
        assert float(state[0]) == k + 1.0 and int(state.view(torch.int32)[1]) == 0
        ref = lo.adam(lo.T(d["p"]), [lo.T(d["g"][0])], [lr], wd=wd, t0=k, **lo.ADAM_HP)[0]
        y = lo.adam(G(d["p"], device), [G(d["g"][0], device)], [lr], wd=wd, t0=k, dtype=torch.float32, **lo.ADAM_HP)[0]
        name = "adam ticket call %d n %d" % (k + 1, n)
        judge(name + " p", p, y["p"], ref["p"], ref["mag_p"])
        judge(name + " m", m, y["m"], ref["m"], ref["mag_m"])
        judge(name + " v", v, y["v"], ref["v"], ref["mag_v"])
