"""CPU tests of tests/loss_oracle.py, the float64 reference of the segmentation loss, the Chamfer backward and Adam: its closed forms
against oracle/ref_cpu.py (nnu_loss, chamfer) under float64 autograd, against the committed figures of the real reference
(tests/golden/nnu_loss.npz) and against torch.optim.Adam on float64 parameters, and the pins on the generated inputs that
tests/test_loss_family_gpu.py relies on: the duplicated targets are exactly the intended ones, the Adam fixtures hold the g == 0,
tiny-g and +-1e3 blocks they claim, every segmentation case has a point of every class it does not drop on purpose and the
number of invalid labels it claims."""
import numpy as np
import pytest
import torch

import loss_oracle as lo
from golden_util import load, seg_loss_case
from oracle import ref_cpu

RTOL = 1e-12


def close(name, got, want, mag=None, rtol=RTOL):
    """|got - want| <= rtol x mag element by element (mag: the sum of absolute summands, |want| when none is given)"""
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    mag = want.abs() if mag is None else mag.expand_as(want)
    err = float(((got - want).abs() / mag.clamp_min(1e-300)).max()) if want.numel() else 0.0
    assert err <= rtol, (name, err)


# --------------------------------------------------------------------------------------------------------------------- seg loss

VALID_SEG = [c for c in lo.SEG_CASES if c[6] in ("uniform", "drop_last", "one_class")]


@pytest.mark.parametrize("case", [c for c in VALID_SEG if c[1] * c[2] <= 20000], ids=lo.seg_id)
def test_nnu_oracle_vs_ref_cpu_autograd(case):
    """valid labels: value and gradient == float64 autograd of oracle/ref_cpu.nnu_loss"""
    d = lo.seg_inputs(case)
    ref = lo.seg_oracle(case)
    z = lo.T(d["logits"]).requires_grad_(True)
    total, ce, gdl = ref_cpu.nnu_loss(z, torch.from_numpy(np.array(d["labels"])), lo.T(d["w"]))
    total.backward()
    for k, v in (("total", total), ("ce", ce), ("gdl", gdl)):
        close(case[0] + " " + k, ref[k], v.detach())
    close(case[0] + " grad", ref["grad"], z.grad, ref["mag"])
    assert ref["n_bad"] == 0


@pytest.mark.parametrize("w_ce,w_dice", lo.SEG_PARAMS)
@pytest.mark.parametrize("smooth", lo.SEG_SMOOTH)
def test_nnu_oracle_weights_and_smooth_vs_autograd(w_ce, w_dice, smooth):
    """w_ce, w_dice and smooth against float64 autograd of the composition F.cross_entropy + Dice closed form"""
    case = lo.seg_case("C-5")
    d = lo.seg_inputs(case)
    ref = lo.seg_oracle(case, w_ce, w_dice, smooth)
    B, C, N = d["logits"].shape
    zv = lo.T(d["logits"]).permute(0, 2, 1).reshape(-1, C).requires_grad_(True)
    total, ce, gdl = lo.nnu_autograd(zv, torch.from_numpy(np.array(d["labels"])).reshape(-1), lo.T(d["w"]), w_ce, w_dice, smooth)
    total.backward()
    for k, v in (("total", total), ("ce", ce), ("gdl", gdl)):
        close(k, ref[k], v.detach())
    close("grad", ref["grad"], zv.grad.view(B, N, C).permute(0, 2, 1), ref["mag"])


@pytest.mark.parametrize("name", ["lab-bad5", "lab-cloud-bad", "lab-wrap32"])
def test_nnu_oracle_masks_invalid_points(name):
    """labels outside [0, C): the result is that of the valid points alone, the rows of the others are exactly zero"""
    case = lo.seg_case(name)
    d = lo.seg_inputs(case)
    ref = lo.seg_oracle(case)
    B, C, N = d["logits"].shape
    y = torch.from_numpy(np.array(d["labels"])).reshape(-1)
    valid = (y >= 0) & (y < C)
    assert ref["n_bad"] == int((~valid).sum()) > 0
    zv = lo.T(d["logits"]).permute(0, 2, 1).reshape(-1, C)[valid].requires_grad_(True)
    total, ce, gdl = lo.nnu_autograd(zv, y[valid], lo.T(d["w"]), 1.0, 1.0, 1.0)
    total.backward()
    for k, v in (("total", total), ("ce", ce), ("gdl", gdl)):
        close(k, ref[k], v.detach())
    rows = ref["grad"].permute(0, 2, 1).reshape(-1, C)
    mrows = ref["mag"].permute(0, 2, 1).reshape(-1, C)
    close("grad", rows[valid], zv.grad, mrows[valid])
    assert bool((rows[~valid] == 0).all()) and bool((mrows[~valid] == 0).all())
    if name == "lab-cloud-bad":
        assert not bool(valid.view(B, N)[1].any()) and bool(valid.view(B, N)[[0, 2]].all())
    elif name == "lab-wrap32":
        bad = y[~valid].numpy()
        assert set(bad) == set(lo.WRAP_LABELS) and len(bad) == B * (N // 10)
        assert ((bad & 0xFFFFFFFF) == 1).all(), "truncated to 32 bits these labels read as class 1"
    else:
        frac = float((~valid).double().mean())
        assert 0.03 <= frac <= 0.07
        assert set(np.unique(y[~valid].numpy())) == set(lo.BAD_LABELS(C))


def test_nnu_oracle_vs_reference_golden():
    """the figures of the real reference (fp32): value 1e-5, gradient 1e-5 of its largest element"""
    g = load("nnu_loss")
    for row in g["cases"]:
        seed, B, C, Np, wt = (int(v) for v in row)
        lg, lb, w = seg_loss_case(seed, B, C, Np, bool(wt), drop_class=(seed == 305))
        ref = lo.nnu(lo.T(lg), torch.from_numpy(lb), lo.T(w))
        for k in ("total", "ce", "gdl"):
            want = float(g["s%d_%s" % (seed, k)])
            assert abs(float(ref[k]) - want) <= 1e-5 * max(abs(want), 1e-3), (seed, k)
        gr = g["s%d_grad" % seed]
        assert np.abs(ref["grad"].numpy() - gr).max() <= 1e-5 * np.abs(gr).max(), seed


def test_nnu_oracle_fp32_run_is_a_yardstick():
    """the same statement in float32 lands within 1e-5 of the float64 one (relative to mag): it measures the number format"""
    case = lo.seg_case("C-9")
    r64, r32 = lo.seg_oracle(case), lo.seg_oracle(case, dtype=torch.float32)
    assert r32["grad"].dtype == torch.float32
    fig = float(((r32["grad"].double() - r64["grad"]).abs() / r64["mag"]).max())
    assert 0 < fig <= 1e-5, fig


@pytest.mark.parametrize("case", lo.SEG_CASES, ids=lo.seg_id)
def test_seg_case_inputs_are_what_they_claim(case):
    name, B, N, C, weighted, lg, lab, _ = case
    d = lo.seg_inputs(case)
    assert d["logits"].shape == (B, C, N) and d["labels"].shape == (B, N) and (d["w"] is not None) == weighted
    y = d["labels"].reshape(-1)
    valid = y[(y >= 0) & (y < C)]
    present = set(np.unique(valid))
    if lab == "one_class":
        assert present == {1}
    elif lab == "drop_last":
        assert present == set(range(C - 1))
    elif B * N >= C:
        assert present == set(range(C)), "every class needs a point"
    if lab in ("uniform", "drop_last", "one_class"):
        assert len(valid) == B * N
    if lg[0] == "offset":
        assert d["logits"].min() > lg[2] - 20 and lg[2] == 1e4
    if lg == ("scale", 40.0):                # exp underflows in fp32 for most classes of most points: z - max < -104
        z = d["logits"].astype(np.float64)
        assert ((z - z.max(1, keepdims=True)) < -104).mean() > 0.05


def test_seg_case_table_names_every_listed_case():
    pts = {(c[1], c[2]) for c in lo.SEG_GRID}
    assert pts == {(1, 1), (1, 255), (1, 256), (1, 257), (3, 5462), (7, 7033)}
    assert 3 * 5462 == 64 * 256 + 2
    assert [c[3] for c in lo.SEG_CLASSES] == [2, 4, 5, 8, 9, 10, 16, 17, 20, 21, 32]
    assert all((c[1], c[2]) == (2, 130) for c in lo.SEG_CLASSES)
    assert any(not c[4] for c in lo.SEG_GRID if (c[1], c[2]) == (3, 5462))


# --------------------------------------------------------------------------------------------------------------------- Chamfer

def _near_tie_free(x, y, gap=1e-9):
    d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    t = d.topk(2, dim=2, largest=False).values if y.shape[1] > 1 else None
    return t is None or bool(((t[..., 1] - t[..., 0]) > gap).all())


@pytest.mark.parametrize("N,M", [(700, 450), (1, 1), (257, 1), (512, 12), (12, 512)])
def test_chamfer_bwd_oracle_vs_autograd(N, M):
    """inputs without near-ties: the closed form from the float64 arg-min == float64 autograd of the nearest-neighbour distances
    under a random incoming gradient, and (g constant 1 / (B N)) of one direction of oracle/ref_cpu.chamfer"""
    rng = np.random.default_rng(N * 31 + M)
    B = 3
    x = torch.from_numpy(rng.uniform(-1, 1, (B, N, 3))).requires_grad_(True)
    y = torch.from_numpy(rng.uniform(-1, 1, (B, M, 3))).requires_grad_(True)
    assert _near_tie_free(x.detach(), y.detach())
    g = torch.from_numpy(rng.standard_normal((B, N)) * np.array(lo.CH_G_SCALE)[:, None])
    g[torch.from_numpy(rng.random((B, N)) < 0.1)] = 0.0
    d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    dist, arg = d.min(2)
    dist.backward(g)
    ref = lo.chamfer_bwd(x.detach(), y.detach(), arg, g)
    close("grad_x", ref["grad_x"], x.grad, ref["mag_x"])
    close("grad_y", ref["grad_y"], y.grad, ref["mag_y"])
    assert bool((ref["grad_x"][g == 0] == 0).all())
    # both directions with the constant gradients of the mean == ref_cpu.chamfer
    x2, y2 = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    ref_cpu.chamfer(x2, y2).backward()
    arg_y = d.detach().min(1).indices
    fwd = lo.chamfer_bwd(x.detach(), y.detach(), arg, torch.full((B, N), 1.0 / (B * N), dtype=torch.float64))
    back = lo.chamfer_bwd(y.detach(), x.detach(), arg_y, torch.full((B, M), 1.0 / (B * M), dtype=torch.float64))
    close("chamfer grad_x", fwd["grad_x"] + back["grad_y"], x2.grad, fwd["mag_x"] + back["mag_y"])
    close("chamfer grad_y", fwd["grad_y"] + back["grad_x"], y2.grad, fwd["mag_y"] + back["mag_x"])


def test_chamfer_tie_inputs_hold_exactly_the_intended_duplicates():
    d = lo.tie_inputs()
    for b in range(lo.TIE_B):
        assert lo.duplicate_groups(d["y"][b]) == sorted(lo.TIE_GROUPS)
        for k, grp in enumerate(lo.TIE_GROUPS):
            q = d["x"][b, lo.TIE_Q * k:lo.TIE_Q * (k + 1)]
            assert (q == d["y"][b, grp[0]]).all()
    # the groups sit where the table says: wave slice = (j % 1024) // 128, tile = j // 1024
    where = [[(j // 1024, (j % 1024) // 128) for j in grp] for grp in lo.TIE_GROUPS]
    assert where == [[(0, 0), (0, 1)], [(0, 7), (1, 0)], [(0, 0), (1, 0)], [(0, 0), (0, 3), (2, 0)]]
    lat = lo.lattice_inputs()
    assert (lat["x"] * 4 == np.round(lat["x"] * 4)).all() and (lat["y"] * 4 == np.round(lat["y"] * 4)).all()
    dist = ((lat["x"][0][:, None].astype(np.float64) - lat["y"][0][None].astype(np.float64)) ** 2).sum(-1)
    tied = (dist == dist.min(1, keepdims=True)).sum(1)
    assert (tied >= 2).mean() > 0.5, "most queries of the lattice must have several exactly nearest targets"


@pytest.mark.parametrize("case", lo.CH_BWD, ids=lo.ch_bwd_id)
def test_chamfer_bwd_inputs_are_what_they_claim(case):
    N, M, dup, _ = case
    d = lo.ch_bwd_inputs(case)
    g = d["g"]
    assert g.shape == (lo.CH_BWD_B, N)
    if N >= 257:
        assert 0.05 <= (g == 0).mean() <= 0.15 and (g > 0).any() and (g < 0).any()
        scale = np.abs(g).max(1)
        assert scale[1] < 1e-2 < 1.0 < scale[0] < 10.0 < scale[2]
    for b in range(lo.CH_BWD_B):
        assert lo.duplicate_groups(d["y"][b]) == ([dup] if dup else [])
    if dup:               # the duplicated point is the nearest target of its four queries (by a wide margin), whose g is not 0
        q = lo.T(d["x"])[:, lo.CH_DUP_Q]
        dist = ((q[:, :, None, :] - lo.T(d["y"])[:, None, :, :]) ** 2).sum(-1)
        near = dist.clone()
        near[:, :, list(dup)] = float("inf")
        assert bool((dist[:, :, dup[0]] < 1e-4).all()) and bool((near.min(2).values > 4 * dist[:, :, dup[0]]).all())
        assert (g[:, lo.CH_DUP_Q] != 0).all()


def test_chamfer_case_tables_name_every_listed_case():
    fwd = {(c[1], c[2]) for c in lo.CH_FWD}
    assert {(n, m) for n in lo.CH_QUERY_N for m in (129, 1025)} <= fwd
    assert {(129, m) for m in lo.CH_TARGET_M} <= fwd
    assert sorted(c[0] for c in lo.CH_FWD).count(2) >= len(lo.CH_FWD) // 2 - 1
    assert [c[:2] for c in lo.CH_BWD] == [(700, 450), (1, 1), (257, 1), (4096, 3), (4096, 12), (12, 4096), (300, 9000), (300, 16400)]
    assert sum(c[2] is not None for c in lo.CH_BWD) == 2


# --------------------------------------------------------------------------------------------------------------------- Adam

@pytest.mark.parametrize("wd", lo.ADAM_WD)
@pytest.mark.parametrize("n", [3, 1023, 4100])
def test_adam_oracle_vs_torch_adam_fp64(n, wd):
    """p, exp_avg and exp_avg_sq after every step == torch.optim.Adam on a float64 parameter, 1e-12 relative"""
    d = lo.adam_inputs(n)
    hp = lo.ADAM_HP
    ref = lo.adam_oracle(n, wd)
    p = torch.nn.Parameter(lo.T(d["p"]))
    opt = torch.optim.Adam([p], lr=lo.f32(lo.ADAM_LR[0]), betas=(lo.f32(hp["b1"]), lo.f32(hp["b2"])), eps=lo.f32(hp["eps"]),
                           weight_decay=lo.f32(wd))
    for s in range(lo.ADAM_STEPS):
        opt.param_groups[0]["lr"] = lo.f32(lo.ADAM_LR[s])
        p.grad = lo.T(d["g"][s])
        opt.step()
        st = opt.state[p]
        close("p step %d" % s, ref[s]["p"], p.detach(), ref[s]["mag_p"])
        close("m step %d" % s, ref[s]["m"], st["exp_avg"], ref[s]["mag_m"])
        close("v step %d" % s, ref[s]["v"], st["exp_avg_sq"], ref[s]["mag_v"])
        assert float(st["step"]) == s + 1


def test_adam_oracle_step_offset_and_fp32_run():
    """t0 shifts the bias corrections (the ticket test applies ONE step at t = 1, 2, 3); the float32 run is a float32 tensor"""
    n = 8
    d = lo.adam_inputs(n)
    one = lo.adam(lo.T(d["p"]), [lo.T(d["g"][0])], [1e-2], wd=0.0, t0=2, **lo.ADAM_HP)[0]
    b1, b2, eps = (lo.f32(lo.ADAM_HP[k]) for k in ("b1", "b2", "eps"))
    g = lo.T(d["g"][0])
    m, v = (1 - b1) * g, (1 - b2) * g * g
    want = lo.T(d["p"]) - lo.f32(1e-2) / (1 - b1 ** 3) * m / (v.sqrt() / (1 - b2 ** 3) ** 0.5 + eps)
    close("t = 3", one["p"], want, one["mag_p"])
    r32 = lo.adam_oracle(1023, 1e-2, dtype=torch.float32)
    assert r32[-1]["p"].dtype == torch.float32
    r64 = lo.adam_oracle(1023, 1e-2)
    assert float(((r32[-1]["p"].double() - r64[-1]["p"]).abs() / r64[-1]["mag_p"]).max()) <= 1e-5


@pytest.mark.parametrize("n", [n for n in lo.ADAM_FLAT_N + lo.ADAM_TICKET_N if n >= lo.ADAM_BLOCK_MIN_N])
def test_adam_fixtures_hold_the_blocks_they_claim(n):
    d = lo.adam_inputs(n)
    b = lo.adam_blocks(n)
    assert n // 8 >= 100
    for s, g in enumerate(d["g"]):
        assert (g[b["zero"]] == 0).all()
        t = np.abs(g[b["tiny"]].astype(np.float64))
        assert (t >= 0.4 * lo.ADAM_TINY_G).all() and (t <= 2.1 * lo.ADAM_TINY_G).all()
        # v of such an element is below fp32's normal range: (1 - b2) g^2 <= 1e-3 x 4.5e-40
        assert ((1 - 0.999) * t ** 2 < lo.TINY32).all()
        assert (np.abs(g[b["huge"]]) == lo.ADAM_HUGE_G).all() and (g[b["huge"]] > 0).any() and (g[b["huge"]] < 0).any()
        assert (g[b["late_zero"]] == 0).all() == (s >= 2)
        rest = g[4 * (n // 8):]
        assert (rest != 0).all() and 0.5 * (0.1 + s) < rest.std() < 2 * (0.1 + s)


def test_adam_case_tables_name_every_listed_case():
    assert lo.ADAM_FLAT_N == [1, 2, 3, 4, 5, 1023, 1049779]
    n4 = lo.ADAM_BIG >> 2
    assert n4 == 1024 * 256 + 300 and lo.ADAM_BIG & 3 == 3          # 1024 workgroups (the cap), 300 float4 left over, tail of 3
    sizes = [int(np.prod(s)) for s in lo.ADAM_SEG_SHAPES]
    n = sum(sizes)
    assert n > 900000 and all(s % 4 == 0 for s in sizes)
    per = -(-(n >> 2) // (lo.ADAM_MAX_CHUNKS - len(sizes)))           # csrc/adam.hip: chunks of at most `per` float4
    assert per > 1024, "a chunk must be longer than the 1024 threads of its workgroup"
    assert (sizes[0] >> 2) % per != 0 and 0 < (sizes[0] >> 2) % per < per      # the last chunk of the first parameter is short
    assert [min(1024, max(1, ((k >> 2) + 255) // 256)) for k in lo.ADAM_TICKET_N] == [1024, 1, 5]
