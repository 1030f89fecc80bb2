"""CPU tests of tests/bn_oracle.py, the float64 reference of the BatchNorm-fused stages: its closed forms against float64 autograd
over torch.nn.BatchNorm1d (every listed case with more than one row), the one-row training contract written out by hand, the
pins on the generated inputs that tests/test_bn_family_gpu.py relies on (no activation argument within KINK_MARGIN of 0, every
selection of a max above 4 x SEL_NOISE x mag, the ties where the tie test says they are), and the host-side argument checks
of fsg_bn_act_*, fsg_bn_act_max_* and fsg_bn_rows_* (nothing is launched)."""
import numpy as np
import pytest
import torch

import bn_oracle as bo
import pw_oracle as po

RTOL = 1e-12


def close(name, got, want, mag=None):
    """|got - want| <= 1e-12 x mag element by element (mag: the sum of absolute summands of that element, |want| when none is given);
    an element without summands must be equal"""
    mag = want.abs() if mag is None else mag.expand_as(want)
    err = float(((got - want).abs() / mag.clamp_min(1e-300)).max()) if want.numel() else 0.0
    assert err <= RTOL, (name, err)


def module64(d, C, training):
    bn = torch.nn.BatchNorm1d(C, eps=bo.EPS, momentum=bo.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(bo.T64(d["gamma"])); bn.bias.copy_(bo.T64(d["beta"]))
        bn.running_mean.copy_(bo.T64(d["rm"])); bn.running_var.copy_(bo.T64(d["rv"]))
    return bn.train(training)


def check_vs_autograd(ref, out, leaves, bn, zero_channel_dgamma=True):
    """closed forms == autograd, every element relative to the sum of the absolute summands of that element"""
    mag = ref["mag"]
    close("out", out.detach(), ref["out"], mag["out"])
    close("dy", leaves[0].grad, ref["dy"], mag["dy"])
    keep = torch.ones_like(ref["dgamma"], dtype=torch.bool)
    if not zero_channel_dgamma:
        keep[bo.ZERO_GAMMA] = False
    close("dgamma", bn.weight.grad[keep], ref["dgamma"][keep], mag["dgamma"][keep])
    close("dbeta", bn.bias.grad, ref["dbeta"], mag["dbeta"])
    if len(leaves) > 1:
        assert torch.equal(leaves[1].grad, ref["dres"])
    if bn.running_mean is not None:
        close("running_mean", bn.running_mean, ref["running_mean"])
        close("running_var", bn.running_var, ref["running_var"])
        assert int(bn.num_batches_tracked) == ref["num_batches_tracked"]


@pytest.mark.parametrize("case", [c for c in bo.CASES_ACT if c[0] > 1], ids=bo.case_id)
def test_bn_act_oracle_vs_autograd(case):
    M, C, training, slope, _ = case
    d = bo.act_inputs(case)
    ref = bo.act_oracle(case)
    bn = module64(d, C, training)
    y = bo.T64(d["y"]).requires_grad_(True)
    out = torch.nn.functional.leaky_relu(bn(y), slope)
    out.backward(bo.T64(d["g"]))
    check_vs_autograd(ref, out, [y], bn)
    if training:
        close("mean", ref["mean"], y.detach().mean(0))
        close("invstd", ref["invstd"], 1.0 / torch.sqrt(y.detach().var(0, unbiased=False) + bo.EPS))


@pytest.mark.parametrize("case", [c for c in bo.CASES_MAX if c[0] * c[1] > 1], ids=bo.case_id)
def test_bn_act_max_oracle_vs_autograd(case):
    """the gamma == 0 channel ties in every row: autograd may route its gradient to any of them, so dgamma of that channel is
    compared with the row the oracle names (the highest y of the cloud) instead"""
    B, N, C, training, _ = case
    d = bo.max_inputs(case)
    ref = bo.max_oracle(case)
    bn = module64(d, C, training)
    y = bo.T64(d["y"]).requires_grad_(True)
    act = torch.nn.functional.leaky_relu(bn(y.view(B * N, C)), bo.MAX_SLOPE).view(B, N, C)
    out = act.max(dim=1)[0]
    out.backward(bo.T64(d["g"]))
    check_vs_autograd(ref, out, [y], bn, zero_channel_dgamma=False)
    z = bo.ZERO_GAMMA
    yz = bo.T64(d["y"])[:, :, z]
    assert torch.equal(ref["arg"][:, z], po.argmax_lowest(yz, 1))
    h = bo.T64(d["g"])[:, z] * po.dlrelu(bo.T64(d["beta"])[z].expand(B), bo.MAX_SLOPE)
    yhat = (yz.gather(1, ref["arg"][:, z][:, None]).squeeze(1) - ref["mean"][z]) * ref["invstd"][z]
    close("dgamma of the gamma == 0 channel", ref["dgamma"][z], (h * yhat).sum(), ref["mag"]["dgamma"][z])
    keep = torch.ones(C, dtype=torch.bool)
    keep[z] = False
    assert torch.equal(ref["arg"][:, keep], act.detach().argmax(1)[:, keep])


@pytest.mark.parametrize("case", [c for c in bo.CASES_ROWS if c[0] > 1], ids=bo.case_id)
def test_bn_rows_oracle_vs_autograd(case):
    M, C, training, relu, has_res, _ = case
    d = bo.rows_inputs(case)
    ref = bo.rows_oracle(case)
    bn = module64(d, C, training)
    x = bo.T64(d["x"]).requires_grad_(True)
    leaves = [x]
    z = bn(x)
    if has_res:
        leaves.append(bo.T64(d["res"]).requires_grad_(True))
        z = z + leaves[1]
    out = torch.relu(z) if relu else z
    out.backward(bo.T64(d["g"]))
    check_vs_autograd(ref, out, leaves, bn)


@pytest.mark.parametrize("training", [True, False])
def test_bn_act_maxavg_oracle_vs_autograd(training):
    """the [max | mean] stage, which the module-semantics test of the GPU suite judges with this oracle"""
    B, N, C = 3, 70, 64
    rng = np.random.default_rng(5)
    y, gamma, beta = bo.channels("max", B * N, C, rng)
    rm, rv = bo.running_buffers(y, C, training, rng)
    y, _ = bo.settle(y, gamma, beta, training, rm, rv, N=N)
    d = dict(gamma=gamma, beta=beta, rm=rm, rv=rv)
    g = torch.from_numpy(rng.standard_normal((B, 2 * C)))
    ref = bo.bn_act_maxavg(bo.T64(y).view(B, N, C), bo.T64(gamma), bo.T64(beta), g, training, 0.2, bo.T64(rm), bo.T64(rv))
    bn = module64(d, C, training)
    yt = bo.T64(y).view(B, N, C).requires_grad_(True)
    act = torch.nn.functional.leaky_relu(bn(yt.view(B * N, C)), 0.2).view(B, N, C)
    out = torch.cat((act.max(dim=1)[0], act.mean(dim=1)), 1)
    out.backward(g)
    # (the gamma == 0 channel: its activation is the same in every row, the max routes g_max to any of them, yhat differs)
    check_vs_autograd(ref, out, [yt], bn, zero_channel_dgamma=False)


def test_one_row_training_contract():
    """M = 1 in training, where torch has no answer: mean = y, variance 0, invstd = 1 / sqrt(eps), out = f(beta); the running
    mean moves towards y and the running variance towards the BIASED value 0; dbeta = h, dgamma = 0, dy = a (h - h - 0) = 0"""
    for stage, case in (("act", bo.CASES_ACT[0]), ("max", bo.CASES_MAX[0]), ("rows", bo.CASES_ROWS[0])):
        if stage == "act":
            d, ref, slope = bo.act_inputs(case), bo.act_oracle(case), case[3]
            y, g = bo.T64(d["y"]), bo.T64(d["g"])
        elif stage == "max":
            d, ref, slope = bo.max_inputs(case), bo.max_oracle(case), bo.MAX_SLOPE
            y, g = bo.T64(d["y"])[0], bo.T64(d["g"])
            assert int(ref["arg"].abs().max()) == 0
        else:
            d, ref, slope = bo.rows_inputs(case), bo.rows_oracle(case), 0.0
            y, g = bo.T64(d["x"]), bo.T64(d["g"])
        assert y.shape[0] == 1
        gamma, beta, rm, rv = (bo.T64(d[k]) for k in ("gamma", "beta", "rm", "rv"))
        assert torch.equal(ref["mean"], y[0]) and torch.equal(ref["var"], torch.zeros_like(y[0]))
        close(stage + " invstd", ref["invstd"], torch.full_like(y[0], bo.EPS ** -0.5))
        close(stage + " out", ref["out"].reshape(-1), torch.where(beta > 0, beta, beta * slope))
        close(stage + " running_mean", ref["running_mean"], 0.9 * rm + 0.1 * y[0])
        close(stage + " running_var", ref["running_var"], 0.9 * rv)
        h = (g * po.dlrelu(beta, slope)).reshape(-1)
        close(stage + " dbeta", ref["dbeta"], h)
        assert torch.equal(ref["dgamma"], torch.zeros_like(h)) and bool((ref["dy"] == 0).all())
        assert ref["num_batches_tracked"] == 1


def test_cumulative_average_and_untracked_statistics():
    """momentum None is the cumulative average 1 / num_batches_tracked, as torch.nn.BatchNorm1d(momentum=None) applies it over
    two calls; without running buffers the batch statistics are used in both modes and nothing is updated"""
    rng = np.random.default_rng(3)
    ys = [torch.from_numpy(rng.standard_normal((37, 64)) * 2 + 1) for _ in range(2)]
    gamma, beta, g = (torch.from_numpy(rng.standard_normal(s)) for s in ((64,), (64,), (37, 64)))
    bn = torch.nn.BatchNorm1d(64, momentum=None).double()
    rm, rv, tracked = bn.running_mean.clone(), bn.running_var.clone(), 0
    for y in ys:
        bn(y)
        ref = bo.bn_act(y, gamma, beta, g, True, 0.2, rm, rv, momentum=None, tracked=tracked)
        rm, rv, tracked = ref["running_mean"], ref["running_var"], ref["num_batches_tracked"]
    close("running_mean", rm, bn.running_mean)
    close("running_var", rv, bn.running_var)
    assert tracked == int(bn.num_batches_tracked) == 2
    ref = bo.bn_act(ys[0], gamma, beta, g, True, 0.2, None, None)
    assert ref["running_mean"] is None and ref["running_var"] is None and ref["num_batches_tracked"] == 0


# --------------------------------------------------------------------------------------------------------------------- input pins

def _all_cases():
    return [("act", c) for c in bo.CASES_ACT] + [("max", c) for c in bo.CASES_MAX] + [("rows", c) for c in bo.CASES_ROWS]


@pytest.mark.parametrize("stage,case", _all_cases(), ids=lambda v: v if isinstance(v, str) else bo.case_id(v))
def test_case_inputs_are_off_the_kinks_and_above_the_selection_noise(stage, case):
    """what the GPU tests rely on to leave nothing out: zero elements inside the kink margin, zero selections under the margin"""
    if stage == "act":
        d, training = bo.act_inputs(case), case[2]
        n_kink = bo.kinks(d["y"], d["gamma"], d["beta"], training, d["rm"], d["rv"])
    elif stage == "rows":
        d, training = bo.rows_inputs(case), case[2]
        n_kink = bo.kinks(d["x"], d["gamma"], d["beta"], training, d["rm"], d["rv"], d["res"])
    else:
        d, training = bo.max_inputs(case), case[3]
        C = d["gamma"].size
        n_kink = bo.kinks(d["y"].reshape(-1, C), d["gamma"], d["beta"], training, d["rm"], d["rv"])
        gap, need = bo.max_margins(bo.max_oracle(case), d["gamma"])
        keep = torch.ones(C, dtype=torch.bool)
        keep[bo.ZERO_GAMMA] = False
        n_short = int((gap[:, keep] <= need[:, keep]).sum())
        print("BNCASE max %s sub-margin selections %d of %d" % (bo.case_id(case), n_short, gap[:, keep].numel()))
        assert n_short == 0
    print("BNCASE %s %s kink elements %d" % (stage, bo.case_id(case), n_kink))
    assert n_kink == 0
    # the channel mix is what the docstring of channels() says
    gamma = d["gamma"]
    assert gamma[bo.ZERO_GAMMA] == 0 and int((gamma == 0).sum()) == 1
    assert bool((gamma[::4] < 0).all()) and int((gamma < 0).sum()) == gamma.size // 4
    first = (d["x"] if stage == "rows" else d["y"]).reshape(-1, gamma.size)
    const = np.array([bo.channel_kind(c) == bo.CONSTANT_KIND for c in range(gamma.size)])
    if stage != "max":
        assert bool((first[:, const] == first[:1, const]).all())
    if first.shape[0] > 100:
        sd = first.astype(np.float64).std(0)
        assert bool((sd[~const] > 0).all()) and (stage == "max" or bool((sd[const] == 0).all()))


def test_tie_inputs_have_the_ties_where_they_belong():
    d = bo.tie_inputs()
    y, gamma = torch.from_numpy(np.array(d["y"])).double(), d["gamma"]
    assert y.shape == (bo.TIE_B, bo.TIE_N, bo.TIE_C) and bool((gamma != 0).all())
    for c in range(bo.TIE_C):
        lo, hi = bo.TIE_PAIRS[c % 5]
        v = y[:, :, c] * (1.0 if gamma[c] >= 0 else -1.0)
        top = v.max(1)[0]
        assert bool((top == bo.TIE_VALUE).all())
        tied = (v == top[:, None]).nonzero()
        assert tied[:, 1].view(bo.TIE_B, 2).tolist() == [[lo, hi]] * bo.TIE_B
    pairs = bo.TIE_PAIRS
    assert pairs[0][1] - pairs[0][0] == 4 and pairs[0][0] // 128 == pairs[0][1] // 128        # one wave of one tile
    assert pairs[1][0] % 4 < pairs[1][1] % 4 and pairs[2][0] % 4 > pairs[2][1] % 4           # two waves, both orders
    assert pairs[3][0] // 128 != pairs[3][1] // 128 and pairs[4][1] - pairs[4][0] == 128      # two tiles
    ref = bo.bn_act_max(y, bo.T64(gamma), bo.T64(d["beta"]), bo.T64(d["g"]), False, bo.MAX_SLOPE, bo.T64(d["rm"]), bo.T64(d["rv"]))
    assert ref["arg"].tolist() == [[bo.TIE_PAIRS[c % 5][0] for c in range(bo.TIE_C)]] * bo.TIE_B


# --------------------------------------------------------------------------------------------------------------------- entry points

def test_bn_entry_points_reject_bad_arguments():
    """host-side checks, before any launch: NULL pointers, C outside the envelope, M / B / N <= 0, a training forward without
    its workspace, and more records than one grid dimension holds (ceil(M / 128) or B ceil(N / 128) above 65535)"""
    from fissure_segmentation_amd import _lib
    p = 64                                                  # never dereferenced: the checks fail first

    def act_fwd(y=p, ws=p, M=16, C=64, training=1):
        return _lib.call("fsg_bn_act_fwd_f32", y, p, p, p, p, M, C, training, 0.1, 1e-5, 0.2, p, p, p, ws, None)

    def act_bwd(g=p, ws=p, M=16, C=64):
        return _lib.call("fsg_bn_act_bwd_f32", g, p, p, p, p, p, M, C, 1, 0.2, p, p, p, ws, None)

    def max_fwd(y=p, ws=p, B=2, N=16, C=64, training=1):
        return _lib.call("fsg_bn_act_max_fwd_f32", y, p, p, p, p, B, N, C, training, 0.1, 1e-5, 0.2, p, p, p, p, p, ws, None)

    def max_bwd(g=p, arg=p, B=2, N=16, C=64):
        return _lib.call("fsg_bn_act_max_bwd_f32", g, p, p, arg, p, p, p, p, B, N, C, 1, 0.2, p, p, p, None)

    def rows_fwd(x=p, ws=p, M=16, C=64, training=1):
        return _lib.call("fsg_bn_rows_fwd_f32", x, None, p, p, p, p, M, C, training, 0.1, 1e-5, 1, p, p, p, ws, None)

    def rows_bwd(g=p, ws=p, out=p, M=16, C=64, relu=1):
        return _lib.call("fsg_bn_rows_bwd_f32", g, p, out, p, p, p, M, C, 1, relu, p, None, p, p, ws, None)

    for fn in (act_fwd, act_bwd, max_fwd, max_bwd, rows_fwd, rows_bwd):
        with pytest.raises(RuntimeError, match="NULL pointer"):
            fn(None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        max_bwd(arg=None)
    with pytest.raises(RuntimeError, match="NULL pointer"):   # the backward passes and the max always need their scratch
        act_bwd(ws=None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        max_fwd(ws=None, training=0)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        rows_bwd(ws=None)
    with pytest.raises(RuntimeError, match="needs the forward output"):
        rows_bwd(out=None)
    for fn in (act_fwd, rows_fwd):
        with pytest.raises(RuntimeError, match="training needs the workspace"):
            fn(ws=None)
    for fn in (act_fwd, act_bwd):
        for M, C in [(16, 96), (16, 0), (0, 64), (-1, 64), (128 * 65536, 64), (128 * 65535 + 1, 64), (2 ** 39, 64)]:
            with pytest.raises(RuntimeError, match="bad shape"):
                fn(M=M, C=C)
    for fn in (max_fwd, max_bwd):
        for B, N, C in [(2, 16, 96), (0, 16, 64), (2, 0, 64), (2, 16, 0), (-2, 16, 64), (70000, 1, 64), (2, 128 * 32768, 64)]:
            with pytest.raises(RuntimeError, match="bad shape"):
                fn(B=B, N=N, C=C)
    for fn in (rows_fwd, rows_bwd):
        for M, C in [(16, 96), (16, 48), (16, 1024), (16, 0), (0, 64), (-3, 64)]:
            with pytest.raises(RuntimeError, match="bad shape"):
                fn(M=M, C=C)
    assert _lib.lib.fsg_bn_rows_workspace_bytes(16, 96) == 0
