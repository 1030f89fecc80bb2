"""Plain float64 statements of the BatchNorm-fused stages (csrc/bn_act.hip: fsg_bn_act_*, fsg_bn_act_max_*; csrc/bn_rows.hip:
fsg_bn_rows_*), written from their contracts in include/fsg_hip.h: torch ops on the CPU, closed forms, no autograd and no
kernels.  tests/test_bn_oracle_cpu.py compares them with float64 autograd over torch.nn.BatchNorm1d, which is what makes them
a reference, and pins the generated inputs; tests/test_bn_family_gpu.py compares the kernels with them.

The contract every function states (a = gamma invstd, yhat = (y - mean) invstd, u = a (y - mean) + beta, M rows per channel):
  training: mean / var are the batch statistics, var BIASED (divided by M) in the normalisation and UNBIASED (M - 1) in the
    running update  running = (1 - momentum) running + momentum batch.  With M = 1 the running update takes the biased value (0):
    that is what bn_finalize_kernel and bnr_finalize_kernel both do; torch refuses M = 1 in training, so this file is the only
    reference there.  Without running buffers (track_running_stats=False) nothing is updated.
  eval: mean / var are the running statistics, which stay as they are.
  backward: h = g f'(u);  dbeta = sum h;  dgamma = sum h yhat;  dy = a (h - dbeta / M - yhat dgamma / M) with batch statistics,
    dy = a h with running statistics.
  max: the row of a (cloud, channel) is the one with the largest sgn y, sgn = -1 for gamma < 0 and +1 otherwise (f(BN(.)) is
    monotone in y), the lowest row among equal values; h is non-zero on that row only.

Every value comes with `mag`, the sum of the absolute summands it is made of, so that one relative bar |got - fp64| / mag holds
for well- and ill-conditioned channels:  pre-activation |a y| + |a mean| + |beta| (+ |residual|);  dbeta sum |h|;  dgamma
sum |h yhat|;  dy |a| (|h| + |dbeta| / M + |yhat| |dgamma| / M);  mean sum |y| / M.  invstd and the running statistics are
measured relative to their float64 value.
"""
import zlib

import numpy as np
import torch

from pw_oracle import KINK_MARGIN, SEL_NOISE, argmax_lowest, away_from_kink, dlrelu, kink_count, lrelu

EPS, MOMENTUM, MAX_SLOPE = 1e-5, 0.1, 0.2
ZERO_GAMMA = 7          # the channel with gamma == 0


# --------------------------------------------------------------------------------------------------------------------- closed forms

def batch_stats(y, training, rm=None, rv=None, eps=EPS, momentum=MOMENTUM, tracked=0):
    """y (M, C) float64 -> dict(mean, var, invstd, running_mean, running_var, num_batches_tracked) under the contract above.
    training with rm / rv None: batch statistics, no update.  momentum None: the cumulative average 1 / (tracked + 1)."""
    counted = tracked + 1 if (training and rm is not None) else tracked
    if momentum is None:
        momentum = 1.0 / max(counted, 1)
    M = y.shape[0]
    if training:
        mean = y.mean(0)
        var = (y - mean).pow(2).mean(0)
        new_rm, new_rv = rm, rv
        if rm is not None:
            unbiased = var * M / (M - 1) if M > 1 else var
            new_rm, new_rv = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unbiased
    else:
        mean, var, new_rm, new_rv = rm, rv, rm.clone(), rv.clone()
    return dict(mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps), running_mean=new_rm, running_var=new_rv,
                num_batches_tracked=counted)


def _backward(out, h, hmag, yhat, a, M, batch):
    """dbeta, dgamma, dy and their mags from h (rows, C) [and |h|], added to `out`"""
    dbeta, dgamma = h.sum(0), (h * yhat).sum(0)
    dy = a * (h - dbeta / M - yhat * dgamma / M) if batch else a * h
    mag = out["mag"]
    mag["dbeta"], mag["dgamma"] = hmag.sum(0), (hmag * yhat.abs()).sum(0)
    mag["dy"] = a.abs() * (hmag + dbeta.abs() / M + yhat.abs() * dgamma.abs() / M) if batch else a.abs() * hmag
    out.update(dbeta=dbeta, dgamma=dgamma, dy=dy)


def bn_act(y, gamma, beta, g, training, slope, rm=None, rv=None, eps=EPS, momentum=MOMENTUM, tracked=0):
    """fsg_bn_act_{fwd,bwd}_f32: out = lrelu(BatchNorm(y)) on rows y (M, C), grad_out g (M, C)"""
    M = y.shape[0]
    out = batch_stats(y, training, rm, rv, eps, momentum, tracked)
    mean, r = out["mean"], out["invstd"]
    a, yhat = gamma * r, (y - mean) * r
    u = a * (y - mean) + beta
    out.update(u=u, out=lrelu(u, slope), mag=dict(out=(a * y).abs() + (a * mean).abs() + beta.abs(), mean=y.abs().mean(0)))
    h = g * dlrelu(u, slope)
    _backward(out, h, h.abs(), yhat, a, M, training)
    return out


def bn_act_max(y, gamma, beta, g, training, slope, rm=None, rv=None, eps=EPS, momentum=MOMENTUM, tracked=0):
    """fsg_bn_act_max_{fwd,bwd}_f32: out (B, C) = max over the N points of lrelu(BatchNorm(y)), y (B, N, C), grad_out g (B, C);
    `arg` (B, C) is the selected row of every (cloud, channel)"""
    B, N, C = y.shape
    M = B * N
    flat = y.reshape(M, C)
    out = batch_stats(flat, training, rm, rv, eps, momentum, tracked)
    mean, r = out["mean"], out["invstd"]
    a = gamma * r
    sgn = torch.where(gamma < 0, -1.0, 1.0).to(y.dtype)
    arg = argmax_lowest(y * sgn, 1)
    ysel = y.gather(1, arg[:, None]).squeeze(1)
    usel = a * (ysel - mean) + beta
    u = a * (y - mean) + beta
    out.update(arg=arg, ysel=ysel, u=u, out=lrelu(usel, slope),
               mag=dict(out=(a * ysel).abs() + (a * mean).abs() + beta.abs(), mean=flat.abs().mean(0),
                        u=(a * y).abs() + (a * mean).abs() + beta.abs()))
    hsel = g * dlrelu(usel, slope)
    h = torch.zeros_like(y).scatter_(1, arg[:, None], hsel[:, None])
    yhat = (flat - mean) * r
    _backward(out, h.reshape(M, C), h.abs().reshape(M, C), yhat, a, M, training)
    out["dy"], out["mag"]["dy"] = out["dy"].view(B, N, C), out["mag"]["dy"].view(B, N, C)
    return out


def bn_act_maxavg(y, gamma, beta, g, training, slope, rm=None, rv=None, eps=EPS, momentum=MOMENTUM, tracked=0):
    """fsg_bn_act_maxavg_{fwd,bwd}_f32: out (B, 2C) = [max | mean] over the N points of lrelu(BatchNorm(y)), y (B, N, C), grad_out
    g (B, 2C) = [g_max | g_avg]: the gradient reaching the BatchNorm output is h = f'(u) (g_max [n = arg] + g_avg / N)"""
    B, N, C = y.shape
    M = B * N
    flat = y.reshape(M, C)
    out = batch_stats(flat, training, rm, rv, eps, momentum, tracked)
    mean, r = out["mean"], out["invstd"]
    a = gamma * r
    sgn = torch.where(gamma < 0, -1.0, 1.0).to(y.dtype)
    arg = argmax_lowest(y * sgn, 1)
    u = a * (y - mean) + beta
    umag = (a * y).abs() + (a * mean).abs() + beta.abs()
    act = lrelu(u, slope)
    pick = lambda t: t.gather(1, arg[:, None]).squeeze(1)
    out.update(arg=arg, u=u, out=torch.cat((pick(act), act.mean(1)), 1),
               mag=dict(out=torch.cat((pick(umag), umag.mean(1)), 1), mean=flat.abs().mean(0), u=umag))
    gmax, gavg = g[:, None, :C], g[:, None, C:]
    sel = torch.zeros_like(y).scatter_(1, arg[:, None], 1.0)
    fp = dlrelu(u, slope)
    h, hmag = fp * (sel * gmax + gavg / N), fp.abs() * (sel * gmax.abs() + gavg.abs() / N)
    _backward(out, h.reshape(M, C), hmag.reshape(M, C), (flat - mean) * r, a, M, training)
    out["dy"], out["mag"]["dy"] = out["dy"].view(B, N, C), out["mag"]["dy"].view(B, N, C)
    return out


def bn_rows(x, res, gamma, beta, g, training, relu, rm=None, rv=None, eps=EPS, momentum=MOMENTUM, tracked=0):
    """fsg_bn_rows_{fwd,bwd}_f32: out = [relu](BatchNorm(x) [+ res]) on rows x (M, C); dres is the gradient of the residual"""
    M = x.shape[0]
    out = batch_stats(x, training, rm, rv, eps, momentum, tracked)
    mean, r = out["mean"], out["invstd"]
    a, xhat = gamma * r, (x - mean) * r
    z = a * (x - mean) + beta + (res if res is not None else 0.0)
    mag = (a * x).abs() + (a * mean).abs() + beta.abs() + (res.abs() if res is not None else 0.0)
    out.update(u=z, out=z.clamp_min(0) if relu else z, mag=dict(out=mag, mean=x.abs().mean(0), dres=g.abs()))
    h = g * (z > 0).to(g.dtype) if relu else g
    _backward(out, h, h.abs(), xhat, a, M, training)
    out["dres"] = h if res is not None else None
    return out


# --------------------------------------------------------------------------------------------------------------------- inputs
# channel kinds, c % 7 (gamma < 0 on every 4th channel: 7 and 4 are coprime, every kind meets both signs from C = 28 on):
#   (location, spread)
KINDS = [(0.0, 1.0),        # N(0, 1)
         (5.0, 0.05),       # N(5, 0.05^2): the case norm.py cites for MIOpen's loss
         (-50.0, 0.5),      # N(-50, 0.5^2)
         (0.0, 1e3),        # spread 1e3
         (0.0, 1e-3),       # spread 1e-3 around 0
         (None, 0.0),       # exactly constant (variance 0); the constant differs from channel to channel
         (1.0, 2.0)]        # N(1, 2^2), what the older tests draw
CONSTANT_KIND = 5


def channel_kind(c):
    return c % len(KINDS)


def nominal(C, rng):
    """(location, spread) of every channel; spread 0 for the constant ones"""
    loc = np.array([KINDS[channel_kind(c)][0] if KINDS[channel_kind(c)][0] is not None else 0.0 for c in range(C)])
    spread = np.array([KINDS[channel_kind(c)][1] for c in range(C)])
    const = rng.uniform(1.0, 4.0, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)
    loc = np.where(spread == 0.0, const, loc)
    return loc, spread


def channels(kind, M, C, rng):
    """float32 y (M, C), gamma (C,), beta (C,): the fixed mix of channel kinds above; gamma in +-[0.5, 1.5], negative on every 4th
    channel and exactly 0 on channel ZERO_GAMMA; |beta| in [0.1, 1.5] (the LeakyReLU argument of a constant or gamma == 0
    channel IS beta, which must stay off the kink).  kind 'act' / 'rows': all kinds; kind 'max': the constant kind is drawn
    as N(0, 1) instead (every row of a constant channel ties; test_bn_act_max_exact_ties_route_to_one_row and
    test_bn_constant_and_shifted_channels cover that)."""
    assert kind in ("act", "max", "rows")
    loc, spread = nominal(C, rng)
    if kind == "max":
        loc, spread = np.where(spread == 0.0, 0.0, loc), np.where(spread == 0.0, 1.0, spread)
    y = (loc + spread * rng.standard_normal((M, C))).astype(np.float32)
    y[:, spread == 0.0] = loc[spread == 0.0].astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C)
    gamma[::4] *= -1
    gamma[ZERO_GAMMA] = 0.0
    beta = rng.uniform(0.1, 1.5, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)
    return y, gamma.astype(np.float32), beta.astype(np.float32)


def running_buffers(y, C, training, rng):
    """float32 running_mean / running_var of a case.  Eval: near the channel's own statistics (location + 0.1 spread, spread^2 x
    [0.5, 1.5]; 1 x that for a constant channel), so that the normalised values are O(1) and the kinks in reach.  Training: the
    running mean has the sign of the batch mean and at least half the channel's scale, so that the update adds two terms of one
    sign and the relative error of the result means something."""
    y64 = y.astype(np.float64)
    mean, sd = y64.mean(0), y64.std(0)
    scale = np.where(sd > 0, sd, 1.0)
    if training:
        rm = np.where(mean < 0, -1.0, 1.0) * (np.abs(mean) + scale * rng.uniform(0.5, 1.5, C))
    else:
        rm = mean + 0.1 * scale * rng.standard_normal(C)
    rv = scale ** 2 * rng.uniform(0.5, 1.5, C)
    return rm.astype(np.float32), rv.astype(np.float32)


def _stats64(y, training, rm, rv):
    y64 = y.astype(np.float64)
    mean, var = (y64.mean(0), y64.var(0)) if training else (rm.astype(np.float64), rv.astype(np.float64))
    return mean, 1.0 / np.sqrt(var + EPS)


def settle(y, gamma, beta, training, rm, rv, N=0, res=None, movable=None):
    """the float32 rows y (M, C) [and res] of a case moved until, under the float64 statistics of the moved rows, no element's
    LeakyReLU / ReLU argument lies within KINK_MARGIN of 0 and (N > 0: clouds of N rows) every selection of a max beats its
    runner-up by more than 4 SEL_NOISE mag.  With a residual the residual is moved (the statistics stay).  Channels with
    gamma == 0 and columns outside `movable` are left alone.  Returns (y, res)."""
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    cols = g64 != 0
    if movable is not None:
        cols &= movable
    for _ in range(50):
        mean, r = _stats64(y, training, rm, rv)
        a = g64 * r
        delta = b64 - a * mean
        moved = False
        if res is not None:
            z = a * y.astype(np.float64) + delta + res.astype(np.float64)
            near = np.abs(z) < 2 * KINK_MARGIN
            if near.any():
                target = np.where(z >= 0, 3.0 * KINK_MARGIN, -3.0 * KINK_MARGIN)
                res = np.where(near, res.astype(np.float64) + target - z, res).astype(np.float32)
                z = a * y.astype(np.float64) + delta + res.astype(np.float64)
                assert not (np.abs(z) < KINK_MARGIN).any()
        elif cols.any() and kink_count(y[:, cols], a[cols], delta[cols], KINK_MARGIN) > 0:
            y = y.copy()
            y[:, cols] = away_from_kink(y[:, cols], a[cols], delta[cols], KINK_MARGIN)
            moved = True
        if N and N > 1 and not moved:
            B = y.shape[0] // N
            y64 = y.astype(np.float64)
            u = (a * y64 + delta).reshape(B, N, -1)
            mag = (np.abs(a * y64) + np.abs(a * mean) + np.abs(b64)).reshape(B, N, -1)
            order = np.argsort(u, axis=1)
            win, second = order[:, -1], order[:, -2]
            uw, us = np.take_along_axis(u, win[:, None], 1)[:, 0], np.take_along_axis(u, second[:, None], 1)[:, 0]
            need = 4 * SEL_NOISE * np.take_along_axis(mag, win[:, None], 1)[:, 0]
            short = (uw - us <= 2 * need) & cols[None]
            if short.any():
                y3 = y64.reshape(B, N, -1)
                bi, ci = np.nonzero(short)
                # the winner goes up by 4 x what it needs (its mag grows with it by far less than that)
                y3[bi, win[bi, ci], ci] += (4 * need[bi, ci] - (uw - us)[bi, ci]) / a[ci]
                y = y3.reshape(-1, y.shape[1]).astype(np.float32)
                moved = True
        if not moved:
            return y, res
    raise AssertionError("the inputs did not settle")


def kinks(y, gamma, beta, training, rm, rv, res=None):
    """number of elements whose activation argument lies within KINK_MARGIN of 0 (float64 statistics of y); the gamma == 0 and
    constant channels count too: their argument is beta"""
    mean, r = _stats64(y, training, rm, rv)
    a = gamma.astype(np.float64) * r
    z = a * (y.astype(np.float64) - mean) + beta.astype(np.float64) + (res.astype(np.float64) if res is not None else 0.0)
    return int((np.abs(z) < KINK_MARGIN).sum())


def max_margins(ref, gamma):
    """(gap, needed) per (cloud, channel) of a bn_act_max() result: top-2 gap of the pre-activation u along the points and
    4 SEL_NOISE mag of the winner; gap = inf for clouds of one point"""
    u, mag = ref["u"], ref["mag"]["u"]
    need = 4 * SEL_NOISE * mag.gather(1, u.argmax(1)[:, None]).squeeze(1)
    if u.shape[1] == 1:
        return torch.full_like(need, float("inf")), need
    t = u.topk(2, dim=1).values
    return t[:, 0] - t[:, 1], need


# --------------------------------------------------------------------------------------------------------------------- cases
# the smallest shapes that reach each code path.  (M, C, training, slope, reason)
CASES_ACT = [
    (1, 64, True, 0.2, "one row in total (torch refuses it; the running variance takes the biased value)"),
    (3, 64, True, 0.2, "waves that own no row"),
    (127, 64, True, 0.2, "one row short of the 128-row tile"),
    (128, 64, True, 0.2, "exactly one tile"),
    (129, 64, True, 0.2, "a one-row record to merge"),
    (130, 128, False, 0.2, "eval, two channel groups, ragged tile"),
    (300, 1024, True, 0.0, "ReLU, the widest layer of the head"),
    (257, 64, True, 1.0, "slope 1: BatchNorm only"),
    (32769, 64, True, 0.2, "257 records: second round of sum_partials_kernel"),
    (65665, 64, True, 0.2, "514 records: second round of bn_finalize_kernel; M C above the 16384 x 256 cap of the backward apply"),
    (16400, 576, True, 0.2, "C no power of two; M C / 4 above the 8192 x 256 cap of the forward apply: the grid-stride loop wraps"),
]
# (B, N, C, training, reason)
CASES_MAX = [
    (1, 1, 64, True, "one row in total"),
    (4, 1, 64, True, "clouds of one point: every point is its cloud's max"),
    (2, 3, 64, True, "waves that own no row"),
    (3, 129, 64, True, "a one-row tile per cloud"),
    (1, 128, 128, True, "one cloud, exactly one tile, two channel groups"),
    (2, 257, 64, False, "eval, three tiles per cloud"),
    (5, 130, 192, True, "C no power of two, ragged tile"),
    (129, 500, 64, True, "516 records: second round of bn_finalize_kernel"),
]
# (M, C, training, relu, res, reason)
CASES_ROWS = [
    (1, 32, True, True, False, "one row in total"),
    (2, 512, True, True, False, "the widest layer, two rows"),
    (1023, 64, True, True, False, "below the switch to the three-launch path"),
    (1024, 64, True, True, False, "the last size of the one-launch kernels"),
    (1025, 64, True, True, False, "the first size of the three-launch path"),
    (1025, 32, True, False, True, "no ReLU, with a residual"),
    (3000, 64, False, True, False, "three-launch backward in eval"),
    (3000, 256, False, True, True, "three-launch backward in eval, with a residual"),
    (1024, 128, False, True, False, "one-launch backward in eval"),
]


def case_id(c):
    return "-".join({True: "T", False: "F"}.get(v, str(v)) if isinstance(v, bool) else str(v) for v in c[:-1])


def _rng(stage, c):
    return np.random.default_rng(zlib.crc32(repr((stage,) + tuple(c[:-1])).encode()))


_cache = {}


def act_inputs(c):
    """float32 numpy inputs of a CASES_ACT entry: y, gamma, beta, g, rm, rv (settled; shared and read-only)"""
    if ("act", c) not in _cache:
        M, C, training, slope, _ = c
        rng = _rng("act", c)
        y, gamma, beta = channels("act", M, C, rng)
        rm, rv = running_buffers(y, C, training, rng)
        y, _ = settle(y, gamma, beta, training, rm, rv, movable=y.astype(np.float64).std(0) > 0 if training else None)
        d = dict(y=y, gamma=gamma, beta=beta, g=rng.standard_normal((M, C)).astype(np.float32), rm=rm, rv=rv)
        _cache[("act", c)] = _freeze(d)
    return _cache[("act", c)]


def max_inputs(c):
    """float32 numpy inputs of a CASES_MAX entry: y (B, N, C), gamma, beta, g (B, C), rm, rv"""
    if ("max", c) not in _cache:
        B, N, C, training, _ = c
        rng = _rng("max", c)
        y, gamma, beta = channels("max", B * N, C, rng)
        rm, rv = running_buffers(y, C, training, rng)
        y, _ = settle(y, gamma, beta, training, rm, rv, N=N, movable=y.astype(np.float64).std(0) > 0 if training else None)
        d = dict(y=y.reshape(B, N, C), gamma=gamma, beta=beta, g=rng.standard_normal((B, C)).astype(np.float32), rm=rm, rv=rv)
        _cache[("max", c)] = _freeze(d)
    return _cache[("max", c)]


def rows_inputs(c):
    """float32 numpy inputs of a CASES_ROWS entry: x, res (or None), gamma, beta, g, rm, rv"""
    if ("rows", c) not in _cache:
        M, C, training, relu, has_res, _ = c
        rng = _rng("rows", c)
        x, gamma, beta = channels("rows", M, C, rng)
        rm, rv = running_buffers(x, C, training, rng)
        res = rng.standard_normal((M, C)).astype(np.float32) if has_res else None
        x, res = settle(x, gamma, beta, training, rm, rv, res=res, movable=x.astype(np.float64).std(0) > 0 if training else None)
        d = dict(x=x, res=res, gamma=gamma, beta=beta, g=rng.standard_normal((M, C)).astype(np.float32), rm=rm, rv=rv)
        _cache[("rows", c)] = _freeze(d)
    return _cache[("rows", c)]


def _freeze(d):
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def T64(a):
    return None if a is None else torch.from_numpy(np.array(a)).double()


def act_oracle(c, d=None):
    d = d or act_inputs(c)
    return bn_act(T64(d["y"]), T64(d["gamma"]), T64(d["beta"]), T64(d["g"]), c[2], c[3], T64(d["rm"]), T64(d["rv"]))


def max_oracle(c, d=None):
    d = d or max_inputs(c)
    return bn_act_max(T64(d["y"]), T64(d["gamma"]), T64(d["beta"]), T64(d["g"]), c[3], MAX_SLOPE, T64(d["rm"]), T64(d["rv"]))


def rows_oracle(c, d=None):
    d = d or rows_inputs(c)
    return bn_rows(T64(d["x"]), T64(d["res"]), T64(d["gamma"]), T64(d["beta"]), T64(d["g"]), c[2], c[3], T64(d["rm"]), T64(d["rv"]))


# --------------------------------------------------------------------------------------------------------------------- ties
TIE_B, TIE_N, TIE_C = 2, 300, 64
# tied rows of channel c: TIE_PAIRS[c % 5].  Rows r and r + 4 belong to one wave of a tile (wave = row % 4), r and r + 1 to two
# waves (the lower row in the lower wave for 21 / 22, in the HIGHER wave for 23 / 24), 127 / 128 and 40 / 168 to two tiles.
TIE_PAIRS = [(10, 14), (21, 22), (23, 24), (127, 128), (40, 168)]
TIE_VALUE = 10.0


def tie_inputs():
    """float32 y (B, N, C) of N(0, 1) clipped to +-6 with the two rows of TIE_PAIRS[c % 5] set to +10 in the channels with
    gamma >= 0 (the max of the channel) and to -10 in those with gamma < 0 (its min: the activation decreases in y there);
    gamma as channels() draws it without the zero, beta, g (B, C); running statistics mean 0 / variance 1 (eval mode)"""
    rng = np.random.default_rng(77)
    y = np.clip(rng.standard_normal((TIE_B, TIE_N, TIE_C)), -6, 6).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, TIE_C).astype(np.float32)
    gamma[::4] *= -1
    beta = rng.uniform(0.1, 1.5, TIE_C).astype(np.float32)
    for c in range(TIE_C):
        for r in TIE_PAIRS[c % 5]:
            y[:, r, c] = TIE_VALUE if gamma[c] >= 0 else -TIE_VALUE
    return _freeze(dict(y=y, gamma=gamma, beta=beta, g=rng.standard_normal((TIE_B, TIE_C)).astype(np.float32),
                        rm=np.zeros(TIE_C, np.float32), rv=np.ones(TIE_C, np.float32)))
