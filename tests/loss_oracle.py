"""Plain float64 statements of the last two stages of a training step, written from their contracts in include/fsg_hip.h and the
headers of the kernels: torch ops on the CPU, closed forms, no autograd and no kernels.
  nnu()          csrc/seg_loss.hip   fsg_nnu_loss_f32: cross-entropy(class weights) + generalised Dice, value and d loss / d logits
  chamfer_bwd()  csrc/chamfer.hip    fsg_chamfer_nn_bwd_f32: the gradient of the nearest-neighbour distances, from a GIVEN arg-min
  adam()         csrc/adam.hip       fsg_adam_flat_f32 / fsg_adam_flat_segments_f32: torch's `_single_tensor_adam` rule
tests/test_loss_oracle_cpu.py compares them with oracle/ref_cpu.py, float64 autograd and torch.optim.Adam on float64 parameters,
which is what makes them a reference, and pins the generated inputs; tests/test_loss_family_gpu.py compares the kernels with them.
Every function takes `dtype`: float64 is the reference, float32 the same statement in the kernels' number format.

Every value comes with `mag`, the sum of the absolute summands it is made of (tests/bn_oracle.py), so that one relative bar
|got - fp64| / mag holds for well- and ill-conditioned elements:
  seg loss   dL/dz_c(i) = p_c (g_c - sum_c' p_c' g_c') + w_ce w[y] / sum w (p_c - [y = c]),  g_c = w_dice (A_c + [y = c] E_c):
             mag = p_c (|g_c| + sum_c' p_c' |g_c'|) + w_ce w[y] / sum w (p_c + [y = c]).  In mag a probability counts as at least
             2^-126: below fp32's normal range exp() may give 0, and an element all of whose summands carry such a p_c is then
             off by its whole (invisible) value; and 2^-126 is added to the element's mag: a gradient of 6.7e-44 is a denormal
             with five bits (logits of scale 40: without this term the figure of such an element is 6.7e-5, for ATen and the
             fp32 run of this file alike).  A point whose label lies outside [0, C) has no summands: mag 0, gradient 0.
  Chamfer    grad_x[i] = 2 g_i (x_i - y_a): mag 2 |g_i| (|x_i| + |y_a|);  grad_y[j] = -sum over arg_i = j: the sum of those mags.
  Adam       the recurrences with every summand replaced by its absolute value, carried through ALL steps (a moment that cancelled
             in step 2 still holds the roundings of its summands in step 4):  mag_p += |update|, from |p_0|;
             mag_m = b1 mag_m + (1 - b1) (|g| + wd mag_p);  mag_v = b2 mag_v + (1 - b2) (|g| + wd mag_p)^2.  Each plus 2^-126: below
             fp32's normal range the spacing is absolute (v of a gradient of 1e-20 is a denormal with a handful of bits).
"""
import zlib

import numpy as np
import torch

TINY32 = 2.0 ** -126          # the lower end of fp32's normal range


def T(a, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.array(a)).to(dtype)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# --------------------------------------------------------------------------------------------------------------------- seg loss

def nnu(logits, labels, w=None, w_ce=1.0, w_dice=1.0, smooth=1.0, dtype=torch.float64):
    """logits (B, C, N), labels (B, N) int64, w (C,) or None -> dict(total, ce, gdl, n_bad, grad (B, C, N), mag (B, C, N)).
    Per class over the points with a label in [0, C): tp_c = sum p_c [y = c], sp_c = sum p_c, cnt_c = sum [y = c],
    vol_c = cnt_c + 1e-6; tp, fp, fn = sum_c (tp_c, sp_c - tp_c, cnt_c - tp_c) / vol_c; num = 2 tp + s, den = 2 tp + fp + fn + s,
    gdl = -num / den; ce = -sum w[y] log p_y / sum w[y]; total = w_ce ce + w_dice gdl.  d den / d p_c(i) = 1 / vol_c and
    d num / d p_c(i) = 2 [y = c] / vol_c give A_c = num / (vol_c den^2), E_c = -2 / (vol_c den)."""
    z = logits.to(dtype)
    B, C, N = z.shape
    valid = (labels >= 0) & (labels < C)
    y = labels.clamp(0, C - 1)
    vm = valid[:, None, :].to(dtype)
    wv = torch.ones(C, dtype=dtype) if w is None else w.to(dtype)
    zs = z - z.max(1, keepdim=True).values
    e = zs.exp()
    s = e.sum(1, keepdim=True)
    p, logp = e / s, zs - s.log()
    onehot = torch.zeros_like(p).scatter_(1, y[:, None, :], 1.0) * vm
    wy = wv[y] * valid.to(dtype)                                               # (B, N)
    ce_den = wy.sum()
    ce = -(wy * (logp * onehot).sum(1)).sum() / ce_den
    tp_c, sp_c, cnt_c = (p * onehot).sum((0, 2)), (p * vm).sum((0, 2)), onehot.sum((0, 2))
    vol = cnt_c + 1e-6
    tp, fp, fn = (tp_c / vol).sum(), ((sp_c - tp_c) / vol).sum(), ((cnt_c - tp_c) / vol).sum()
    num, den = 2 * tp + smooth, 2 * tp + fp + fn + smooth
    gdl = -num / den
    A, E = (w_dice * num / (vol * den * den))[None, :, None], (-w_dice * 2.0 / (vol * den))[None, :, None]
    g, gm = A + onehot * E, A.abs() + onehot * E.abs()
    cs = (w_ce * wy / ce_den)[:, None, :]
    grad = (p * (g - (p * g).sum(1, keepdim=True)) + cs * (p - onehot)) * vm
    pm = p + TINY32
    mag = (pm * (gm + (pm * gm).sum(1, keepdim=True)) + cs.abs() * (pm + onehot) + TINY32) * vm
    return dict(total=w_ce * ce + w_dice * gdl, ce=ce, gdl=gdl, n_bad=int((~valid).sum()), grad=grad, mag=mag)


def nnu_autograd(zv, yv, w, w_ce, w_dice, smooth):
    """the same loss as a composition for autograd, on the points that count: zv (P, C) logits of any dtype / device, yv (P,) labels
    in [0, C) -> (total, ce, gdl).  F.cross_entropy(weight=w) + the Dice closed form on softmax(zv)."""
    ce = torch.nn.functional.cross_entropy(zv, yv, weight=w)
    p = torch.softmax(zv, 1)
    onehot = torch.zeros_like(p).scatter_(1, yv[:, None], 1.0)
    tp_c, sp_c, cnt_c = (p * onehot).sum(0), p.sum(0), onehot.sum(0)
    vol = cnt_c + 1e-6
    tp, fp, fn = (tp_c / vol).sum(), ((sp_c - tp_c) / vol).sum(), ((cnt_c - tp_c) / vol).sum()
    gdl = -(2 * tp + smooth) / (2 * tp + fp + fn + smooth)
    return w_ce * ce + w_dice * gdl, ce, gdl


# (name, B, N, C, weighted, logits, labels, reason).  logits: ("scale", s) = s N(0, 1); ("offset", s, o) = s N(0, 1) + o.
# labels: "uniform" = every class; "bad5" = about 5 % drawn from {-1, -100, C, C + 7}; "cloud_bad" = every point of cloud 1
# invalid; "drop_last" = no point of class C - 1; "one_class" = every point has class 1.
SEG_GRID = [
    ("pts-1x1", 1, 1, 4, True, ("scale", 2.0), "uniform", "single point"),
    ("pts-1x255", 1, 255, 4, True, ("scale", 2.0), "uniform", "one short of a workgroup"),
    ("pts-1x256", 1, 256, 4, True, ("scale", 2.0), "uniform", "exactly one workgroup"),
    ("pts-1x257", 1, 257, 4, True, ("scale", 2.0), "uniform", "a one-point second workgroup"),
    ("pts-3x5462", 3, 5462, 4, True, ("scale", 2.0), "uniform",
     "16386 points = 64 x 256 + 2: two threads run a second iteration, in another cloud than their first"),
    ("pts-3x5462-now", 3, 5462, 4, False, ("scale", 2.0), "uniform", "the same without class weights"),
    ("pts-7x7033", 7, 7033, 4, True, ("scale", 2.0), "uniform", "49231 points: three to four iterations, ragged"),
]
SEG_CLASSES = [("C-%d" % C, 2, 130, C, True, ("scale", 2.0), "uniform",
                "both sides of the template (4|5, 8|9, 16|17) and Rp (4|5, 9|10, 20|21) boundaries")
               for C in (2, 4, 5, 8, 9, 10, 16, 17, 20, 21, 32)]
SEG_LABELS = [
    ("lab-bad5", 3, 700, 5, True, ("scale", 2.0), "bad5", "about 5 % of the labels outside [0, C)"),
    ("lab-cloud-bad", 3, 300, 4, True, ("scale", 2.0), "cloud_bad", "every point of cloud 1 invalid"),
    ("lab-drop-last", 2, 500, 4, True, ("scale", 2.0), "drop_last", "no point of the last class: its volume term is 1 / 1e-6"),
    ("lab-one-class", 2, 300, 4, True, ("scale", 2.0), "one_class", "all points have one class"),
    ("lab-wrap32", 2, 300, 4, True, ("scale", 2.0), "wrap32",
     "invalid labels whose low 32 bits are a valid class (+-2^32 + 1): the range test must see all 64 bits"),
]
WRAP_LABELS = np.array([-(1 << 32) + 1, (1 << 32) + 1], dtype=np.int64)
SEG_LOGITS = [
    ("logit-scale40", 2, 300, 6, True, ("scale", 40.0), "uniform", "exp underflows for most classes"),
    ("logit-offset1e4", 2, 300, 6, True, ("offset", 2.0, 1e4), "uniform", "+1e4 on every class: shift-invariant in exact arithmetic"),
]
SEG_CASES = SEG_GRID + SEG_CLASSES + SEG_LABELS + SEG_LOGITS
SEG_PARAMS = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.3, 2.0)]          # (w_ce, w_dice)
SEG_SMOOTH = [1.0, 0.0]
BAD_LABELS = lambda C: np.array([-1, -100, C, C + 7])                   # noqa: E731


def seg_id(c):
    return c[0]


def seg_case(name):
    return [c for c in SEG_CASES if c[0] == name][0]


_cache = {}


def seg_inputs(c):
    """float32 logits (B, C, N), int64 labels (B, N), float32 class weights or None of a SEG_CASES entry (shared, read-only).
    Every class that the case does not drop on purpose has at least one point (label 0 .. C - 1 are dealt out first)."""
    if ("seg", c[0]) not in _cache:
        name, B, N, C, weighted, lg, lab, _ = c
        rng = _rng("seg", name)
        z = rng.standard_normal((B, C, N)) * lg[1]
        if lg[0] == "offset":
            z = z + lg[2]
        hi = C - 1 if lab == "drop_last" else C
        y = rng.integers(0, hi, (B, N)).astype(np.int64)
        if lab == "one_class":
            y[:] = 1
        elif B * N >= hi:
            flat = y.reshape(-1)
            flat[rng.permutation(B * N)[:hi]] = np.arange(hi)          # every kept class is present
        if lab == "wrap32":
            y[:, 7::10] = np.resize(WRAP_LABELS, y[:, 7::10].shape)
            y[0, :C * 10:10] = np.arange(C)
        if lab == "bad5":
            bad = rng.random((B, N)) < 0.05
            keep = np.zeros(B * N, bool)
            for cls in range(C):                                       # one point of every class stays valid
                keep[np.flatnonzero(y.reshape(-1) == cls)[0]] = True
            bad &= ~keep.reshape(B, N)
            y[bad] = rng.choice(BAD_LABELS(C), int(bad.sum()))
        elif lab == "cloud_bad":
            y[1] = np.resize(BAD_LABELS(C), N)
            flat = y[[0, 2]].reshape(-1)
            flat[:C] = np.arange(C)
            y[0], y[2] = flat[:N], flat[N:]
        w = (0.5 + rng.random(C)).astype(np.float32) if weighted else None
        _cache[("seg", c[0])] = _freeze(dict(logits=z.astype(np.float32), labels=y, w=w))
    return _cache[("seg", c[0])]


def seg_oracle(c, w_ce=1.0, w_dice=1.0, smooth=1.0, dtype=torch.float64):
    d = seg_inputs(c)
    return nnu(T(d["logits"], dtype), torch.from_numpy(np.array(d["labels"])), T(d["w"], dtype), w_ce, w_dice, smooth, dtype)


# --------------------------------------------------------------------------------------------------------------------- Chamfer

def chamfer_bwd(x, y, arg, g, dtype=torch.float64):
    """x (B, N, 3), y (B, M, 3), arg (B, N) integer, g (B, N) = d loss / d dist -> dict(grad_x, grad_y, mag_x, mag_y):
    grad_x[i] = 2 g_i (x_i - y_arg(i)), grad_y[j] = -sum over arg(i) = j of the same."""
    x, y, g = x.to(dtype), y.to(dtype), g.to(dtype)
    a = arg.long()[:, :, None].expand(-1, -1, 3)
    ya = y.gather(1, a)
    gx = 2.0 * g[:, :, None] * (x - ya)
    mx = 2.0 * g.abs()[:, :, None] * (x.abs() + ya.abs())
    gy = torch.zeros_like(y).scatter_add_(1, a, -gx)
    my = torch.zeros_like(y).scatter_add_(1, a, mx)
    return dict(grad_x=gx, grad_y=gy, mag_x=mx, mag_y=my)


# forward: (B, N, M, reason); B = 2 for every other one, so the batch strides are used
CH_QUERY_N = [1, 63, 64, 65, 127, 128, 129, 300]            # the query tile of 128, two per lane
CH_TARGET_M = [1, 127, 128, 129, 1023, 1024, 1025, 2049]    # the 1024-candidate tile over eight waves of 128
CH_FWD = []
for _i, _n in enumerate(CH_QUERY_N):
    CH_FWD.append((1 + _i % 2, _n, 129, "query-tile edge, two wave slices"))
    CH_FWD.append((2 - _i % 2, _n, 1025, "query-tile edge, a one-candidate second tile"))
for _i, _m in enumerate(CH_TARGET_M):
    if (129, _m) not in [(c[1], c[2]) for c in CH_FWD]:
        CH_FWD.append((1 + _i % 2, 129, _m, "candidate-tile edge"))


def ch_fwd_id(c):
    return "%dx%dx%d" % c[:3]


def ch_fwd_inputs(c):
    if ("chf", c[:3]) not in _cache:
        B, N, M, _ = c
        rng = _rng("chf", B, N, M)
        _cache[("chf", c[:3])] = _freeze(dict(x=rng.uniform(-1, 1, (B, N, 3)).astype(np.float32),
                                             y=rng.uniform(-1, 1, (B, M, 3)).astype(np.float32)))
    return _cache[("chf", c[:3])]


# ties: groups of target indices that hold the same point (the lowest is the original), 8 queries sit exactly on each
TIE_GROUPS = [(5, 130),            # two wave slices of one tile
              (1000, 1030),        # the last slice of tile 0 and the first of tile 1
              (3, 1027),           # the same wave in two tiles
              (0, 500, 2048)]      # a triple over three tiles
TIE_B, TIE_N, TIE_M, TIE_Q = 2, 300, 2049, 8
LATTICE_B, LATTICE_N, LATTICE_M = 2, 200, 1500


def tie_inputs():
    """x (B, 300, 3), y (B, 2049, 3) uniform in [-1, 1]^3 with the targets of every TIE_GROUPS entry equal to its first and the
    queries 8 k .. 8 k + 7 exactly on the point of group k"""
    if "tie" not in _cache:
        rng = _rng("tie")
        x = rng.uniform(-1, 1, (TIE_B, TIE_N, 3)).astype(np.float32)
        y = rng.uniform(-1, 1, (TIE_B, TIE_M, 3)).astype(np.float32)
        for k, grp in enumerate(TIE_GROUPS):
            for j in grp[1:]:
                y[:, j] = y[:, grp[0]]
            x[:, TIE_Q * k:TIE_Q * (k + 1)] = y[:, grp[0]][:, None]
        _cache["tie"] = _freeze(dict(x=x, y=y))
    return _cache["tie"]


def lattice_inputs():
    """coordinates rounded to 1/4 in [-1, 1] (9^3 = 729 lattice points for 1500 targets): many exactly equal distances and many
    duplicated targets"""
    if "lattice" not in _cache:
        rng = _rng("lattice")
        x = np.round(rng.uniform(-1, 1, (LATTICE_B, LATTICE_N, 3)) * 4) / 4
        y = np.round(rng.uniform(-1, 1, (LATTICE_B, LATTICE_M, 3)) * 4) / 4
        _cache["lattice"] = _freeze(dict(x=x.astype(np.float32), y=y.astype(np.float32)))
    return _cache["lattice"]


def duplicate_groups(y):
    """sorted list of the index tuples of equal rows of y (M, 3)"""
    _, inv, cnt = np.unique(y, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    return sorted(tuple(np.flatnonzero(inv == u)) for u in np.flatnonzero(cnt > 1))


# backward: (N, M, dup, reason), all with CH_BWD_B clouds.  dup = (low, high): target `high` is a copy of target `low`
CH_BWD_B = 3
CH_BWD = [
    (700, 450, (4, 5), "the size of the older test"),
    (1, 1, None, "smallest"),
    (257, 1, None, "one target takes all queries"),
    (4096, 3, None, "every target above 1024 in-edges: the `tmp` branch of csr_sort_rows_kernel"),
    (4096, 12, None, "collapsed, below the cap of the LDS sort"),
    (12, 4096, None, "almost all rows empty"),
    (300, 9000, (17, 8999), "8192 < M <= 16384: the count / scan / fill route"),
    (300, 16400, None, "M above the LDS limit of the builder: the ordered path falls back to atomics"),
]
CH_ORDERED_MAX_M = 16384          # csrc/edgeconv.hip fsg_csr_bipartite_launch: sizeof(int) M <= 64 KB
CH_G_SCALE = [1.0, 1e-3, 50.0]    # per cloud
CH_DUP_Q = slice(5, 9)            # the queries next to a duplicated target


def ch_bwd_id(c):
    return "%dto%d" % c[:2]


def ch_bwd_inputs(c):
    """x, y as above (dup applied) and g (B, N): N(0, 1) x the cloud's scale, about 10 % exact zeros"""
    if ("chb", c[:2]) not in _cache:
        N, M, dup, _ = c
        rng = _rng("chb", N, M)
        x = rng.uniform(-1, 1, (CH_BWD_B, N, 3)).astype(np.float32)
        y = rng.uniform(-1, 1, (CH_BWD_B, M, 3)).astype(np.float32)
        if dup:                   # queries CH_DUP_Q sit 1e-3 from the duplicated point: it is somebody's nearest neighbour
            y[:, dup[1]] = y[:, dup[0]]
            x[:, CH_DUP_Q] = (y[:, dup[0]][:, None] + 1e-3 * rng.standard_normal((CH_BWD_B, 4, 3))).astype(np.float32)
        g = rng.standard_normal((CH_BWD_B, N)) * np.array(CH_G_SCALE)[:, None]
        g[rng.random((CH_BWD_B, N)) < 0.1] = 0.0
        if N >= 12:
            g[:, 3] = 0.0
        if dup:
            g[:, CH_DUP_Q] = np.array(CH_G_SCALE)[:, None] * np.array([1.0, -0.5, 2.0, 0.25])
        _cache[("chb", c[:2])] = _freeze(dict(x=x, y=y, g=g.astype(np.float32)))
    return _cache[("chb", c[:2])]


# --------------------------------------------------------------------------------------------------------------------- Adam

def f32(v):
    """the value a float argument of the C entry points carries"""
    return float(np.float32(v))


def adam(p, g_steps, lr_steps, b1, b2, eps, wd, dtype=torch.float64, t0=0):
    """the rule in the header of csrc/adam.hip (torch/optim/adam.py `_single_tensor_adam`: L2 weight decay, no amsgrad) from
    zero moments, step count t0 + 1, t0 + 2, ...:
      g' = g + wd p;  m = m + (1 - b1) (g' - m);  v = b2 v + (1 - b2) g'^2;  p -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    p (n,), g_steps a list of (n,) gradients, lr_steps one learning rate per step; the hyper-parameters as the kernel receives them
    (rounded to float).  Returns one dict(p, m, v, mag_p, mag_m, mag_v) per step."""
    b1, b2, eps, wd = f32(b1), f32(b2), f32(eps), f32(wd)
    p = p.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    mag_p, mag_m, mag_v = p.abs(), torch.zeros_like(p), torch.zeros_like(p)      # the summands of ALL steps so far
    out = []
    for k, (g, lr) in enumerate(zip(g_steps, lr_steps)):
        t = t0 + k + 1
        g = g.to(dtype)
        gp, gpm = g + wd * p, g.abs() + wd * mag_p
        mag_m, mag_v = b1 * mag_m + (1 - b1) * gpm, b2 * mag_v + (1 - b2) * gpm * gpm
        m = m + (1 - b1) * (gp - m)
        v = b2 * v + (1 - b2) * gp * gp
        upd = (f32(lr) / (1 - b1 ** t)) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        mag_p = mag_p + upd.abs()
        p = p - upd
        out.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), mag_p=mag_p + TINY32, mag_m=mag_m + TINY32, mag_v=mag_v + TINY32))
    return out


ADAM_HP = dict(b1=0.9, b2=0.999, eps=1e-8)
ADAM_WD = [0.0, 1e-2]
ADAM_STEPS = 4
ADAM_LR = [1e-2, 1e-2, 5e-3, 5e-3]                       # changed before step 3
ADAM_BIG = 4 * (1024 * 256) + 4 * 300 + 3                # 1 049 779: one grid-stride iteration for 300 float4 plus a tail of 3
ADAM_FLAT_N = [1, 2, 3, 4, 5, 1023, ADAM_BIG]
ADAM_SEG_SHAPES = [(1024, 1000), (25, 1000), (16, 4), (4,), (8, 8)]
ADAM_MAX_CHUNKS = 224                                    # csrc/adam.hip FSG_ADAM_MAX_CHUNKS
ADAM_TICKET_N = [ADAM_BIG, 8, 4100]                      # 1024 workgroups, then 1, then 5 on ONE state
ADAM_BLOCK_MIN_N = 1023                                  # from this size on a fixture carries the element blocks below
ADAM_TINY_G, ADAM_HUGE_G = 1e-20, 1e3


def adam_blocks(n):
    """name -> slice of the element blocks of a fixture of n >= ADAM_BLOCK_MIN_N elements (each n // 8 long):
    zero: g == 0 in every step;  tiny: |g| about 1e-20 (v denormal or zero, the denominator is eps);  huge: g = +-1e3;
    late_zero: g == 0 from step 3 on (m and v decay);  the rest: N(0, 1) x the step's scale"""
    k = n // 8
    return dict(zero=slice(0, k), tiny=slice(k, 2 * k), huge=slice(2 * k, 3 * k), late_zero=slice(3 * k, 4 * k))


def adam_inputs(n):
    """float32 p (n,) and ADAM_STEPS gradients (n,); the gradient scale changes per step (0.1 + step)"""
    if ("adam", n) not in _cache:
        rng = _rng("adam", n)
        p = rng.standard_normal(n).astype(np.float32)
        gs = []
        for s in range(ADAM_STEPS):
            g = rng.standard_normal(n) * (0.1 + s)
            if n >= ADAM_BLOCK_MIN_N:
                b = adam_blocks(n)
                k = n // 8
                g[b["zero"]] = 0.0
                g[b["tiny"]] = ADAM_TINY_G * rng.uniform(0.5, 2.0, k) * np.where(rng.random(k) < 0.5, -1.0, 1.0)
                g[b["huge"]] = ADAM_HUGE_G * np.where(rng.random(k) < 0.5, -1.0, 1.0)
                if s >= 2:
                    g[b["late_zero"]] = 0.0
            gs.append(g.astype(np.float32))
        _cache[("adam", n)] = _freeze(dict(p=p, g=gs))
        for g in gs:
            g.setflags(write=False)
    return _cache[("adam", n)]


def adam_oracle(n, wd, dtype=torch.float64, steps=ADAM_STEPS, t0=0):
    d = adam_inputs(n)
    return adam(T(d["p"], dtype), [T(g, dtype) for g in d["g"][:steps]], ADAM_LR[:steps], wd=wd, dtype=dtype, t0=t0, **ADAM_HP)
