"""numpy oracles of the DSEG-AE kernels (csrc/dseg_ae.hip), written from their rules:

  partition : every (item, object) group takes its points in ascending order of their index; groups in (item, object) order
  extend    : mean and unbiased standard deviation of every point's distance to the nearest OTHER point of its segment; a padded
              row is xyz[src] + direction / |direction| * (z * std + mean); fewer than two points: mean = std = 0
  fps       : start at the given row, then always the point whose distance to the chosen set is largest, the lowest index among
              equals

`extend` runs in fp64 (the oracle) or in fp32 (`dtype=np.float32`: a plain restatement whose distance to the oracle says what
fp32 arithmetic costs on an input -- the tests' bar is a multiple of it)."""
import numpy as np

GOLDEN_SEED, GOLDEN_N, GOLDEN_TARGET = 20241, 700, 1024     # tests/golden/dseg_ae_extend.npz (tools/make_golden_dseg_ae.py)
FLOOR = 4.8e-7      # of the coordinate magnitude: 4 ulp of fp32 (the house bar's floor)


def partition(labels, x, num_labels, first_label=1):
    """labels (B, N) ints, x (B, C, N) -> counts (B, L) int32, offset (B L) int32, xyz (B N, 3) fp32, src (B N) int32 (rows past
    offset[-1] zero)"""
    B, N = labels.shape
    counts = np.zeros((B, num_labels), np.int32)
    xyz, src = np.zeros((B * N, 3), np.float32), np.zeros(B * N, np.int32)
    q = 0
    for b in range(B):
        for l in range(num_labels):
            rows = np.flatnonzero(labels[b].astype(np.int64) == first_label + l)
            counts[b, l] = len(rows)
            xyz[q:q + len(rows)] = x[b, :3][:, rows].T
            src[q:q + len(rows)] = rows
            q += len(rows)
    return counts, np.cumsum(counts.reshape(-1)).astype(np.int32), xyz, src


def _bounds(ends):
    ends = [int(e) for e in ends]
    return list(zip([0] + ends[:-1], ends))


def nearest_other(pts):
    """pts (n, 3), n >= 2 -> distance of every point to the nearest other one, direct form, in pts.dtype"""
    d2 = np.full((len(pts), len(pts)), np.inf, pts.dtype)
    for a in range(0, len(pts), 256):       # (blocks: bounded memory)
        diff = pts[a:a + 256, None, :] - pts[None, :, :]
        d2[a:a + 256] = (diff * diff).sum(-1, dtype=pts.dtype)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(d2.min(1))


def extend(xyz, ends, targets, src_idx, direction, z, dtype=np.float64):
    """-> out (n_new, 3), new_ends, stats (G, 2), all in dtype.  The draws are packed over the padded rows in segment order."""
    xyz, direction, z = xyz.astype(dtype), np.asarray(direction).reshape(-1, 3).astype(dtype), np.asarray(z).reshape(-1).astype(dtype)
    bounds = _bounds(ends)
    targets = [int(targets)] * len(bounds) if np.isscalar(targets) else [int(t) for t in targets]
    out, stats, new_ends, p = [], [], [], 0
    for (st, en), tg in zip(bounds, targets):
        pts = xyz[st:en]
        mean = std = dtype(0)
        if en - st >= 2:
            nn = nearest_other(pts)
            mean, std = nn.mean(dtype=dtype), nn.std(ddof=1, dtype=dtype)
        pad = max(tg - (en - st), 0)
        d, s = direction[p:p + pad], np.asarray(src_idx[p:p + pad], np.int64)
        norm = np.sqrt((d * d).sum(1, dtype=dtype))[:, None]
        out += [pts, pts[s] + d / norm * (z[p:p + pad, None] * std + mean)]
        stats.append([mean, std])
        new_ends.append((new_ends[-1] if new_ends else 0) + en - st + pad)
        p += pad
    return np.concatenate(out).astype(dtype), np.array(new_ends, np.int32), np.array(stats, dtype)


def fps(xyz, ends, n_samples, starts=None):
    """fp64 farthest point sampling per segment -> one index list (rows of xyz) per segment; an empty segment gives zeros"""
    out = []
    for g, (st, en) in enumerate(_bounds(ends)):
        m = int(n_samples[g])
        if en == st:
            out.append(np.zeros(m, np.int64))
            continue
        axes = [np.ascontiguousarray(xyz[st:en, a], np.float64) for a in range(3)]
        cur = int(starts[g]) if starts is not None else 0
        md, d, tmp = np.full(en - st, np.inf), np.empty(en - st), np.empty(en - st)
        idx = np.empty(m, np.int64)
        for t in range(m):
            idx[t] = st + cur
            d.fill(0.)
            for p in axes:                  # (one axis at a time into preallocated rows: this loop is the tests' whole cost)
                np.subtract(p, p[cur], out=tmp)
                np.multiply(tmp, tmp, out=tmp)
                d += tmp
            np.minimum(md, d, out=md)
            cur = int(md.argmax())          # the first of equal maxima: the lowest index
        out.append(idx)
    return out


def golden_draws():
    """the cloud and the three draws of tests/golden/dseg_ae_extend.npz, replayed from its seed on torch's CPU generator in the
    order the reference makes them: the cloud, the source rows, the directions, the magnitudes"""
    import torch
    gen_state = torch.random.get_rng_state()
    try:
        torch.manual_seed(GOLDEN_SEED)
        pad = GOLDEN_TARGET - GOLDEN_N
        points = torch.rand(1, GOLDEN_N, 3)
        src = torch.randint(GOLDEN_N, (pad,))
        direction = torch.randn(1, pad, 3)
        z = torch.randn(1, pad, 1)
    finally:
        torch.random.set_rng_state(gen_state)
    return points, src, direction, z
