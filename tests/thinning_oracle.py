"""numpy oracle of csrc/thinning.hip: the two-sub-iteration thinning of Gonzalez & Woods (what ITK's
BinaryThinningImageFilter documents) in the (y, x) plane of every slice of a (..., H, W) volume, with clamped borders.

(a) `thin`        the rule voxel by voxel on np.pad(mode='edge') neighbours -> (result bool, pairs per slice)
(b) `thin_words`  the kernel's formulation restated on uint64 words: shifts with carries from the adjacent words, border bits,
                  the bit-sliced neighbour count, the running ones / twos of the transition planes, the tail mask
(c) scene builders shared by the tests and tools/bench_kernels.py

Neighbours of p1 = (y, x): p2 (y-1, x), p3 (y-1, x+1), p4 (y, x+1), p5 (y+1, x+1), p6 (y+1, x), p7 (y+1, x-1), p8 (y, x-1),
p9 (y-1, x-1).  A step marks the set voxels with 2 <= p2 + ... + p9 <= 6, exactly one 0 -> 1 transition in the cycle
p2, p3, ..., p9, p2, and (odd step) p2 p4 p6 = 0 and p4 p6 p8 = 0 / (even step) p2 p4 p8 = 0 and p2 p6 p8 = 0, then clears them
all at once.  Odd and even steps alternate until a pair clears nothing in the slice; a slice's count is the number of pairs
that cleared something.  Parity with SimpleITK is unpinned: this file is the authority."""
import numpy as np

OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # p2 .. p9 as (dy, dx)


# ------------------------------------------------------------------------------------------------------ (a) per voxel
def _neighbours(img, border):
    """img (S, H, W) uint8 -> the eight planes p2..p9; border 'edge' (the rule) or 'zero' (to show that it matters)"""
    H, W = img.shape[-2:]
    pad = np.pad(img, ((0, 0), (1, 1), (1, 1)), mode="edge") if border == "edge" else np.pad(img, ((0, 0), (1, 1), (1, 1)))
    return [pad[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in OFFSETS]


def step_marks(img, odd, border="edge"):
    """the voxels that one step clears: img (S, H, W) uint8 of 0 / 1 -> bool"""
    p = [x.astype(np.int32) for x in _neighbours(img, border)]
    p2, p3, p4, p5, p6, p7, p8, p9 = p
    n = sum(p)
    trans = sum((p[k] == 0) & (p[(k + 1) % 8] == 1) for k in range(8))
    if odd:
        cd = (p2 * p4 * p6 == 0) & (p4 * p6 * p8 == 0)
    else:
        cd = (p2 * p4 * p8 == 0) & (p2 * p6 * p8 == 0)
    return (img == 1) & (n >= 2) & (n <= 6) & (trans == 1) & cd


def thin(vol, border="edge"):
    """vol (..., H, W), nonzero = set -> (thinned bool of the same shape, pairs int32 of shape vol.shape[:-2]).  All slices
    step together: a slice whose pair cleared nothing is at a fixed point of both steps, so going on changes nothing in it."""
    vol = np.asarray(vol)
    img = (vol != 0).astype(np.uint8).reshape((-1,) + vol.shape[-2:])
    pairs = np.zeros(img.shape[0], np.int32)
    cap = img.shape[1] * img.shape[2] + 1
    for _ in range(cap):
        cleared = np.zeros(img.shape[0], bool)
        for odd in (True, False):
            m = step_marks(img, odd, border)
            cleared |= m.any(axis=(1, 2))
            img = img & ~m
        if not cleared.any():
            break
        pairs += cleared
    return img.astype(bool).reshape(vol.shape), pairs.reshape(vol.shape[:-2])


# ------------------------------------------------------------------------------------------------------ (b) on words
def pack_words(vol):
    """(..., H, W) nonzero = set -> (..., H, ceil(W / 64)) uint64: bit i of word j is voxel x = 64 j + i, bits past W are 0"""
    b = np.asarray(vol) != 0
    W = b.shape[-1]
    WW = (W + 63) // 64
    padded = np.zeros(b.shape[:-1] + (WW * 64,), np.uint8)
    padded[..., :W] = b
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").astype(np.uint64).reshape(b.shape[:-1] + (WW,))


def unpack_words(words, W):
    by = np.ascontiguousarray(words.astype("<u8")).view(np.uint8)
    return np.unpackbits(by, axis=-1, bitorder="little")[..., :W].astype(bool)


def _east_west(rows, W):
    """rows (S, H, WW) uint64 -> (the plane of the x + 1 neighbours, of the x - 1 neighbours), clamped at x = W - 1 and x = 0"""
    one, s63 = np.uint64(1), np.uint64(63)
    WW = rows.shape[-1]
    right = np.zeros_like(rows)
    right[..., :-1] = rows[..., 1:]
    left = np.zeros_like(rows)
    left[..., 1:] = rows[..., :-1]
    east = (rows >> one) | (right << s63)
    west = (rows << one) | (left >> s63)
    east[..., WW - 1] |= rows[..., WW - 1] & (one << np.uint64((W - 1) & 63))     # x = W - 1 reads itself
    west[..., 0] |= rows[..., 0] & one                                              # x = 0 reads itself
    return east, west


def step_words(cur, W, odd):
    """one step on (S, H, WW) uint64 words -> the words after it"""
    up = np.concatenate((cur[:, :1], cur[:, :-1]), axis=1)         # row y - 1, clamped at y = 0
    dn = np.concatenate((cur[:, 1:], cur[:, -1:]), axis=1)         # row y + 1, clamped at y = H - 1
    p2, p6 = up, dn
    p3, p9 = _east_west(up, W)
    p4, p8 = _east_west(cur, W)
    p5, p7 = _east_west(dn, W)
    # (a) the count of the eight planes, bit-sliced: full adders down to the four bits b3 b2 b1 b0
    s1, c1 = p2 ^ p3 ^ p4, (p2 & p3) | (p4 & (p2 ^ p3))
    s2, c2 = p5 ^ p6 ^ p7, (p5 & p6) | (p7 & (p5 ^ p6))
    s3, c3 = p8 ^ p9, p8 & p9
    b0, c4 = s1 ^ s2 ^ s3, (s1 & s2) | (s3 & (s1 ^ s2))
    t1, d1 = c1 ^ c2 ^ c3, (c1 & c2) | (c3 & (c1 ^ c2))
    b1, d2 = t1 ^ c4, t1 & c4
    b2, b3 = d1 ^ d2, d1 & d2
    cond_a = (b1 | b2 | b3) & ~(b3 | (b2 & b1 & b0))               # not below 2, not 7 or 8
    # (b) exactly one of the eight transition planes
    ring = (p2, p3, p4, p5, p6, p7, p8, p9, p2)
    ones, twos = np.zeros_like(cur), np.zeros_like(cur)
    for k in range(8):
        t = ~ring[k] & ring[k + 1]
        twos |= ones & t
        ones |= t
    cond_b = ones & ~twos
    cond_cd = (~(p4 & p6) | ~(p2 | p8)) if odd else (~(p2 & p8) | ~(p4 | p6))
    return cur & ~(cond_a & cond_b & cond_cd)


def thin_words(vol):
    """`thin` through the word formulation: (..., H, W) -> (thinned bool, pairs int32)"""
    vol = np.asarray(vol)
    H, W = vol.shape[-2:]
    cur = pack_words(vol).reshape(-1, H, (W + 63) // 64)
    tail = np.full(cur.shape[-1], ~np.uint64(0))
    if W & 63:
        tail[-1] = (np.uint64(1) << np.uint64(W & 63)) - np.uint64(1)
    pairs = np.zeros(cur.shape[0], np.int32)
    for _ in range(H * W + 1):
        a = step_words(cur, W, True)
        b = step_words(a, W, False)
        cleared = ((cur ^ b) != 0).any(axis=(1, 2))                # steps only clear, so cur ^ b is all that the pair cleared
        cur = b
        if not cleared.any():
            break
        pairs += cleared
    cur &= tail
    return unpack_words(cur, W).reshape(vol.shape), pairs.reshape(vol.shape[:-2])


# ------------------------------------------------------------------------------------------------------ (c) scenes
SHAPES = ((1, 1, 1), (2, 1, 9), (2, 9, 1), (3, 17, 63), (3, 17, 64), (3, 17, 65), (2, 33, 130), (2, 5, 128))
DENSITIES = (0.3, 0.6, 0.85, 1.0)


def random_field(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def density_batch(shape):
    """the four densities of one shape as a batch (4, D, H, W)"""
    return np.stack([random_field(shape, d, 1000 * k + sum(shape)) for k, d in enumerate(DENSITIES)])


def disc(size=64, radius=28):
    y, x = np.mgrid[:size, :size]
    c = size // 2
    return (y - c) ** 2 + (x - c) ** 2 <= radius ** 2


def shapes_scene():
    """(3, 60, 150): an ellipse over the 63|64 and 127|128 word boundaries, a slanted band from border to border, and a cross
    that touches three borders"""
    y, x = np.mgrid[:60, :150]
    ellipse = ((y - 30) / 22.0) ** 2 + ((x - 90) / 50.0) ** 2 <= 1
    band = np.abs(y - 0.35 * x - 3) <= 4
    cross = (np.abs(x - 64) <= 3) | ((np.abs(y - 40) <= 2) & (x >= 40))
    return np.stack((ellipse, band, cross))


def mixed_batch():
    """(2, 3, 64, 64): an empty slice, a full slice, the radius-28 disc; a 2 x 2 block, a 3 x 3 block, both in one slice with a
    line -- slices that finish after different numbers of pairs"""
    v = np.zeros((2, 3, 64, 64), bool)
    v[0, 1] = True
    v[0, 2] = disc()
    v[1, 0, 10:12, 20:22] = True
    v[1, 1, 30:33, 40:43] = True
    v[1, 2, 10:12, 20:22] = True
    v[1, 2, 30:33, 40:43] = True
    v[1, 2, 50, 5:60] = True
    return v


def band512(seed=7):
    """one 512 x 512 slice: a slanted band of half-width 20 plus 2 % noise"""
    y, x = np.mgrid[:512, :512]
    band = np.abs(y - 0.4 * x - 150) <= 20
    return (band | (np.random.default_rng(seed).random((512, 512)) < 0.02))[None]


def blobs(shape, seed, n=6):
    """a few random discs and boxes per slice"""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    y, x = np.mgrid[:H, :W]
    v = np.zeros(shape, bool)
    for z in range(D):
        for _ in range(n):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, max(3, min(H, W) // 3))
            if rng.random() < 0.5:
                v[z] |= (y - cy) ** 2 + (x - cx) ** 2 <= r * r
            else:
                v[z] |= (np.abs(y - cy) <= r) & (np.abs(x - cx) <= r // 2 + 1)
    return v


def two_sheets(shape=(40, 48, 56), half=1.6):
    """label volume int64 (D, H, W): two sheets of half-thickness `half` voxels (measured along y), one per lung side, each
    crossing every slice as a graph y = f(z, x): label 1 in the left half of x, label 2 in the right half"""
    D, H, W = shape
    z, y, x = np.mgrid[:D, :H, :W].astype(np.float64)
    f1 = 0.30 * H + 0.25 * x + 0.10 * z + 1.5 * np.sin(x / 5.0)
    f2 = 0.75 * H - 0.30 * (x - W / 2) + 0.08 * z
    lab = np.zeros(shape, np.int64)
    lab[(np.abs(y - f1) <= half) & (x >= 3) & (x < W // 2 - 3) & (z >= 2) & (z < D - 2)] = 1
    lab[(np.abs(y - f2) <= half) & (x >= W // 2 + 3) & (x < W - 3) & (z >= 2) & (z < D - 2)] = 2
    return lab
