"""CPU restatement of the voxel CNN (MobileNetASPP) in plain torch, written from the architecture, dtype-generic: every function
computes in the dtype of the tensors it is given (fp64 for the reference values, fp32 for the error bar).  The network is a set of
functions over a state dict {key: tensor} with the reference's keys.  Does not import the package."""
import math
from collections import OrderedDict

import torch
from torch.nn import functional as F

IN_CH = (1, 16, 24, 24, 32, 32, 32, 64)
MID_CH = (32, 96, 144, 144, 192, 192, 192, 384)
OUT_CH = (16, 24, 24, 32, 32, 32, 64, 64)
STRIDE = (1, 1, 1, 1, 1, 2, 1, 1)
RATES = (2, 4, 8, 16)
ASPP_CH = 128
EPS = 1e-5


def block_prefix(i):
    residual = IN_CH[i] == OUT_CH[i] and STRIDE[i] == 1
    return f"backbone.layers.{i + 1}." + ("module." if residual else ""), residual


# ------------------------------------------------------------------------------------------------ keys and weights
def state_shapes(num_classes):
    """the 200 keys of the reference's MobileNetASPP(num_classes).state_dict() with their shapes, in registration order"""
    out = OrderedDict()

    def conv(key, cout, cin, k, bias=False):
        out[key + ".weight"] = (cout, cin, k, k, k)
        if bias:
            out[key + ".bias"] = (cout,)

    def bn(key, c):
        for name in ("weight", "bias", "running_mean", "running_var"):
            out[f"{key}.{name}"] = (c,)
        out[key + ".num_batches_tracked"] = ()

    for i in range(8):
        p, _ = block_prefix(i)
        conv(p + "0", MID_CH[i], IN_CH[i], 3 if i == 0 else 1)
        bn(p + "1", MID_CH[i])
        conv(p + "3", MID_CH[i], 1, 3)
        bn(p + "4", MID_CH[i])
        conv(p + "6", OUT_CH[i], MID_CH[i], 1)
        bn(p + "7", OUT_CH[i])
    for j in range(len(RATES) + 2):
        conv(f"aspp.convs.{j}.0", ASPP_CH, 64, 3 if 1 <= j <= len(RATES) else 1)
        bn(f"aspp.convs.{j}.1", ASPP_CH)
    conv("aspp.project.0", ASPP_CH, (len(RATES) + 2) * ASPP_CH, 1)
    bn("aspp.project.1", ASPP_CH)
    conv("head.0", 64, ASPP_CH + 16, 1)
    bn("head.1", 64)
    conv("head.3", 64, 64, 3)
    bn("head.4", 64)
    conv("head.6", num_classes, 64, 1, bias=True)
    return out


class _Bag:
    """just enough of a module for golden_util.fill_state_dict"""

    def __init__(self, shapes):
        self.sd = OrderedDict((k, torch.zeros(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32))
                              for k, s in shapes.items())

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd):
        self.sd = OrderedDict(sd)


def filled_state(num_classes, seed):
    """the weights golden_util.fill_state_dict gives the reference's module for this seed (the values depend on key and shape only)"""
    from golden_util import fill_state_dict
    return fill_state_dict(_Bag(state_shapes(num_classes)), seed).sd


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def volume(seed, shape, scale=1.0):
    """a seeded smooth-plus-noise test volume, fp32"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float32)
    return (scale * (x + 0.5 * F.avg_pool3d(x, 3, 1, 1) * 3)).contiguous()


# ------------------------------------------------------------------------------------------------ the network
def bn(x, sd, key, training=False):
    if training:
        return F.batch_norm(x, None, None, sd[key + ".weight"], sd[key + ".bias"], True, 0.1, EPS)
    shape = (1, -1, 1, 1, 1)
    scale = sd[key + ".weight"] / torch.sqrt(sd[key + ".running_var"] + EPS)
    return (x - sd[key + ".running_mean"].view(shape)) * scale.view(shape) + sd[key + ".bias"].view(shape)


def fold(sd, key):
    scale = sd[key + ".weight"] / torch.sqrt(sd[key + ".running_var"] + EPS)
    return scale, sd[key + ".bias"] - sd[key + ".running_mean"] * scale


def relu6(x):
    return x.clamp(0, 6)


def mbconv(x, w1, s1, b1, wd, s2, b2, w3, s3, b3, stride=1, residual=False, first=False, pre=None):
    """the inverted-residual block on folded (scale, shift) pairs; `pre`: a list that receives the two pre-activations"""
    v = (1, -1, 1, 1, 1)
    cmid = wd.shape[0]
    u = F.conv3d(x, w1.reshape(cmid, -1, 3, 3, 3), stride=2, padding=1) if first else F.conv3d(x, w1.reshape(cmid, -1, 1, 1, 1))
    u = u * s1.view(v) + b1.view(v)
    t = F.conv3d(relu6(u), wd.reshape(cmid, 1, 3, 3, 3), stride=stride, padding=1, groups=cmid)
    t = t * s2.view(v) + b2.view(v)
    if pre is not None:
        pre += [u, t]
    y = F.conv3d(relu6(t), w3.reshape(w3.shape[0], cmid, 1, 1, 1)) * s3.view(v) + b3.view(v)
    return y + x if residual else y


def block_args(sd, i):
    """block i of the backbone as the arguments of `mbconv`"""
    p, residual = block_prefix(i)
    tensors = (sd[p + "0.weight"], *fold(sd, p + "1"), sd[p + "3.weight"], *fold(sd, p + "4"), sd[p + "6.weight"], *fold(sd, p + "7"))
    return tensors, dict(stride=STRIDE[i], residual=residual, first=i == 0)


BLOCK_INPUT_SCALE = 48.0


def block_input(sd, i, shape, seed, B=2, scale=BLOCK_INPUT_SCALE):
    """fp64 input (B, Cin, *shape) for a test of block i alone that makes BOTH ReLU6 clamps of the block count.  Item 0 is white
    noise.  White noise alone leaves too few entries above 6 behind the depthwise stage (its input is already clamped to
    [0, 6] and most of a small volume is border), so the other items are a probe: a constant channel vector, chosen by least
    squares to drive up the expanded channels whose depthwise kernel and scale would carry a saturated neighbourhood past 6,
    plus a quarter of white noise."""
    t, _ = block_args(cast(sd, torch.float64), i)
    w1, s1, _, wd, s2, b2 = t[:6]
    cmid = wd.shape[0]
    wanted = 6 * s2 * wd.reshape(cmid, -1).sum(1) + b2 > 7
    A = (s1[:, None] * w1.reshape(cmid, -1))[wanted]
    if i == 0:
        A = A.sum(1, keepdim=True)
    d = torch.linalg.lstsq(A, torch.ones(A.shape[0], 1, dtype=A.dtype)).solution[:, 0]
    x = torch.randn((B, IN_CH[i], *shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    x[1:] = (d / d.abs().max()).view(1, -1, 1, 1, 1) + 0.25 * x[1:]
    return x * scale


def block(x, sd, i, training=False, pre=None):
    p, residual = block_prefix(i)
    u = bn(F.conv3d(x, sd[p + "0.weight"], stride=2 if i == 0 else 1, padding=1 if i == 0 else 0), sd, p + "1", training)
    t = bn(F.conv3d(relu6(u), sd[p + "3.weight"], stride=STRIDE[i], padding=1, groups=MID_CH[i]), sd, p + "4", training)
    if pre is not None:
        pre += [u, t]
    y = bn(F.conv3d(relu6(t), sd[p + "6.weight"]), sd, p + "7", training)
    return y + x if residual else y


def backbone(x, sd, training=False, pre=None):
    x1 = block(x, sd, 0, training, pre)
    x2 = x1
    for i in range(1, 8):
        x2 = block(x2, sd, i, training, pre)
    return x1, x2


def aspp(x, sd, training=False):
    res = []
    for j in range(len(RATES) + 2):
        key = f"aspp.convs.{j}"
        if j == 0:
            y = F.conv3d(x, sd[key + ".0.weight"])
        elif j <= len(RATES):
            y = F.conv3d(x, sd[key + ".0.weight"], padding=RATES[j - 1], dilation=RATES[j - 1])
        else:
            y = F.conv3d(x.mean(dim=(2, 3, 4), keepdim=True), sd[key + ".0.weight"])
        y = torch.relu(bn(y, sd, key + ".1", training))
        res.append(y.expand(-1, -1, *x.shape[2:]))
    y = F.conv3d(torch.cat(res, dim=1), sd["aspp.project.0.weight"])
    return torch.relu(bn(y, sd, "aspp.project.1", training))     # the dropout behind it: identity in eval mode, p = 0 in the fixture


def half_res_logits(x, sd, training=False):
    x1, x2 = backbone(x, sd, training)
    y = aspp(x2, sd, training)
    y = torch.cat([x1, F.interpolate(y, scale_factor=2, mode="nearest")], dim=1)
    y = torch.relu(bn(F.conv3d(y, sd["head.0.weight"]), sd, "head.1", training))
    y = torch.relu(bn(F.conv3d(y, sd["head.3.weight"], padding=1), sd, "head.4", training))
    return F.conv3d(y, sd["head.6.weight"], sd["head.6.bias"])


def forward(x, sd, training=False):
    return F.interpolate(half_res_logits(x, sd, training), scale_factor=2, mode="trilinear", align_corners=False)


# ------------------------------------------------------------------------------------------------ patch inference
def patch_starts(size, min_overlap, patch):
    out = []
    for n, p in zip(size, patch):
        if p >= n:
            out.append([0])
            continue
        steps = math.ceil((n - p * min_overlap) / (p - p * min_overlap))
        overlap = (steps * p - n) / (steps - 1)
        out.append([math.floor(s * (p - overlap) + 0.5) for s in range(steps)])
    return out


def front_back(missing):
    """split of a padding of `missing` cells: the larger half in front"""
    return missing - missing // 2, missing // 2


def gaussian_map(patch, dtype=torch.float64):
    """impulse at p // 2 filtered by a Gaussian of sigma p / 4 truncated at 4 sigma, zero outside the patch (mode 'constant')"""
    lines = []
    for p in patch:
        sigma = p / 4.0
        r = int(4.0 * sigma + 0.5)
        k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=torch.float64) / sigma) ** 2)
        k = k / k.sum()
        lines.append(torch.stack([k[i - p // 2 + r] if abs(i - p // 2) <= r else k.new_zeros(()) for i in range(p)]))
    m = lines[0][:, None, None] * lines[1][None, :, None] * lines[2][None, None, :]
    m[m == 0] = m[m != 0].min()
    return m.to(dtype)


def predict_all_patches(img, sd, patch, min_overlap=0.5, use_gaussian=True):
    """the reference's loop: per patch replicate-pad, forward, softmax, weight, crop, add; then normalise and softmax AGAIN"""
    B, _, D, H, W = img.shape
    K = sd["head.6.weight"].shape[0]
    out = torch.zeros(B, K, D, H, W, dtype=img.dtype)
    norm = torch.zeros(B, 1, D, H, W, dtype=img.dtype)
    g = gaussian_map(patch, img.dtype) if use_gaussian else torch.ones(patch, dtype=img.dtype)
    starts = patch_starts((D, H, W), min_overlap, patch)
    for z in starts[0]:
        for y in starts[1]:
            for x in starts[2]:
                part = img[:, :, z:z + patch[0], y:y + patch[1], x:x + patch[2]]
                n = part.shape[2:]
                fb = [front_back(p - m) for p, m in zip(patch, n)]
                padded = F.pad(part, [fb[2][0], fb[2][1], fb[1][0], fb[1][1], fb[0][0], fb[0][1]], mode="replicate")
                prob = torch.softmax(forward(padded, sd), dim=1) * g
                crop = (slice(None), slice(None)) + tuple(slice(f, f + m) for (f, _), m in zip(fb, n))
                region = (slice(None), slice(None), slice(z, z + n[0]), slice(y, y + n[1]), slice(x, x + n[2]))
                out[region] += prob[crop]
                norm[region] += g[None, None][crop]
    return torch.softmax(out / norm, dim=1)


def cnn_keypoint_mask(softmax_pred, mask):
    return (softmax_pred.argmax(1)[0] != 0) & mask
