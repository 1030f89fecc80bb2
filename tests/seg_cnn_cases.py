"""The cases that tests/test_seg_cnn_cpu.py and tests/test_seg_cnn_gpu.py share: shapes, seeds, inputs and the error bar."""
import functools

import torch

import seg_cnn_oracle as so

WEIGHT_SEED, NUM_CLASSES = 11, 3          # of the fixtures (tools/make_golden_seg_cnn.py)
FLOOR = 4.8e-7                            # 4 ulp of fp32 at the output's largest magnitude


def block_shape(i):
    """block 0: 11x8x14; the stride-2 block: 9x6x11 (odd extents: the output-size rule); stride-1 blocks: 5x6x9"""
    return (11, 8, 14) if i == 0 else ((9, 6, 11) if so.STRIDE[i] == 2 else (5, 6, 9))


# (name, block, spatial shape, batch): the eight configurations of MobileNet3D, then one stride-1 block where every voxel is
# border and one whose last axis spans more than two of the kernel's 4-voxel tiles (11 = 2 tiles + 3) with a second row of tiles
BLOCK_CASES = [(f"block{i}", i, block_shape(i), 2) for i in range(8)] + [("block2_1x1x1", 2, (1, 1, 1), 2), ("block7_long", 7, (3, 5, 11), 1)]


@functools.lru_cache(maxsize=None)
def state():
    return so.filled_state(NUM_CLASSES, WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def state64():
    return so.cast(state(), torch.float64)


@functools.lru_cache(maxsize=None)
def block_case(name):
    """-> (x fp64, block arguments fp64, keywords, y fp64, error of the oracle's own fp32 run, pre-activations)"""
    _, i, shape, B = next(c for c in BLOCK_CASES if c[0] == name)
    x = so.block_input(state(), i, shape, 100 + i, B=max(B, 2))[:B].float().double()     # values that fp32 holds exactly
    tensors, kw = so.block_args(state64(), i)
    pre = []
    y = so.mbconv(x, *tensors, **kw, pre=pre)
    t32, _ = so.block_args(state(), i)
    y32 = so.mbconv(x.float(), *t32, **kw)
    return x, tensors, kw, y, float((y32.double() - y).abs().max()), pre


def bar(err32, ref):
    """the project's usual bar: 4 x the error of the oracle's own fp32 run, at least 4.8e-7 of the largest magnitude"""
    return max(4.0 * err32, FLOOR * float(ref.abs().max()))


def fractions(p):
    return float((p < 0).double().mean()), float(((p >= 0) & (p <= 6)).double().mean()), float((p > 6).double().mean())


# ------------------------------------------------------------------ the keypoint case: 20x24x28, patches of 16
KP_SHAPE, KP_SEED, KP_PATCH, KP_INPUT_SCALE = (20, 24, 28), 31, (16, 16, 16), 3.0


@functools.lru_cache(maxsize=None)
def keypoint_case():
    """-> (img fp32 (1, 1, D, H, W), mask (D, H, W) bool, softmax fp64, softmax of the oracle's fp32 run)"""
    img = so.volume(KP_SEED, (1, 1, *KP_SHAPE), KP_INPUT_SCALE)
    g = torch.Generator().manual_seed(KP_SEED + 1)
    mask = torch.rand(KP_SHAPE, generator=g) < 0.7
    p64 = so.predict_all_patches(img.double(), state64(), KP_PATCH)
    p32 = so.predict_all_patches(img, state(), KP_PATCH)
    return img, mask, p64, p32


def ambiguous(softmax64, e):
    """(D, H, W) bool: voxels whose two largest scores lie within the error bar e of each other (each may move by e)"""
    top = softmax64[0].topk(2, dim=0).values
    return (top[0] - top[1]) <= 2 * e
