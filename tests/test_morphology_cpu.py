"""CPU tests of the ball morphology / connected components port (csrc/morphology.hip): the structuring element, the oracle's
own conventions (tests/morphology_oracle.py), the synthetic lung volume the GPU tests use, the host-side argument checks of
the Python layer and of the C ABI, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import morphology_oracle as mo
from fissure_segmentation_amd import functional as F
from fissure_segmentation_amd.data_processing import find_lobes as fl
from fissure_segmentation_amd.utils import image_ops


def test_ball_counts_and_offsets():
    assert [int(mo.ball(r).sum()) for r in (1, 2, 3, 4)] == [19, 81, 179, 389]
    for r in (0, 1, 2, 3, 4, 8, (1, 2, 3), (0, 0, 5), (8, 0, 3)):
        offs = F.ball_offsets(r)
        assert offs.dtype == torch.int64
        rz, ry, rx = mo.radius3(r)
        want = np.argwhere(mo.ball(r)) - np.array([rz, ry, rx])
        assert np.array_equal(offs.numpy(), want), r            # the integer test and the fp64 one agree, in raster order
    assert len(F.ball_offsets((0, 0, 5))) == 11 and len(F.ball_offsets(0)) == 1


def test_oracle_numbers_components_in_raster_order_of_their_first_voxel():
    m = mo.random_mask((17, 19, 70), 0.45, 0)
    for conn, want in ((6, 458), (18, 3), (26, 2)):
        lab, n = mo.label(m, conn)
        assert n == want
        first = [int(np.flatnonzero(lab.ravel() == i)[0]) for i in range(1, n + 1)]
        assert first == sorted(first)


def test_oracle_shapes_used_by_the_gpu_tests():
    s = mo.serpentine()
    assert mo.label(s, 6)[1] == 1 and int(s.sum()) == 11134
    p = np.pad(s, 1)
    nb = sum(np.roll(p, sh, ax).astype(int) for ax in range(3) for sh in (1, -1))[1:-1, 1:-1, 1:-1]   # 6-neighbours in the path
    assert int((nb[s] > 2).sum()) == 0 and int((nb[s] == 1).sum()) == 2      # a path: two ends, no branch
    c = mo.checkerboard()
    assert mo.label(c, 6)[1] == c.size // 2 and mo.label(c, 18)[1] == 1
    t = mo.three_label_map()
    d = mo.multiple_objects_morphology(t, 2, "dilate")
    assert ((mo.dilate(t == 1, 2) & mo.dilate(t == 2, 2)).sum() > 0) and ((mo.dilate(t == 2, 2) & mo.dilate(t == 3, 2)).sum() > 0)
    assert set(np.unique(d)) == {0, 1, 2, 3}
    e = mo.multiple_objects_morphology(t, 2, "erode")
    assert np.all(e[12] == 0) and (e == 2).sum() > 0


def test_closing_and_opening_conventions():
    a = np.zeros((6, 7, 9), bool)
    a[0, 0, 0] = True
    assert np.array_equal(mo.closing(a, 2), a)                 # a corner voxel survives: the dilation is known outside
    assert not mo.opening(np.ones((6, 7, 9), bool), 4).any()   # the volume is thinner than the ball on the zero-extended grid
    assert mo.opening(np.ones((12, 12, 12), bool), 4).sum() > 0
    m = mo.random_mask((9, 10, 11), 0.3, 1)
    assert np.all(mo.closing(m, 1) >= m) and np.all(mo.opening(m, 1) <= m)
    assert np.array_equal(mo.erode(m, (1, 2, 3), 1), ~mo.dilate(~m, (1, 2, 3), 0))


def test_synthetic_lung_volume():
    lung, fis = mo.lung_volume()
    assert lung.shape == (72, 56, 112) and set(np.unique(fis)) == {0, 1, 2, 3}
    not_lobes = mo.dilate(mo.closing(~mo.erode(lung, 2, 1) | (fis != 0), 2), 2, 0)
    lab, n = mo.label(mo.opening(~not_lobes, 4), 6)
    sizes, sums = mo.stats(lab, n)
    assert n == 5 and sorted(sizes.tolist()) == sorted([6923, 18425, 19638, 18425, 4192])
    assert len(set(sizes.tolist())) == 4                          # a size tie: the tie rule decides the order
    order = mo.size_order(sizes)
    assert sizes[order].tolist() == [19638, 18425, 18425, 6923, 4192] and order[1] < order[2]
    lobes, ok = mo.find_lobes(fis, lung)
    assert ok and lobes.dtype == np.int64 and set(np.unique(lobes)) == {0, 1, 2, 3, 4, 5}
    cx = [np.argwhere(lobes == l)[:, 2].mean() for l in range(1, 6)]
    cz = [np.argwhere(lobes == l)[:, 0].mean() for l in range(1, 6)]
    assert max(cx[0], cx[1], cx[4]) < min(cx[2], cx[3])           # 1, 2, 5 right (smaller x), 3, 4 left
    assert cz[0] < cz[4] < cz[1] and cz[2] < cz[3]
    lobes4, ok4 = mo.find_lobes(fis, lung, exclude_rhf=True)
    assert ok4 and sorted(np.bincount(lobes4.ravel())[1:].tolist()) == sorted([6923, 18425, 30895, 18425])
    cx = [np.argwhere(lobes4 == l)[:, 2].mean() for l in range(1, 5)]
    cz = [np.argwhere(lobes4 == l)[:, 0].mean() for l in range(1, 5)]
    assert max(cx[0], cx[1]) < min(cx[2], cx[3])                  # 1, 2 right (smaller x), 3, 4 left
    assert cz[0] < cz[1] and cz[2] < cz[3]
    assert mo.lobe_numbering_holds(lobes) and mo.lobe_numbering_holds(lobes4, exclude_rhf=True)
    assert not mo.lobe_numbering_holds(lobes[::-1]) and not mo.lobe_numbering_holds(lobes4[:, :, ::-1], exclude_rhf=True)
    comp, ok0 = mo.find_lobes(np.zeros_like(fis), lung)
    assert not ok0 and comp.dtype == np.int32 and comp.max() == 2


def test_six_component_lung_volume():
    """more components than lobes: the smallest is dropped, with and without the right horizontal fissure"""
    lung, fis = mo.lung_volume_six()
    not_lobes = mo.dilate(mo.closing(~mo.erode(lung, 2, 1) | (fis != 0), 2), 2, 0)
    lab, n = mo.label(mo.opening(~not_lobes, 4), 6)
    assert n == 6 and mo.stats(lab, n)[0].tolist() == [6923, 1545, 9434, 19638, 18425, 4192]
    lobes, ok = mo.find_lobes(fis, lung)
    assert ok and mo.lobe_numbering_holds(lobes)
    assert np.bincount(lobes.ravel())[1:].tolist() == [6923, 4192, 9434, 18425, 19638]
    lobes4, ok4 = mo.find_lobes(fis, lung, exclude_rhf=True)
    assert ok4 and mo.lobe_numbering_holds(lobes4, exclude_rhf=True)
    assert np.bincount(lobes4.ravel())[1:].tolist() == [6923, 30895, 9434, 18425]


def test_relabel_by_size_oracle():
    lab = np.array([[[1, 1, 2, 3, 3, 0, 4, 4, 4]]], np.int32)
    assert mo.relabel_by_size(lab, 4).tolist() == [[[2, 2, 4, 3, 3, 0, 1, 1, 1]]]


def test_python_argument_checks():
    v = torch.zeros(4, 5, 6, dtype=torch.bool)
    for bad in (-1, 9, (1, 2), (1, 2, 9), 1.5, (1, 2, 3.0)):
        with pytest.raises(ValueError, match="radius"):
            F.binary_dilate(v, bad)
    with pytest.raises(ValueError, match="radius"):
        F.ball_offsets(9)
    with pytest.raises(ValueError, match="border"):
        F.binary_erode(v, 1, border=2)
    for bad in (4, 8, 27, None):
        with pytest.raises(ValueError, match="connectivity"):
            F.connected_components(v, bad)
    with pytest.raises(ValueError, match="bool or integer"):
        F.binary_closing(v.float(), 1)
    with pytest.raises(ValueError, match="bool or integer"):
        F.binary_opening(torch.zeros(5, 6, dtype=torch.bool), 1)
    with pytest.raises(ValueError, match="int32 labels"):
        F.component_stats(torch.zeros(4, 5, 6, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match="morphology operation"):
        image_ops.multiple_objects_morphology(torch.zeros(4, 5, 6, dtype=torch.uint8), 2, "close")
    with pytest.raises(ValueError, match="one"):
        fl.find_lobes(torch.zeros(4, 5, 6, dtype=torch.uint8), torch.zeros(4, 5, 7, dtype=torch.uint8))


def test_cpu_tensors_are_refused():
    v = torch.zeros(4, 5, 6, dtype=torch.bool)
    lab = torch.zeros(4, 5, 6, dtype=torch.int32)
    for call in (lambda: F.binary_dilate(v, 1), lambda: F.binary_erode(v, 1), lambda: F.binary_closing(v, 2),
                 lambda: F.binary_opening(v, 4), lambda: F.connected_components(v), lambda: F.component_stats(lab, 3),
                 lambda: F.relabel_by_size(lab, 3), lambda: fl.find_lobes(v.to(torch.uint8), v),
                 lambda: image_ops.multiple_objects_morphology(v.to(torch.uint8), 2, "dilate")):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_reference_alias():
    import sys

    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from utils.image_ops import multiple_objects_morphology
        from data_processing.find_lobes import find_lobes
        assert multiple_objects_morphology is image_ops.multiple_objects_morphology and find_lobes is fl.find_lobes
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]


def test_host_side_error_codes():
    """every argument check runs before anything is launched: NULL volumes cannot be reached"""
    from fissure_segmentation_amd import _lib
    lib = _lib.lib
    B, D, H, W = 2, 7, 8, 70
    need = lib.fsg_cc_workspace_bytes(B, D, H, W)
    assert need >= 4 * B * D * H * W and lib.fsg_cc_workspace_bytes(B, 0, H, W) == 0
    one = 8   # a non-NULL pointer value that is never followed
    assert lib.fsg_ball_dilate_bits(one, B, D, H, W, 9, 1, 1, 0, 0, 0, one + 8, None) == 1 and b"radius" in lib.fsg_last_error()
    assert lib.fsg_ball_dilate_bits(one, B, D, H, W, 1, -1, 1, 0, 0, 0, one + 8, None) == 1
    assert lib.fsg_ball_dilate_bits(one, B, D, H, W, 1, 1, 1, 2, 0, 0, one + 8, None) == 1 and b"border" in lib.fsg_last_error()
    assert lib.fsg_ball_dilate_bits(None, B, D, H, W, 1, 1, 1, 0, 0, 0, None, None) == 1 and b"NULL" in lib.fsg_last_error()
    assert lib.fsg_ball_dilate_bits(one, B, D, H, W, 1, 1, 1, 0, 0, 0, one, None) == 1      # in place
    assert lib.fsg_ball_dilate_bits(one, B, 0, H, W, 1, 1, 1, 0, 0, 0, one + 8, None) == 1 and b"shape" in lib.fsg_last_error()
    assert lib.fsg_ball_dilate_bits(one, 1, 2048, 1024, 1024, 1, 1, 1, 0, 0, 0, one + 8, None) == 1 and b"2^31" in lib.fsg_last_error()
    assert lib.fsg_cc_label_bits(one, B, D, H, W, 8, one, one, one, need, None) == 1 and b"connectivity" in lib.fsg_last_error()
    assert lib.fsg_cc_label_bits(one, B, D, H, W, 6, one, one, one, need - 1, None) == 1 and b"workspace" in lib.fsg_last_error()
    assert lib.fsg_cc_label_bits(None, B, D, H, W, 6, None, None, one, need, None) == 1 and b"NULL" in lib.fsg_last_error()
    assert lib.fsg_bits_pack_u8(None, B, D, H, W, -1, None, None) == 1 and b"NULL" in lib.fsg_last_error()
    assert lib.fsg_bits_pack_u8(one, B, D, H, W, 256, one, None) == 1
    assert lib.fsg_bits_unpack_u8(None, B, D, H, W, None, None) == 1
    assert lib.fsg_bits_window(one, B, D, H, W, 0, 0, 0, D, H, 0, one + 8, None) == 1
    assert lib.fsg_component_stats_i32(one, B, D, H, W, 0, one, None) == 1 and b"cap" in lib.fsg_last_error()
    assert lib.fsg_relabel_lut_i32(one, B, D * H * W, one, 0, one, 0, None) == 1
