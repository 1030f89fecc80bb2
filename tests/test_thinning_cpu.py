"""CPU tests of the thinning rule: the word formulation of csrc/thinning.hip restated in numpy (tests/thinning_oracle.py (b))
against the rule voxel by voxel (a), the rule's known properties with their outputs written out, and the host contract of
`functional.binary_thinning`, `poisson_reconstruction` and `binary_to_fissure_segmentation`."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import thinning_oracle as to


def _same(vol):
    a, pa = to.thin(vol)
    b, pb = to.thin_words(vol)
    assert np.array_equal(a, b)
    assert np.array_equal(pa, pb)
    return a, pa


# ------------------------------------------------------------------------------------------------ words == voxels
@pytest.mark.parametrize("shape", to.SHAPES)
def test_word_formulation_equals_the_rule(shape):
    _, pairs = _same(to.density_batch(shape))                     # densities 0.3, 0.6, 0.85, 1.0
    assert pairs.shape == (len(to.DENSITIES), shape[0])
    assert np.all(pairs[-1] == 0)                                 # the all-set slices are fixed points


def test_word_formulation_on_shapes():
    scene = to.shapes_scene()
    assert scene.shape == (3, 60, 150)
    assert scene[2, 0].any() and scene[2, -1].any() and scene[2, :, -1].any() and scene[1, :, 0].any()   # objects on the borders
    out, pairs = _same(scene)
    assert np.all(pairs >= 3) and out.any(axis=(1, 2)).all()


def test_word_formulation_on_blobs_and_mixed_batch():
    _same(to.blobs((3, 33, 130), 3))
    _same(to.mixed_batch())


def test_pack_words_layout():
    v = np.zeros((2, 130), bool)
    v[0, [0, 63, 64, 129]] = True
    w = to.pack_words(v)
    assert w.shape == (2, 3) and w.dtype == np.uint64
    assert [int(x) for x in w[0]] == [1 | (1 << 63), 1, 2] and not w[1].any()
    assert np.array_equal(to.unpack_words(w, 130), v)


# ------------------------------------------------------------------------------------------------ properties
def _one(img):
    out, pairs = _same(np.asarray(img, bool)[None])
    return out[0], int(pairs[0])


def test_small_blocks():
    img = np.zeros((8, 8), bool)
    img[2:4, 2:4] = True
    out, pairs = _one(img)
    assert not out.any() and pairs == 1                           # a 2 x 2 block vanishes
    img = np.zeros((8, 8), bool)
    img[2:5, 2:5] = True
    out, pairs = _one(img)
    want = np.zeros((8, 8), bool)
    want[3, 3] = True
    assert np.array_equal(out, want) and pairs == 1               # a 3 x 3 block leaves its centre


def test_disc_needs_twenty_pairs():
    out, pairs = _one(to.disc(64, 28))
    assert pairs == 20 and out.sum() == 1


@pytest.mark.parametrize("shape", [(1, 9), (9, 1), (5, 9), (1, 1)])
def test_full_slices_are_fixed_points(shape):
    out, pairs = _one(np.ones(shape, bool))                       # clamped borders: every neighbour of every voxel is set
    assert out.all() and pairs == 0


def test_diagonal_line_is_unchanged():
    img = np.zeros((20, 20), bool)
    img[np.arange(3, 17), np.arange(3, 17)] = True
    out, pairs = _one(img)
    assert np.array_equal(out, img) and pairs == 0


def test_idempotent_and_subset():
    for vol in (to.blobs((3, 33, 70), 11), to.random_field((3, 17, 65), 0.6, 12)):
        out, _ = to.thin(vol)
        assert not (out & ~vol).any()
        again, pairs = to.thin(out)
        assert np.array_equal(again, out) and not pairs.any()


def test_slices_do_not_interact():
    vol = to.blobs((4, 33, 70), 21)
    out, pairs = to.thin(vol)
    for z in (0, 2):
        alone, p = to.thin(vol[z:z + 1])
        assert np.array_equal(alone[0], out[z]) and p[0] == pairs[z]
    other = vol.copy()
    other[1] = ~other[1]
    assert np.array_equal(to.thin(other)[0][[0, 2, 3]], out[[0, 2, 3]])


def test_border_rule_matters():
    field = to.random_field((4, 33, 130), 0.6, 5)
    clamped, zero = to.thin(field)[0], to.thin(field, border="zero")[0]
    assert (clamped != zero).any()
    inner = (clamped != zero)[:, 3:-3, 3:-3]
    assert (clamped != zero).sum() > inner.sum()                  # and the difference starts at the border


# ------------------------------------------------------------------------------------------------ host contract
def test_symbols_exported_and_limit():
    from fissure_segmentation_amd import _lib
    assert hasattr(_lib.lib, "fsg_thin_bits") and "fsg_thin_bits" in _lib.SIGNATURES
    assert _lib.lib.fsg_thin_max_words() == _lib.THIN_MAX_WORDS
    assert _lib.THIN_MAX_WORDS >= 512 * (512 // 64)               # slices of 512 x 512 are served
    # the library refuses a larger slice and NULL planes before any launch (no GPU needed for that)
    null = ctypes.c_void_p(0)
    assert _lib.lib.fsg_thin_bits(null, 1, 1, _lib.THIN_MAX_WORDS + 1, 64, null, null, null) != 0
    assert b"words" in _lib.lib.fsg_last_error()
    assert _lib.lib.fsg_thin_bits(null, 1, 1, 4, 4, null, null, null) != 0


def test_binary_thinning_argument_rules():
    from fissure_segmentation_amd import functional as F
    with pytest.raises(RuntimeError, match="GPU only"):
        F.binary_thinning(torch.ones(2, 3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or integer"):
        F.binary_thinning(torch.ones(2, 3, 4))
    with pytest.raises(ValueError, match="empty"):
        F.binary_thinning(torch.ones(0, 3, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="bool or integer"):
        F.binary_thinning(torch.ones(3, 4, dtype=torch.uint8))


def test_poisson_reconstruction_lives_in_its_own_module():
    import fissure_segmentation_amd as fsg
    from fissure_segmentation_amd.data_processing import pointcloud_surface_fitting as pcf, surface_fitting as sf
    from fissure_segmentation_amd.data_processing import poisson_reconstruction as pr
    assert not hasattr(sf, "poisson_reconstruction") and not hasattr(pcf, "poisson_reconstruction")
    assert callable(pr.poisson_reconstruction)
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from data_processing.surface_fitting import o3d_mesh_to_labelmap, pointcloud_surface_fitting, poisson_reconstruction
        from utils.fissure_utils import binary_to_fissure_segmentation
        assert poisson_reconstruction.__module__ == "fissure_segmentation_amd.data_processing.poisson_reconstruction"
        assert pointcloud_surface_fitting.__module__ == "fissure_segmentation_amd.data_processing.pointcloud_surface_fitting"
        assert o3d_mesh_to_labelmap.__module__ == "fissure_segmentation_amd.data_processing.surface_fitting"
        assert binary_to_fissure_segmentation.__module__ == "fissure_segmentation_amd.utils.fissure_utils"
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
    with pytest.raises(RuntimeError, match="GPU only"):
        pr.poisson_reconstruction(torch.zeros(2, 3, 4, dtype=torch.int64), torch.ones(2, 3, 4, dtype=torch.bool), (1., 1., 1.))
    with pytest.raises(ValueError, match="integer label volume"):
        pr.poisson_reconstruction(torch.zeros(2, 3, 4), torch.ones(2, 3, 4, dtype=torch.bool), (1., 1., 1.))


def test_binary_to_fissure_segmentation_on_the_cpu():
    from fissure_segmentation_amd.utils.fissure_utils import binary_to_fissure_segmentation
    lung = torch.tensor([[[0, 1, 1, 2], [1, 1, 2, 2], [0, 0, 2, 2]],
                         [[1, 1, 0, 2], [1, 0, 0, 2], [1, 1, 2, 0]]])
    seg = torch.tensor([[[1, 1, 0, 1], [0, 1, 1, 0], [1, 0, 0, 1]],
                        [[1, 0, 1, 1], [0, 1, 0, 1], [1, 1, 1, 1]]])
    want = torch.tensor([[[0, 1, 0, 2], [0, 1, 2, 0], [0, 0, 0, 2]],
                         [[1, 0, 0, 2], [0, 0, 0, 2], [1, 1, 2, 0]]])
    out = binary_to_fissure_segmentation(seg, lung)
    assert out is seg and torch.equal(seg, want)                  # edited in place and returned
    with pytest.raises(ValueError, match="spacing"):
        binary_to_fissure_segmentation(seg.clone(), lung, resample_spacing=1.5)
    with pytest.raises(ValueError, match="lung mask"):
        binary_to_fissure_segmentation(seg.clone(), lung[:1])
