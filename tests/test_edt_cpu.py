"""CPU tests of the Euclidean distance transform port (csrc/edt.hip) and of the lung split on top of it: the oracle against
the definition, the restatement of the kernel's passes against the oracle, the scenes the GPU tests use, the plausibility rule
of process_lung_mask.py, the host-side argument checks of the Python layer and of the C ABI, and the refusal of CPU tensors."""
import warnings

import numpy as np
import pytest
import torch

import edt_oracle as eo
from fissure_segmentation_amd import functional as F
from fissure_segmentation_amd.data_processing import process_lung_mask as plm

BASE = (2, 19, 21, 70)          # the shape of the GPU tests
REL = 4.8e-7                    # four fp32 ulps: one rounding each in the product, the square and the two sums


@pytest.mark.parametrize("sampling", [None, (2.5, 1.0, 0.75), (0.7, 1.1, 2.3)])
def test_oracle_equals_the_definition(sampling):
    for seed, density in ((0, 0.5), (1, 0.05), (2, 0.01)):
        m = eo.random_sites((1, 5, 6, 7), density, seed)[0]
        np.testing.assert_allclose(eo.edt_sq(m, sampling), eo.brute_sq(m, sampling), rtol=1e-12, atol=0)
    assert np.isinf(eo.brute_sq(np.ones((2, 3, 4), bool))).all()


@pytest.mark.parametrize("density", [0.5, 0.02, 0.001])
def test_pass_restatement_int32_is_exact(density):
    m = eo.random_sites(BASE, density, 11)
    for b in range(BASE[0]):
        d2, idx = eo.passes(m[b])
        want = np.rint(eo.edt_sq(m[b])).astype(np.int64)
        assert d2.dtype == np.int32 and np.array_equal(d2, want)
        z, y, x = np.unravel_index(idx, m[b].shape)
        assert not m[b][z, y, x].any()                                         # the winner is a site ...
        g = np.indices(m[b].shape)
        assert np.array_equal((g[0] - z) ** 2 + (g[1] - y) ** 2 + (g[2] - x) ** 2, want)   # ... at the returned distance


@pytest.mark.parametrize("sampling", [(2.5, 1.0, 0.75), (0.7, 1.1, 2.3)])
@pytest.mark.parametrize("density", [0.5, 0.02, 0.001])
def test_pass_restatement_fp32_is_inside_the_bar(sampling, density):
    m = eo.random_sites(BASE, density, 12)
    s32 = tuple(float(np.float32(v)) for v in sampling)
    for b in range(BASE[0]):
        d2, _ = eo.passes(m[b], sampling)
        want = eo.edt_sq(m[b], s32)
        assert d2.dtype == np.float32 and np.array_equal(d2 == 0, want == 0)
        assert np.all(np.abs(d2.astype(np.float64) - want) <= REL * want)


def test_pass_restatement_ties_and_empty():
    m = np.ones((3, 5, 9), bool)
    d2, idx = eo.passes(m)
    assert (d2 == eo.INT_INF).all() and (idx == -1).all()
    d2, idx = eo.passes(m, (1.0, 2.0, 3.0))
    assert np.isinf(d2).all() and (idx == -1).all()
    m[1, 2, 2] = m[1, 2, 6] = False                  # x = 4 is two voxels from both: the lower index wins
    d2, idx = eo.passes(m)
    assert d2[1, 2, 4] == 4 and idx[1, 2, 4] == (1 * 5 + 2) * 9 + 2
    m = np.ones((3, 5, 9), bool)
    m[1, 1, 4] = m[1, 3, 4] = False                  # the same along H
    assert eo.passes(m)[1][1, 2, 4] == (1 * 5 + 1) * 9 + 4


def test_scenes_run_as_the_gpu_tests_describe_them():
    m = eo.lungs_bridged()
    assert eo.ndi.label(m, eo.ndi.generate_binary_structure(3, 1))[1] == 1
    out, radii, warn = eo.lung_split(m)
    assert radii == [3] and not warn
    assert np.array_equal(out != 0, m) and set(np.unique(out)) == {0, 1, 2}
    assert np.argwhere(out == 2)[:, 2].mean() < np.argwhere(out == 1)[:, 2].mean()       # smaller x is the right lung: 2
    m = eo.lungs_speck()
    out, radii, warn = eo.lung_split(m)
    assert radii == [] and warn and int((m & (out == 0)).sum()) == 5 and out[2, 3, 30:35].max() == 0
    with pytest.raises(ValueError, match="detached"):
        eo.lung_split(eo.one_ball())
    lab = eo.label_scene()
    assert set(np.unique(lab)) == {0, 1, 2, 7} and set(np.unique(eo.nearest_label(lab, (1, 2)))) == {1, 2}
    sym = eo.nearest_label(eo.label_scene_symmetric(), (1, 2))
    assert (sym[:, :, :33] == 1).all() and (sym[:, :, 33:] == 2).all()                  # the plane x = 32 goes to label 1
    a, b = eo.slabs()
    st = eo.labelmap_distances(a, b, (1.5, 1.0, 2.0))
    assert all(np.isfinite(v) and v > 0 for v in st) and st[0] < st[3] < st[2]


def test_check_left_right_lung_plausible(capsys):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert plm.check_left_right_lung_plausible([1000]) is False
        assert plm.check_left_right_lung_plausible([]) is False
        assert "only one component" in capsys.readouterr().out
        assert plm.check_left_right_lung_plausible([100, 1001]) is False
        assert "Implausible volume-ratio" in capsys.readouterr().out
        assert plm.check_left_right_lung_plausible([100, 1000]) is True          # a ratio of exactly 10 passes
        assert plm.check_left_right_lung_plausible([900, 1000]) is True
        assert plm.check_left_right_lung_plausible([900, 1000], max_volume_ratio=1.05) is False
    with pytest.warns(UserWarning, match="Found 3 connected components in lung mask, but expected 2"):
        assert plm.check_left_right_lung_plausible([5, 900, 1000]) is True
    assert "[1000, 900, 5]" in capsys.readouterr().out
    for sizes in ([1000], [100, 1001], [5, 900, 1000], [900, 1000]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert plm.check_left_right_lung_plausible(sizes) == eo.plausible(sizes)[0]


def test_cpu_tensors_are_refused():
    v = torch.zeros(4, 5, 6, dtype=torch.bool)
    lab = torch.zeros(4, 5, 6, dtype=torch.int32)
    for call in (lambda: F.distance_transform_edt(v), lambda: F.distance_transform_edt(v[None], sampling=(1, 2, 3)),
                 lambda: F.distance_transform_edt(v, return_indices=True), lambda: F.nearest_label(lab, (1, 2)),
                 lambda: F.labelmap_distances(v, v), lambda: plm.maybe_detach_mask(v),
                 lambda: plm.binary_lung_mask_to_left_right(v)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_argument_checks():
    big_dim = torch.zeros(1, dtype=torch.bool).expand(1, 2, 16385)
    big_vol = torch.zeros(1, dtype=torch.bool).expand(2048, 1024, 1024)
    for vol in (big_dim, big_vol, big_vol[None]):
        with pytest.raises(ValueError, match="16384 or 2\\^31"):
            F.distance_transform_edt(vol)
    with pytest.raises(ValueError, match="16384 or 2\\^31"):
        F.nearest_label(big_dim.to(torch.int32), (1, 2))
    v = torch.zeros(4, 5, 6, dtype=torch.bool)
    with pytest.raises(ValueError, match="bool or integer"):
        F.distance_transform_edt(v.float())
    with pytest.raises(ValueError, match="bool or integer"):
        F.distance_transform_edt(v[0])
    for bad in ((1, 2), (1, 0, 1), (1, -1, 1), (1, float("nan"), 1), (1, float("inf"), 1)):
        with pytest.raises(ValueError, match="sampling"):
            F.distance_transform_edt(v, sampling=bad)
    with pytest.raises(ValueError, match="at least one"):
        F.distance_transform_edt(v, return_distances=False)
    lab = torch.zeros(4, 5, 6, dtype=torch.int32)
    for bad in ((), (1, 1), tuple(range(65))):
        with pytest.raises(ValueError, match="candidates"):
            F.nearest_label(lab, bad)
    with pytest.raises(ValueError, match="integer label map"):
        F.nearest_label(lab[None], (1, 2))
    with pytest.raises(ValueError, match="one shape"):
        F.labelmap_distances(v, v[:3])
    with pytest.raises(ValueError, match="two different values"):
        plm.binary_lung_mask_to_left_right(v, 1, 1)
    with pytest.raises(ValueError, match="\\(D, H, W\\)"):
        plm.maybe_detach_mask(v[None])


def test_reference_alias():
    import sys

    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from data_processing.process_lung_mask import binary_lung_mask_to_left_right, check_left_right_lung_plausible
        assert binary_lung_mask_to_left_right is plm.binary_lung_mask_to_left_right
        assert check_left_right_lung_plausible is plm.check_left_right_lung_plausible
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]


def test_host_side_error_codes():
    """every argument check runs before anything is launched: the pointers are never followed"""
    from fissure_segmentation_amd import _lib
    lib = _lib.lib
    B, D, H, W = 2, 7, 8, 70
    V = D * H * W
    assert lib.fsg_edt_workspace_bytes(B, D, H, W, 0) >= 4 * B * V and lib.fsg_edt_workspace_bytes(B, D, H, W, 1) >= 8 * B * V
    assert lib.fsg_edt_workspace_bytes(B, 0, H, W, 0) == 0
    need, one = lib.fsg_edt_workspace_bytes(B, D, H, W, 1), 8
    assert lib.fsg_edt_sq_i32(one, B, D, H, 16385, one, None, one, 1 << 40, None) == 1 and b"16384" in lib.fsg_last_error()
    assert lib.fsg_edt_sq_i32(one, 1, 2048, 1024, 1024, one, None, one, 1 << 40, None) == 1 and b"2^31" in lib.fsg_last_error()
    assert lib.fsg_edt_sq_i32(one, B, D, H, W, one, one, one, need - 1, None) == 1 and b"workspace" in lib.fsg_last_error()
    assert lib.fsg_edt_sq_i32(one, B, D, H, W, one, None, None, need, None) == 1 and b"workspace" in lib.fsg_last_error()
    assert lib.fsg_edt_sq_i32(None, B, D, H, W, None, None, one, need, None) == 1 and b"NULL" in lib.fsg_last_error()
    assert lib.fsg_edt_sq_f32(one, B, D, H, W, 1.0, 0.0, 1.0, one, None, one, need, None) == 1 and b"spacing" in lib.fsg_last_error()
    assert lib.fsg_edt_sq_f32(one, B, D, H, W, 1.0, float("nan"), 1.0, one, None, one, need, None) == 1
    assert lib.fsg_edt_sq_f32(None, B, D, H, W, 1.0, 1.0, 1.0, None, None, one, need, None) == 1 and b"NULL" in lib.fsg_last_error()
    assert lib.fsg_edt_nearest_label(one, 0, 65, V, one, None, one, None) == 1 and b"K=65" in lib.fsg_last_error()
    assert lib.fsg_edt_nearest_label(one, 0, 2, 0, one, None, one, None) == 1
    assert lib.fsg_edt_nearest_label(None, 0, 2, V, None, None, None, None) == 1 and b"NULL" in lib.fsg_last_error()
