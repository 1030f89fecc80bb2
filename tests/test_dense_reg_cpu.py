"""CPU tests of the dense Adam registration (csrc/dense_reg.hip, functional.reg_smooth3 / reg_objective / reg_pack_features,
shape_model/adam_registration.py): properties of the oracle tests/reg_oracle.py that the GPU tests lean on, the packing, and
every refusal that happens on the host before a launch."""
import pytest
import torch

import reg_oracle as ro


def test_oracle_smoothing_is_self_adjoint():
    """<T a, b> = <a, T b> in fp64.  Tolerance: each side is a sum of n = 13 * 10 * 11 * 3 = 4290 products of magnitude
    |Ta| |b| <= max|a| max|b|; with entries ~ N(0, 1) the absolute rounding of one such fp64 sum, and of the 343-term sums
    inside T, is below n * 2^-53 * max|a| * max|b| -- the tolerance used is 4 n 2^-53 max|a| max|b| (two sums, two operators)."""
    g = torch.Generator().manual_seed(3)
    a = torch.randn(1, 3, 13, 10, 11, generator=g, dtype=torch.float64)
    b = torch.randn(1, 3, 13, 10, 11, generator=g, dtype=torch.float64)
    lhs, rhs = (ro.smooth3(a) * b).sum(), (a * ro.smooth3(b)).sum()
    tol = 4 * a.numel() * 2.0 ** -53 * float(a.abs().max()) * float(b.abs().max())
    print(f"adjoint: lhs {float(lhs):.17g} rhs {float(rhs):.17g} tol {tol:.3e}")
    assert abs(float(lhs - rhs)) <= tol
    assert abs(float(lhs)) > 1e3 * tol          # the agreement is not that of two zeros


def test_oracle_smoothing_is_not_the_truncated_seven_tap():
    """interior: the 7-tap [1 3 6 7 6 3 1] / 27; within two cells of a border the zero boundary after every pool removes walks"""
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 1, 13, 10, 11, generator=g, dtype=torch.float64) + 1
    s, t = ro.smooth3(x), ro.truncated7(x)
    inner = (slice(None), slice(None), slice(2, -2), slice(2, -2), slice(2, -2))
    assert float((s - t)[inner].abs().max()) < 1e-14
    edge = (s - t).abs()
    edge[inner] = 0
    assert float(edge.max()) > 1e-3 and bool((t[0, 0, 0] > s[0, 0, 0]).all())     # positive input: the truncated tap keeps more
    short = torch.ones(1, 1, 3, 3, 3, dtype=torch.float64)
    assert float((ro.smooth3(short) - ro.truncated7(short)).abs().max()) > 1e-2   # an axis shorter than the support


def test_oracle_gradient_matches_central_differences():
    """fp64, h = 1e-5, at nodes whose sample coordinate keeps 0.05 of a voxel from every integer (the trilinear gradient jumps
    there).  Inside a cell the objective is a quadratic in one entry, so the central difference has no truncation error and
    what remains is the rounding of the two objective values (of order 1) divided by 2 h: about 2^-52 / 2e-5 = 1e-11 absolute.
    The bound, 1e-7 of the largest gradient entry (entries are of order 1e-2 to 1e-1 here, so about 1e-9 absolute), leaves two
    orders of magnitude over that"""
    S, C, lam = (5, 6, 7), 5, .65
    g = torch.Generator().manual_seed(5)
    disp = (torch.rand(1, 3, *S, generator=g, dtype=torch.float64) * 2 - 1) * 2.5
    ff, fm = ro.half_features((1, C) + S, 6), ro.half_features((1, C) + S, 7)
    _, _, grad = ro.objective_with_grad(disp, ff, fm, lam, torch.float64)
    clear = ~ro.near_integer(disp, 0.05)
    picks = torch.nonzero(clear[0])[::7][:12]
    assert len(picks) >= 8
    h, worst = 1e-5, 0.0
    for i0, i1, i2 in picks.tolist():
        for ch in range(3):
            vals = []
            for sgn in (1, -1):
                d = disp.clone()
                d[0, ch, i0, i1, i2] += sgn * h
                c, r = ro.objective(d, ff, fm, lam)
                vals.append(float(c + r))
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - float(grad[0, ch, i0, i1, i2])))
    print(f"finite differences: worst {worst:.3e} of {float(grad.abs().max()):.3e}")
    assert worst <= 1e-7 * float(grad.abs().max())


def test_pack_features_pads_and_permutes():
    from fissure_segmentation_amd import functional as F_hip
    g = torch.Generator().manual_seed(8)
    for C, Cp in ((1, 8), (8, 8), (22, 24), (25, 32)):
        feat = torch.rand(2, C, 3, 4, 5, generator=g, dtype=torch.float64)
        packed = F_hip.reg_pack_features(feat)
        assert packed.dtype == torch.float16 and tuple(packed.shape) == (2, 3, 4, 5, Cp) and packed.is_contiguous()
        assert torch.equal(packed[..., :C], feat.permute(0, 2, 3, 4, 1).half())
        assert not bool(packed[..., C:].any())
    with pytest.raises(ValueError):
        F_hip.reg_pack_features(torch.zeros(3, 4, 5))
    with pytest.raises(ValueError):
        F_hip.reg_pack_features(torch.zeros(1, 2, 3, 4, 5, dtype=torch.int32))


def test_functions_refuse_bad_input_on_the_host():
    from fissure_segmentation_amd import functional as F_hip
    disp = torch.zeros(1, 3, 4, 5, 6)
    ff = F_hip.reg_pack_features(torch.rand(1, 5, 4, 5, 6))
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.reg_smooth3(disp)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.reg_objective(disp, ff, ff, .65, channels=5)
    for bad in (torch.zeros(1, 3, 2, 5, 6), torch.zeros(1, 3, 4, 5, 1), torch.zeros(3, 4, 5, 6), torch.zeros(1, 3, 4, 5, 6).long()):
        with pytest.raises(ValueError):
            F_hip.reg_smooth3(bad)
    with pytest.raises(ValueError, match=">= 3"):
        F_hip.reg_objective(torch.zeros(1, 3, 2, 5, 6), ff, ff, .65)
    with pytest.raises(ValueError):                                   # two channels: not a displacement field
        F_hip.reg_objective(torch.zeros(1, 2, 4, 5, 6), ff, ff, .65)
    with pytest.raises(ValueError, match="does not match"):           # another grid
        F_hip.reg_objective(torch.zeros(1, 3, 4, 5, 7), ff, ff, .65)
    with pytest.raises(ValueError, match="does not match"):           # another batch
        F_hip.reg_objective(torch.zeros(2, 3, 4, 5, 6), ff, ff, .65)
    with pytest.raises(ValueError, match="multiple of 8"):
        F_hip.reg_objective(disp, ff[..., :5].contiguous(), ff[..., :5].contiguous(), .65)
    with pytest.raises(ValueError, match="fp16"):
        F_hip.reg_objective(disp, ff.float(), ff.float(), .65)
    with pytest.raises(ValueError):                                   # fixed and moving of different widths
        F_hip.reg_objective(disp, ff, torch.cat([ff, ff], -1), .65)
    with pytest.raises(ValueError, match="channels"):
        F_hip.reg_objective(disp, ff, ff, .65, channels=9)


def test_library_refuses_bad_arguments_before_any_launch():
    from fissure_segmentation_amd import _lib
    assert _lib.lib.fsg_reg_objective_workspace_bytes(2, 13, 10, 11) == 2 * 6 * 16      # 1430 nodes = 6 workgroups of 256
    assert _lib.lib.fsg_reg_objective_workspace_bytes(1, 2048, 2048, 512) == 0          # 2^31 nodes
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_reg_smooth3_f32", None, 1, 3, 4, 4, 4, 16, None)
    with pytest.raises(RuntimeError, match="must differ"):
        _lib.call("fsg_reg_smooth3_f32", 16, 1, 3, 4, 4, 4, 16, None)
    with pytest.raises(RuntimeError, match=">= 3"):
        _lib.call("fsg_reg_smooth3_f32", 16, 1, 3, 4, 2, 4, 32, None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        _lib.call("fsg_reg_smooth3_f32", 16, 1, 3, 2048, 2048, 512, 32, None)
    ok = (1, 5, 8, 4, 4, 4, .65, 12.)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_reg_objective_f16", 16, 16, 16, *ok, 16, None, 16, 1 << 20, None)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _lib.call("fsg_reg_objective_f16", 16, 16, 16, 1, 5, 12, 4, 4, 4, .65, 12., 16, 16, 16, 1 << 20, None)
    with pytest.raises(RuntimeError, match="Cp"):
        _lib.call("fsg_reg_objective_f16", 16, 16, 16, 1, 9, 8, 4, 4, 4, .65, 12., 16, 16, 16, 1 << 20, None)
    with pytest.raises(RuntimeError, match=">= 3"):
        _lib.call("fsg_reg_objective_f16", 16, 16, 16, 1, 5, 8, 4, 4, 2, .65, 12., 16, 16, 16, 1 << 20, None)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("fsg_reg_objective_f16", 16, 24, 16, *ok, 16, 16, 16, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("fsg_reg_objective_f16", 16, 16, 16, *ok, 16, 16, 16, 8, None)


def test_module_refuses_bad_input_on_the_host():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.shape_model import adam_registration as ar
    assert ar.GRID_SP == 2
    ff = F_hip.reg_pack_features(torch.rand(1, 5, 4, 5, 6))
    with pytest.raises(RuntimeError, match="GPU only"):
        ar.adam_instance_optimisation(ff, ff, channels=5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ar.displacement_field(torch.zeros(1, 3, 4, 5, 6), (8, 10, 12))
    vol = torch.zeros(1, 1, 8, 10, 12)
    with pytest.raises(RuntimeError, match="GPU only"):
        ar.registration_features(vol, vol, vol, vol)
    small = F_hip.reg_pack_features(torch.rand(1, 5, 2, 5, 6))
    with pytest.raises(ValueError, match=">= 3"):
        ar.adam_instance_optimisation(small, small)
    with pytest.raises(ValueError, match="does not match"):
        ar.adam_instance_optimisation(ff, F_hip.reg_pack_features(torch.rand(1, 5, 4, 5, 7)))
    with pytest.raises(ValueError, match="multiple of 8"):
        ar.adam_instance_optimisation(ff[..., :5].contiguous(), ff[..., :5].contiguous())
    with pytest.raises(ValueError, match="affine_pre_reg"):
        ar.adam_instance_optimisation(ff, ff, affine_pre_reg=torch.eye(4))
    with pytest.raises(ValueError):
        ar.displacement_field(torch.zeros(1, 3, 4, 5, 6), (8, 10))
    with pytest.raises(ValueError):
        ar.displacement_field(torch.zeros(1, 2, 4, 5, 6), (8, 10, 12))
    with pytest.raises(ValueError):
        ar.registration_features(vol, vol[:, :, :4], vol, vol)
    with pytest.raises(ValueError, match=">= 6"):
        ar.registration_features(vol[:, :, :5], vol[:, :, :5], vol[:, :, :5], vol[:, :, :5])
