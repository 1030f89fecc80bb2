"""DPSRNet on the GPU (models/dpsr_net.py): compute_psr_grid against DPSR on the oracle's normals, the batched groups of
generate_meshes against the per-group path (the check of the NaN padding and of `lengths`), the meshes, one training step with
DPSRLoss and predict_full_pointcloud.  Grids are compared under the project's bar (dpsr_oracle.bar) with magnitude 0.5, the
range of DPSR's scale step.  The labels come from a stub in place of `seg_net` that returns fixed logits, so nothing depends on
training.  Figures are printed as NORMALS_PARITY lines."""
import numpy as np
import pytest
import torch

import dpsr_oracle as do
import normals_oracle as no

pytestmark = pytest.mark.gpu
RES = (32, 32, 32)
SIG = 2.0
B, N, C = 2, 256, 3
PER_LABEL = 100
CENTRES = {1: (-0.35, 0.05, 0.0), 2: (0.4, -0.1, 0.1)}
AXES = (0.3, 0.25, 0.2)


def _dev():
    return torch.device("cuda:0")


def _case(starved=True):
    """coords (B, 3, N) fp32 and labels (B, N): label 1 on one ellipsoid, label 2 on a second, shifted one, the rest background
    scattered in the cube, all shuffled.  With `starved`, item 1 has only two points of label 2 (the others turn background)."""
    rng = np.random.default_rng(40)
    coords, labels = [], []
    for b in range(B):
        parts = [no.ellipsoid(PER_LABEL, 0.003, seed=41 + 2 * b + lb, axes=AXES, centre=CENTRES[lb]) for lb in (1, 2)]
        bg = rng.uniform(-0.9, 0.9, (N - 2 * PER_LABEL, 3)).astype(np.float32)
        lab = np.concatenate([np.full(PER_LABEL, 1), np.full(PER_LABEL, 2), np.zeros(len(bg), np.int64)])
        if starved and b == 1:
            lab[PER_LABEL + 2:2 * PER_LABEL] = 0
        order = rng.permutation(N)
        coords.append(np.concatenate(parts + [bg])[order].T)
        labels.append(lab[order])
    return np.stack(coords).astype(np.float32), np.stack(labels)


class _FixedLogits(torch.nn.Module):
    """stands in for seg_net: the logits that make `labels` the argmax, whatever the input"""

    def __init__(self, labels, num_classes):
        super().__init__()
        self.num_classes = num_classes
        self.register_buffer("logits", 10.0 * torch.nn.functional.one_hot(torch.from_numpy(labels), num_classes).permute(0, 2, 1).float())

    def forward(self, x):
        return self.logits[:x.shape[0]]


class _Anchored(torch.nn.Module):
    """a real segmentation network whose argmax is pinned: fixed logits plus a small multiple of the network's own"""

    def __init__(self, net, labels, num_classes):
        super().__init__()
        self.net, self.fixed, self.num_classes = net, _FixedLogits(labels, num_classes), num_classes

    def forward(self, x):
        return self.fixed(x) + 1e-3 * self.net(x)


def _net():
    from fissure_segmentation_amd.models.dpsr_net import DPSRNet
    torch.manual_seed(0)
    return DPSRNet("DGCNN", k=8, in_features=3, num_classes=C, dpsr_res=RES, dpsr_sigma=SIG).to(_dev())


def _oracle_grid(pts):
    """pts (n, 3) fp32 numpy -> (phi64, phi32) of DPSR on the oracle's normals (k = min(30, n - 1)), through the torch
    restatement of tests/dpsr_oracle.py; the inputs must leave no sign of a normal to a borderline projection"""
    k = min(30, len(pts) - 1)
    o64, o32 = no.frames(pts, k), no.frames(pts, k, dtype=np.float32)
    assert (o64["margin"] > 2).all() and (o64["gap"] >= 0.05).all(), "the test's cloud has an ill-defined normal"
    V = torch.from_numpy(pts)[None]
    phi64 = do.dpsr(V.double(), torch.from_numpy(o64["normals"])[None], RES, SIG)
    phi32 = do.dpsr(V, torch.from_numpy(o32["normals"])[None], RES, SIG)
    return phi64[0], phi32[0]


def _group(coords, labels, b, lb):
    return np.ascontiguousarray(coords[b].T[labels[b] == lb])


@pytest.fixture(scope="module")
def case():
    coords, labels = _case()
    oracle = {(b, lb): _oracle_grid(_group(coords, labels, b, lb)) for b, lb in ((0, 1), (0, 2), (1, 1))}
    return coords, labels, oracle


def test_compute_psr_grid_equals_dpsr_on_oracle_normals(case):
    coords, labels, oracle = case
    net = _net()
    pts = _group(coords, labels, 0, 1)
    got = net.compute_psr_grid(torch.from_numpy(pts)[None].to(_dev()))
    assert got.shape == (1,) + RES and got.dtype == torch.float32
    ok, msg = do.bar("NORMALS_PARITY", "compute_psr_grid", got[0], *oracle[0, 1], 0.5)
    assert ok, msg
    with pytest.raises(ValueError, match="neighborhood_size"):
        net.compute_psr_grid(torch.zeros(1, 2, 3, device=_dev()))


def test_batched_groups_equal_the_per_group_path(case):
    coords, labels, oracle = case
    net = _net()
    net.seg_net = _FixedLogits(labels, C).to(_dev())
    x = torch.from_numpy(coords).to(_dev())
    grids, counts = net._group_psr_grids(x, net.seg_net(x))
    assert grids.shape == (B * (C - 1),) + RES and counts.tolist() == [PER_LABEL, PER_LABEL, PER_LABEL, 2]
    for (b, lb), (phi64, phi32) in oracle.items():
        g = b * (C - 1) + lb - 1
        alone = net.compute_psr_grid(torch.from_numpy(_group(coords, labels, b, lb))[None].to(_dev()))[0]
        print(f"NORMALS_PARITY group ({b}, {lb}): batched - alone {float((grids[g] - alone).abs().max()):.3e}")
        for label, got in (("batched", grids[g]), ("alone", alone)):
            ok, msg = do.bar("NORMALS_PARITY", f"group ({b}, {lb}) {label}", got, phi64, phi32, 0.5)
            assert ok, msg
    assert bool((grids[3] == 1).all())                        # two points: no surface, the constant positive field
    assert bool(torch.isfinite(grids).all())


def test_meshes(case):
    coords, labels, _ = case
    net = _net()
    net.seg_net = _FixedLogits(labels, C).to(_dev())
    x = torch.from_numpy(coords).to(_dev())
    meshes = net.generate_meshes(x, net.seg_net(x))
    assert len(meshes) == B * (C - 1)
    nv = meshes.num_verts_per_mesh().tolist()
    assert min(nv[:3]) > 0 and nv[3] == 0 and meshes.faces_list()[3].shape == (0, 3)
    for g, (verts, faces) in enumerate(zip(meshes.verts_list(), meshes.faces_list())):
        assert bool(torch.isfinite(verts).all()) and (verts.numel() == 0 or float(verts.abs().max()) <= 1)
        if faces.numel():
            assert int(faces.min()) >= 0 and int(faces.max()) < verts.shape[0]
    # batch-major, label-minor: mesh g surrounds the cloud of group (g // 2, g % 2 + 1).  Vertex columns (x, y, z) run along the
    # grid's (last, middle, first) axis, the points' components (2, 1, 0)
    for g in range(3):
        b, lb = divmod(g, C - 1)
        centre = _group(coords, labels, b, lb + 1).mean(0)
        v = meshes.verts_list()[g].cpu().numpy()[:, ::-1]
        assert np.abs((v.max(0) + v.min(0)) / 2 - centre).max() < 0.1, (g, centre)
    # the starved group leaves the others as they are: item 0 alone gives the same first two meshes
    first = net.generate_meshes(x[:1], net.seg_net(x[:1]))
    assert len(first) == C - 1 and first.num_verts_per_mesh().tolist() == nv[:2]
    for a, b_ in zip(first.verts_list(), meshes.verts_list()[:2]):
        assert float((a - b_).abs().max()) <= 1e-4
    assert all(torch.equal(a, b_) for a, b_ in zip(first.faces_list(), meshes.faces_list()[:2]))


def test_one_training_step():
    from fissure_segmentation_amd.losses.dpsr_loss import DPSRLoss
    from fissure_segmentation_amd import functional as F
    from fissure_segmentation_amd.mesh import Meshes
    coords, labels = _case(starved=False)
    net = _net().train()
    net.seg_net = _Anchored(net.seg_net, labels, C).to(_dev())
    x = torch.from_numpy(coords).to(_dev())
    kept = x.clone()
    seg, meshes = net(x)
    assert torch.equal(x, kept)                               # the clamp works on a copy
    assert seg.shape == (B, C, N) and len(meshes) == B * (C - 1) and min(meshes.num_verts_per_mesh().tolist()) > 0
    assert not meshes.verts_packed().requires_grad            # the argmax loses the gradients, as in the reference
    z, y, xx = np.mgrid[:12, :12, :12].astype(np.float32)
    ball = torch.from_numpy(np.sqrt((xx - 5.5) ** 2 + (y - 5.5) ** 2 + (z - 5.5) ** 2) - 4)[None].to(_dev())
    v, f, n, _, _ = F.marching_cubes(ball)
    target = (torch.from_numpy(labels).to(_dev()), Meshes([v] * 4, [f] * 4, [n] * 4))
    loss, parts = DPSRLoss(None)((seg, meshes), target, current_epoch_fraction=0.5)
    assert float(parts["Chamfer"]) > 0
    loss.backward()
    assert bool(torch.isfinite(loss))
    total = 0.0
    for name, p in net.seg_net.net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        total += float(p.grad.abs().sum())
    assert total > 0


def test_predict_full_pointcloud():
    from fissure_segmentation_amd.mesh import Meshes
    coords, _ = _case(starved=False)
    net = _net().eval()
    pc = torch.from_numpy(coords).to(_dev())
    with torch.no_grad():
        seg, meshes = net.predict_full_pointcloud(pc, sample_points=128, n_runs_min=2)
    assert seg.shape == (B, C, N) and isinstance(meshes, Meshes) and len(meshes) == B * (C - 1)
    assert bool(torch.isfinite(meshes.verts_packed()).all())
