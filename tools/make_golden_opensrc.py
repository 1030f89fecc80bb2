"""Generate tests/golden/open_*.npz by running the REAL reference's upstream DGCNN and PointNet (models/dgcnn_opensrc.py).

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU with torch alone.
Written in the format of the other fixtures: seeds, outputs, grad_x, per-parameter gradient norm/head, the BatchNorm
running statistics after the step, the state_dict keys.  No reference source text is written.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_opensrc.py
"""
import os
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

# (name, seed, input channels, points, k, emb_dims, static, train)    all with B = 2, dropout = 0, 5 outputs
DGCNN_CASES = [("open_dynamic", 801, 3, 1024, 20, 128, False, True),
               ("open_static", 802, 6, 512, 16, 128, True, True),
               ("open_fallback_train", 803, 3, 512, 8, 96, False, True),
               ("open_fallback_eval", 804, 3, 512, 8, 96, False, False),
               ("open_eval", 805, 3, 1024, 20, 128, False, False)]
# (name, seed, points, emb_dims, train)
POINTNET_CASES = [("open_pointnet_eval", 811, 256, 128, False), ("open_pointnet_train", 812, 256, 128, True)]
OUT_CHANNELS = 5


def dgcnn_args(k, emb, static):
    return SimpleNamespace(k=k, emb_dims=emb, dropout=0., static=static)


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import import_reference
    import numpy as np
    import torch
    from golden_util import GOLDEN_DIR, cloud, fill_state_dict
    import_reference()
    import models.dgcnn_opensrc as r_open

    torch.manual_seed(0)
    torch.set_num_threads(8)

    def step(net, x, gseed):
        xt = torch.from_numpy(x).requires_grad_(True)
        y = net(xt)
        g = np.random.default_rng(gseed).standard_normal(tuple(y.shape)).astype(np.float32)
        y.backward(torch.from_numpy(g))
        out = {"out": y.detach().numpy(), "grad_x": xt.grad.numpy(), "keys": np.array(list(net.state_dict().keys()))}
        for n, p in net.named_parameters():
            gr = p.grad.reshape(-1)
            out["gnorm_" + n] = np.float64(gr.double().norm().item())
            out["ghead_" + n] = gr[:16].numpy().copy()
        for n, b in net.named_buffers():
            if "running" in n:
                out["buf_" + n] = b.numpy().copy()
        return out

    def save(name, **arrs):
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **arrs)
        print("wrote", name, len(arrs), "arrays", os.path.getsize(path), "bytes")

    for name, seed, cin, n_pts, k, emb, static, train in DGCNN_CASES:
        net = fill_state_dict(r_open.DGCNN(dgcnn_args(k, emb, static), cin, OUT_CHANNELS), seed).train(train)
        res = step(net, cloud(seed + 1000, 2, cin, n_pts), seed + 2000)
        save(name, seed=seed, cin=cin, N=n_pts, k=k, emb=emb, static=int(static), train=int(train), **res)

    for name, seed, n_pts, emb, train in POINTNET_CASES:
        net = fill_state_dict(r_open.PointNet(SimpleNamespace(emb_dims=emb, dropout=0.), OUT_CHANNELS), seed).train(train)
        res = step(net, cloud(seed + 1000, 2, 3, n_pts), seed + 2000)
        save(name, seed=seed, N=n_pts, emb=emb, train=int(train), **res)


if __name__ == "__main__":
    main()
