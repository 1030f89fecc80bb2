"""fwd+bwd(+Adam) timings of the other BASELINE configurations (sanity, not the headline)."""
import os, sys, time
import torch, torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fissure_segmentation_amd as fsg
from fissure_segmentation_amd.models.pointtransformer.seg_model import PointTransformerCompatibility
from fissure_segmentation_amd.models.folding_net import DGCNNFoldingNet
from fissure_segmentation_amd.models.dgcnn import DGCNNSeg
from fissure_segmentation_amd.losses.chamfer_loss import ChamferLoss
dev = torch.device("cuda:0")

GRAPH = "--graph" in sys.argv
if GRAPH: sys.argv.remove("--graph")

def run(name, net, x, lossfn, steps=10, warm=3, flat_adam=False):
    if flat_adam:
        from fissure_segmentation_amd.optim import FlatAdam
        opt = FlatAdam(net.parameters(), lr=1e-3, capturable=GRAPH)
    else:
        opt = torch.optim.Adam(net.parameters(), lr=1e-3, capturable=GRAPH, fused=True)
    def step():
        opt.zero_grad(set_to_none=True); l = lossfn(net(x)); l.backward(); opt.step(); return l
    if GRAPH:   # static shapes: capture fwd + loss + bwd + Adam once, replay
        name = name.replace("eager", "hipGraph replay")
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warm): step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        opt.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_l = step()
        def step():
            g.replay(); return static_l
    for _ in range(warm): step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps): l = step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    pts = x.shape[0] * x.shape[2]
    print(f"{name:55s} {1e3*dt:9.2f} ms/step  {pts/dt/1e6:7.3f} M points/s  loss {float(l):.4f}")

which = sys.argv[1:] or ["pt", "ae", "c4", "dgssm"]
torch.manual_seed(0)
if "pt" in which:
    for B in (8,):
        x = torch.rand(B, 3, 2048, device=dev) * 2 - 1; y = torch.randint(0, 4, (B, 2048), device=dev)
        run(f"C3 PointTransformer B={B} N=2048 in=3 (eager, fp32)", PointTransformerCompatibility(3, 4).to(dev).train(), x, lambda o: F.cross_entropy(o, y))
if "ae" in which:
    x = torch.rand(8, 3, 4096, device=dev) * 2 - 1
    net = DGCNNFoldingNet(k=20, n_embedding=512, shape_type="plane", n_input_points=4096, decode_mesh=True).to(dev).train()
    cl = ChamferLoss()
    run("C5 PC-AE FoldingNet + Chamfer B=8 N=4096 k=20 (eager)", net, x, lambda o: cl(o, x))
if "c4" in which:
    x = torch.rand(4, 3, 8192, device=dev) * 2 - 1; y = torch.randint(0, 4, (4, 8192), device=dev)
    run("C4 shape DGCNN-seg N=8192 k=40 B=4/GPU (eager, fp32)", DGCNNSeg(k=40, in_features=3, num_classes=4).to(dev).train(), x, lambda o: F.cross_entropy(o, y))
if "dgssm" in which:   # DG-SSM backbone at its defaults (cli/cli_args.py:15,80,81; dg_ssm.py:107-112)
    from types import SimpleNamespace
    from fissure_segmentation_amd.models.dgcnn_opensrc import DGCNN
    x = torch.rand(32, 3, 1024, device=dev) * 2 - 1; target = torch.randn(32, 12, device=dev)
    net = DGCNN(SimpleNamespace(k=20, emb_dims=1024, dropout=0., static=False), 3, 12).to(dev).train()
    run("DG-SSM upstream DGCNN B=32 N=1024 k=20 emb=1024 MSE (eager)", net, x, lambda o: F.mse_loss(o.squeeze(-1), target))
if "dgssm_full" in which:   # the whole DG-SSM step: backbone + three heads + fused decode/transform + DGSSMLoss + FlatAdam
    from fissure_segmentation_amd.losses.dgssm_loss import DGSSMLoss
    from fissure_segmentation_amd.models.dg_ssm import DGSSM
    B, P, M = 32, 2048, 20
    net = DGSSM(k=20, in_features=3, ssm_modes=M)
    evec = torch.linalg.qr(torch.randn(3 * P, M))[0]
    net.ssm.register_parameters_from_state_dict({"num_modes": torch.tensor(M), "percent_of_variance": torch.tensor(0.95),
                                                 "mean_shape": torch.rand(1, 3 * P) * 2 - 1,
                                                 "eigenvalues": 1.2 ** -torch.arange(M, dtype=torch.float32)[None], "eigenvectors": evec[None]})
    net = net.to(dev).train()
    x = torch.rand(B, 3, 1024, device=dev) * 2 - 1
    with torch.no_grad():
        tw = net.ssm.random_samples(B)
        target = (net.ssm.decode(tw), tw, torch.cat([0.1 * torch.randn(B, 6, device=dev), 1 - 0.1 * torch.rand(B, 3, device=dev)], 1))
    crit = DGSSMLoss()
    run(f"DG-SSM full step B={B} N=1024 k=20 P={P} M={M} DGSSMLoss FlatAdam (eager)", net, x, lambda o: crit(o, target)[0], flat_adam=True)
