"""Tuning aid: fused fp32 ConvNeXt MLP — the persistent kernel (default), the one-tile-per-workgroup kernel (KPF_MLP_V1=1) and the two
plain GEMM launches, interleaved in one process.

    python tools/mlp_bench.py                 # the three shapes of the headline workloads
    python tools/mlp_bench.py --sweep         # C = 96 and 128 over M = 4096 ... 1048576
    python tools/mlp_bench.py --cfg 1         # KPF_MLP_CFG for the persistent kernel (see kpf_convnext_mlp_f32)
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from keypointfusion_amd import engine as E, lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--cfg", default="", help="comma-separated KPF_MLP_CFG values to add as variants")
ap.add_argument("--no-plain", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
shapes = [(C, M) for C in (96, 128) for M in (4096, 16384, 65536, 262144, 1048576)] if args.sweep else [(96, 262144), (192, 65536), (128, 262144)]
for C, M in shapes:
    y = torch.randn(M, C, generator=g).to(dev); x = torch.randn(M, C, generator=g).to(dev)
    w1 = (torch.randn(4 * C, C, generator=g) / C ** 0.5).to(dev); b1 = torch.randn(4 * C, generator=g).to(dev)
    w2 = (torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5).to(dev); b2 = torch.randn(C, generator=g).to(dev); gam = torch.rand(C, generator=g).to(dev)
    out = torch.empty_like(x)

    def fused(env):
        def fn():
            for k in ("KPF_MLP_V1", "KPF_MLP_CFG"):  # read per call by the library
                os.environ.pop(k, None)
            os.environ.update(env)
            L.check(L.load().kpf_convnext_mlp_f32(E._ptr(y), E._ptr(x), E._ptr(w1), E._ptr(b1), E._ptr(w2), E._ptr(b2), E._ptr(gam), E._ptr(out), M, C, E._stream()))
        return fn

    pc1 = E.PackedConv(w1, b1, dev); pc2 = E.PackedConv(w2, b2, dev)
    ya = E.Act(y.view(-1), 1, 1, M, C); xa = E.Act(x.view(-1), 1, 1, M, C); h = E.Act.empty(1, 1, M, 4 * C, dev); oa = E.Act(out.view(-1), 1, 1, M, C)

    def plain():
        E.conv(pc1, ya, out=h, flags=L.KPF_ACT_GELU); E.conv(pc2, h, out=oa, gamma=gam, res=xa)

    variants = [("v1", fused({"KPF_MLP_V1": "1"}))]
    if C != 192:  # (192 runs the v1 kernel whatever the switch says)
        variants.append(("persistent", fused({})))
        variants += [("persistent cfg=%s" % c, fused({"KPF_MLP_CFG": c})) for c in args.cfg.split(",") if c]
    if not args.no_plain:
        variants.append(("plain", plain))
    times = {n: [] for n, _ in variants}
    for name, fn in variants:
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):  # interleaved rounds: every variant sees the same clock / thermal state
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters): fn()
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    for name, _ in variants:
        ms = statistics.median(times[name])
        print("C=%d M=%d %-18s median %.4f ms  min %.4f  max %.4f  %.1f TF" % (C, M, name, ms, min(times[name]), max(times[name]), 16.0 * M * C * C / ms / 1e9), flush=True)
