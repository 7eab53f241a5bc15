"""Tuning aid (GPU box; needs `make -C keypointfusion_amd/csrc dbg`): where a tile of the fused fp32 ConvNeXt MLP spends its time, for the
one-tile-per-workgroup kernel (KPF_MLP_V1=1) and the persistent one.  Per kernel: the in-kernel clock (shader cycles per 100-MHz tick),
mean prologue (tile start -> chunk loop), chunk loop and epilogue per tile in cycles and microseconds, the MFMA issue bound of the chunk
loop.  (Stamps of different workgroups are not compared: the shader clock is not one counter across the chip.)
usage: KPF_LIB_PATH=keypointfusion_amd/libkpf_hip_dbg.so python tools/mlp_tile_time.py"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from keypointfusion_amd import engine as E, lib as L
dev = torch.device("cuda:0")
lib = L.load()
lib.kpf_mlp_dbg_read.argtypes = [C.c_void_p, C.c_int]
g = torch.Generator().manual_seed(0)
for Cc, M in ((96, 262144), (128, 262144)):
    y = torch.randn(M, Cc, generator=g).to(dev); x = torch.randn(M, Cc, generator=g).to(dev)
    w1 = (torch.randn(4 * Cc, Cc, generator=g) / Cc ** 0.5).to(dev); b1 = torch.randn(4 * Cc, generator=g).to(dev)
    w2 = (torch.randn(Cc, 4 * Cc, generator=g) / (4 * Cc) ** 0.5).to(dev); b2 = torch.randn(Cc, generator=g).to(dev); gam = torch.rand(Cc, generator=g).to(dev)
    out = torch.empty_like(x)

    def run():
        L.check(lib.kpf_convnext_mlp_f32(E._ptr(y), E._ptr(x), E._ptr(w1), E._ptr(b1), E._ptr(w2), E._ptr(b2), E._ptr(gam), E._ptr(out), M, Cc, E._stream()))

    for name, v1 in (("v1", "1"), ("persistent", "0")):
        os.environ["KPF_MLP_V1"] = v1
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        lib.kpf_mlp_dbg_clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        n = 8 * 8192
        buf = (C.c_ulonglong * n)()
        assert lib.kpf_mlp_dbg_read(buf, n) == 0
        t = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8).astype(np.int64)
        t = t[(t[:, 0] > 0) & (t[:, 3] > t[:, 0])]
        clk = (t[:, 3] - t[:, 0]).sum() / max(1, (t[:, 5] - t[:, 4]).sum()) * 100.0  # MHz
        us = lambda cyc: cyc / clk  # noqa: E731
        pro, loop, epi = (t[:, 1] - t[:, 0]).mean(), (t[:, 2] - t[:, 1]).mean(), (t[:, 3] - t[:, 2]).mean()
        bound = 16.0 * 128 * Cc * Cc / 256  # 128-row tile: 2 GEMMs x 2 x 128 x C x 4C FLOP on four SIMDs at 64 FLOP/clk each
        print("C=%d M=%d %-10s %.1f us (with stamps) | tiles %d | clock %.0f MHz | per tile: prologue %.0f cyc %.2f us, chunk loop %.0f cyc %.2f us "
              "(MFMA issue bound %.0f cyc), epilogue %.0f cyc %.2f us, total %.2f us" % (
                  Cc, M, name, ms * 1e3, len(t), clk, pro, us(pro), loop, us(loop), bound, epi, us(epi), us(pro + loop + epi)), flush=True)
