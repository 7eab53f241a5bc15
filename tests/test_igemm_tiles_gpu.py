"""Every tile configuration of the implicit GEMM (csrc/kpf_conv.hip: kpf_conv2d_f32, kpf_conv2d_h16) forced on small shapes through engine.FORCE_TILE /
engine16.FORCE_TILE16 and pinned to a float64 restatement of the same convolution.  The per-op cases of test_parity_gpu.py reach the 32 x 64 and 64 x 64 tiles
only (the cost model's choice at their sizes); the tiles the benchmark runs are pinned here.

Shapes.  B = 2, OH = 13, OW = 11: M = 286 pixels = one whole 256-row tile + 30 rows = eight whole 32-row tiles + 30.  N = 200 channels (264 in the 16-bit
family, whose widest tile is 256) at [32, 32 + N) of a wider pixel row: every tile width has a whole tile and a ragged one and the float4 path stays open; N = 105 with
out_ld = 105 closes it (every tile on the per-element path).  test_tile_tables_and_geometry (no GPU) holds the (BM, BN) tables and proves that
every tile has an interior, a ragged-M and a ragged-N workgroup on these shapes.

What is asserted, per variant (one float64 reference per variant, shared by its tiles):
 1. accuracy of the library's own tile choice.  fp32 and split operands: e_kernel <= 4 * e_plain + 8 * 2^-24 (test_fusion_head_kernels_gpu.py: both relative to
    max|ref64|, e_plain = the same restatement in fp32 torch on the CPU).  16-bit storage: the two bounds of igemm_bounds.h16_excess against float64 on the
    operands as stored; with KPF_ACT_GELU_SAVE the output is GELU of the pre-activation AS STORED (igemm_body: "gelu of the value as stored"), so its reference is
    gelu64 of the kernel's own second output, which in turn is held to the rounding bound.  KPF_MMA_BF16 / _F16: float64 products of the rounded operands, 2e-5
    of the range (test_head_mma_products_of_rounded_operands).
 2. every forced tile returns the BITS of the library's choice, or one of the documented refusals (REFUSALS), on exactly the tiles the dispatcher's code
    names: "Same k order in every tile shape: same bits" (kpf_conv2d_f32 / kpf_conv2d_h16).  gemm16_8ph_kernel (case 30) is held to 1 only; whether it is
    bit-equal to the igemm tiles is printed.
 3. canaries: outputs are finite; the guard row behind the last pixel, the columns outside [coff, coff + N), the pads of the residual and of the saved
    pre-activation keep their NaN bit pattern; the input's pad columns are NaN, so a kernel that read them would not stay finite.
 4. engine.AUTOTUNE returns the untuned bits, does not accumulate into an in-place residual and remembers one of its candidates.
One line per comparison ("ERR ..." for 1, "TILE ..." for 2); profiles/igemm_tile_errors.txt is one run on the MI355X."""
import functools
import math
import re
import zlib
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from igemm_bounds import PREC, h16_excess

FLOOR = 8 * 2.0 ** -24
CANARY = 0x7FC0BEEF                      # a quiet NaN with a payload (fp32)
CANARY16 = {"bf16": 0x7FC1, "f16": 0x7E01}  # quiet NaNs of the 16-bit types
B, OH, OW = 2, 13, 11
M = B * OH * OW

# (BM, BN) per configuration index of the switch in kpf_conv2d_f32 (tile_cfg - 1); 9-16: ring / one-stage forms for split operands (10, 11 retired to 0, 1)
F32_TILES = [(128, 128), (128, 96), (128, 64), (256, 48), (128, 112), (64, 128), (64, 64), (32, 64), (256, 128),
             (256, 128), (128, 128), (128, 96), (128, 64), (128, 128), (128, 96), (128, 64), (64, 64), (128, 192)]
F32_ARITH = [0, 1, 2, 3, 4, 5, 6, 7, 8, 17]   # what engine._autotune tries for fp32 arithmetic
F32_ROUNDED = {0, 2, 8}                       # launch_cfg: the tile shapes that have the ARITH_R_* kernels (KPF_MMA_BF16 / _F16)
# case of the switch in kpf_conv2d_h16 -> (BM, BN, LDS stages); 7 is its default; 30 is gemm16_8ph_kernel
H16_TILES = {0: (128, 128, 2), 1: (128, 96, 2), 2: (128, 64, 2), 5: (64, 128, 2), 6: (64, 64, 2), 7: (32, 64, 2), 8: (256, 128, 2), 20: (256, 128, 3),
             21: (128, 128, 3), 22: (128, 128, 4), 26: (256, 256, 2), 30: (256, 256, 2), 41: (64, 64, 4), 44: (32, 64, 8)}
H16_IGEMM = [c for c in H16_TILES if c != 30]
REFUSALS = ("KPF_ACT_GELU_SAVE needs fp32 arithmetic",                                   # launch_arith: outside fp32 two-stage
            "KPF_RES_GELU_GRAD needs a 1x1 stride-1 convolution in fp32 arithmetic",     # launch_arith
            "KPF_RES_GELU_GRAD needs a 1x1 stride-1 convolution on a two-stage tile",    # launch_arith_h16: the rings
            "split activations need in_ld, in_coff multiples of 32 and no operand prologue")


# ----------------------------------------------------------------------------------------------------------------------------------------
# without a GPU: the tables above are the switches', and the shapes reach all three output paths of every tile
# ----------------------------------------------------------------------------------------------------------------------------------------
def _switch(src, fn):
    """{case: (BM, BN, stages)} of the `switch (best)` that follows the definition of `fn` in the kernel source (default: case 7)."""
    body = src[src.index('extern "C" int %s(' % fn):]
    body = body[body.index("switch (best)"):]
    body = body[:body.index("\n}\n")]
    out = {}
    for ln in body.splitlines():
        m = re.match(r"\s*(case (\d+)|default):", ln)
        if not m:
            continue
        forms = re.findall(r"launch_cfg(?:_h16)?<(\d+), (\d+), (\d+), (\d+)(?:, (\d+))?>", ln)
        assert forms, ln
        shapes = {(16 * int(tm) * int(wm), 16 * int(tn) * int(wn)) for tm, tn, wm, wn, _ in forms}
        assert len(shapes) == 1, ln
        out[int(m.group(2)) if m.group(2) else 7] = shapes.pop() + (max(int(f[4] or 2) for f in forms),)
    return out


def test_tile_tables_and_geometry():
    from keypointfusion_amd import lib as L
    assert len(F32_TILES) == int(L.load().kpf_conv_num_tile_cfgs())
    src = (Path(L.__file__).parent / "csrc" / "kpf_conv.hip").read_text()
    f32 = _switch(src, "kpf_conv2d_f32")
    assert sorted(f32) == list(range(len(F32_TILES))) and all(f32[i][:2] == F32_TILES[i] for i in f32), f32
    h16 = _switch(src, "kpf_conv2d_h16")
    assert {**h16, 30: (256, 256, 2)} == H16_TILES, h16
    assert set(F32_ARITH) <= set(range(len(F32_TILES))) and F32_ROUNDED <= set(F32_ARITH)
    for (bm, bn), n in [(t, 200) for t in F32_TILES] + [(t[:2], 264) for t in H16_TILES.values()]:  # (the widths the aligned variants of each family run at)
        assert (M // bm) * (n // bn) >= 1 and M % bm and n % bn, (bm, bn, n)  # an interior tile, a ragged last row tile, a ragged last channel tile
        assert 256 % bm == 0                                                 # the (2, 16, 16) map: every pixel tile inside one image (NCHW transpose)
        assert 105 % bn                                                      # ... with the `n < N` tail
    assert 300 % 256 and 512 % 256 == 0 and 256 % 128 == 0                   # case 30's shape: accepted (N % 256, K % 128), ragged last pixel tile


# ----------------------------------------------------------------------------------------------------------------------------------------
# case builders (CPU only)
# ----------------------------------------------------------------------------------------------------------------------------------------
def to_split(t):
    """fp32 [..., C] -> same-shape fp32 tensor whose bytes are [32 x f16 hi | 32 x f16 lo] per 32-channel block (include/kpf.h)."""
    Cc = t.shape[-1]
    hi = t.half()
    lo = (t - hi.float()).half()
    return torch.stack([hi.reshape(-1, Cc // 32, 32), lo.reshape(-1, Cc // 32, 32)], 2).contiguous().view(torch.float32).reshape(t.shape)


def from_split(t):
    Cc = t.shape[-1]
    blk = t.contiguous().view(torch.float16).reshape(-1, Cc // 32, 2, 32).float()
    return (blk[:, :, 0] + blk[:, :, 1]).reshape(t.shape)


def _flag(name):
    from keypointfusion_amd import lib as L
    return getattr(L, name)


ONE_BY_ONE = ["lin", "relu", "leaky", "pro", "gelu", "gelu_save", "res", "res_gamma", "res_inplace", "res_relu", "ggrad"]
VARIANTS = ONE_BY_ONE + ["conv3", "conv3_res", "conv3_s2", "k1_short", "patch", "grouped", "u_lin", "u_gelu", "u_gelu_save", "u_res", "u_ggrad", "u_conv3",
                         "nchw_16x16", "nchw_13x11"]
SPLIT_VARIANTS = ["lin", "gelu", "res", "res_inplace", "pro", "out_split", "conv3", "u_lin", "u_res", "gelu_save", "ggrad"]


@functools.lru_cache(maxsize=None)
def _variant(fam, name, n_wide=200):
    """Operands (as the kernel is given them, fp32 tensors holding storage-precision values), launch settings and the float64 / plain-fp32 results."""
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%s/%d" % (fam, name, n_wide)).encode()))
    h16 = fam in PREC
    q = (lambda t: t.to(PREC[fam][0]).float()) if h16 else (lambda t: t)  # storage rounding
    v = SimpleNamespace(fam=fam, name=name, h16=h16, k=1, stride=1, pad=0, patch=False, G=1, flags=0, pro=None, gamma=None, res=None, inplace=False,
                        out2=False, nchw=False, out_split=False, H=OH, W=OW, OH=OH, OW=OW, cin=128 if h16 else 96, N=n_wide, out_coff=32, round_to=None)
    base = name[2:] if name.startswith("u_") else name
    if base.startswith("conv3"):
        v.k, v.pad, v.cin = 3, 1, 24 if h16 else (32 if "split" in fam else 20)
    if base == "conv3_s2":
        v.stride, v.H, v.W = 2, 26, 21
    if base == "k1_short":
        v.cin = 24 if h16 else 20
    if base == "patch":
        v.k, v.stride, v.patch, v.cin, v.H, v.W = 2, 2, True, 24, 26, 22
    if base == "grouped":
        v.G = 2
    if base.startswith("nchw"):
        v.nchw, v.N, v.out_coff = True, 105, 0
        if base == "nchw_16x16":
            v.H = v.W = v.OH = v.OW = 16
    if base == "out_split":
        v.out_split, v.N = True, 224  # (N, out_ld, out_coff multiples of 32)
    if name.startswith("u_"):
        v.N, v.out_coff = 105, 0
    v.M = B * v.OH * v.OW
    v.out_ld = v.G * v.N if (name.startswith("u_") or v.nchw) else v.out_coff + v.G * v.N + 32
    v.in_coff = 0 if v.patch else 32
    v.in_ld = v.G * v.cin + v.in_coff
    v.flags = {"relu": "KPF_ACT_RELU", "pro": "KPF_ACT_RELU", "leaky": "KPF_ACT_LEAKY", "gelu": "KPF_ACT_GELU", "gelu_save": "KPF_ACT_GELU", "out_split": "KPF_ACT_GELU",
               "res_relu": "KPF_RELU_AFTER_RES", "ggrad": "KPF_RES_GELU_GRAD", "nchw_16x16": "KPF_ACT_RELU", "mma_bf16": "KPF_MMA_BF16",
               "mma_f16": "KPF_MMA_F16"}.get(base, None)
    v.flags = _flag(v.flags) if v.flags else 0
    if base.startswith("mma_"):
        v.round_to = PREC[base[4:]][0]
    v.x = q(torch.randn(B, v.H, v.W, v.G * v.cin, generator=g))
    K = v.k * v.k * v.cin
    v.w = q(torch.randn(v.G * v.N, v.cin, v.k, v.k, generator=g) / K ** 0.5)
    v.bias = torch.randn(v.G * v.N, generator=g) * (0.1 if h16 else 1.0)
    if base == "pro":
        v.pro = (torch.rand(v.cin, generator=g) + 0.5, torch.randn(v.cin, generator=g) * 0.2)
    if base in ("res", "res_gamma", "res_inplace", "res_relu", "ggrad", "conv3_res"):
        v.res = q(torch.randn(B, v.OH, v.OW, v.G * v.N, generator=g))
        v.inplace = base == "res_inplace"
    if base == "res_gamma":
        v.gamma = torch.rand(v.N, generator=g) + 0.1
    v.out2 = base == "gelu_save"
    unaligned = name.startswith("u_")
    v.side_ld, v.side_coff = (v.G * v.N + 2, 1) if unaligned else (v.G * v.N + 16, 8)  # the residual / saved pre-activation live in a slice of their own
    if v.inplace:
        v.side_ld, v.side_coff = v.out_ld, v.out_coff
    if fam == "in_split":  # the operand is what the split rows hold: hi + lo, 22 bits
        v.x = from_split(to_split(v.x))
    v.ref, v.ref2 = _restate(v, torch.float64)
    v.plain, v.plain2 = _restate(v, torch.float32)
    assert bool(torch.isfinite(v.ref).all()) and float(v.ref.abs().max()) > 0.5
    if v.flags & (_flag("KPF_ACT_RELU") | _flag("KPF_ACT_LEAKY") | _flag("KPF_RELU_AFTER_RES")) or v.pro:
        z = v.ref2 if v.res is None else v.ref
        assert 0.2 < float((z > 0).double().mean()) < 0.9  # the activation has both of its branches to take
    return v


def _restate(v, dt):
    """-> (the output [B][OH][OW][G * N], the pre-activation acc + bias) in precision dt."""
    t = lambda a: a.to(dt)
    x, w, b = v.x, v.w, v.bias
    if v.round_to is not None:
        x, w = x.to(v.round_to).float(), w.to(v.round_to).float()
    x, w, b = t(x), t(w), t(b)
    if v.pro is not None:
        ps, pt = v.pro
        if dt == torch.float64:  # fmaf(x, s, t) of the kernel: one rounding to fp32 (the float64 sum of the exact product is that, up to double rounding)
            x = F.relu((x * ps.double() + pt.double()).float())
            x = (x.to(PREC[v.fam][0]) if v.h16 else x).double()  # (16 bits: the prologue rounds back to the storage type)
        else:
            x = F.relu(x * ps + pt)
            x = x.to(PREC[v.fam][0]).float() if v.h16 else x
    n, c = v.N, v.cin
    z = torch.cat([F.conv2d(x[..., i * c:(i + 1) * c].permute(0, 3, 1, 2), w[i * n:(i + 1) * n], b[i * n:(i + 1) * n], stride=v.stride, padding=v.pad)
                   for i in range(v.G)], 1).permute(0, 2, 3, 1).contiguous()
    assert z.shape == (B, v.OH, v.OW, v.G * n), z.shape
    fl, y = v.flags, z
    if fl & _flag("KPF_ACT_GELU"):
        y = F.gelu(z)
    if fl & _flag("KPF_ACT_RELU"):
        y = F.relu(z)
    if fl & _flag("KPF_ACT_LEAKY"):
        y = F.leaky_relu(z, 0.01)
    if v.res is not None:
        r = t(v.res)
        if fl & _flag("KPF_RES_GELU_GRAD"):  # d/dr [r Phi(r)] = Phi(r) + r phi(r)
            y = z * (0.5 * (1 + torch.erf(r / math.sqrt(2.0))) + r * torch.exp(-0.5 * r * r) / math.sqrt(2 * math.pi))
        else:
            y = (z * t(v.gamma).repeat(v.G) if v.gamma is not None else z) + r
            if fl & _flag("KPF_RELU_AFTER_RES"):
                y = F.relu(y)
    return y, z


# ----------------------------------------------------------------------------------------------------------------------------------------
# one launch through engine.conv / engine16.conv16 on canary-filled buffers
# ----------------------------------------------------------------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from keypointfusion_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _canary(dev, v, rows, ld):
    if v.h16:
        return torch.full((rows, ld), CANARY16[v.fam], dtype=torch.int16, device=dev).view(PREC[v.fam][0])
    return torch.full((rows, ld), CANARY, dtype=torch.int32, device=dev).view(torch.float32)


def _raw(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _kept(v, t):
    return bool((_raw(t) == (CANARY16[v.fam] if t.element_size() == 2 else CANARY)).all()) if t.numel() else True


def _bits(a, b):
    return torch.equal(_raw(a), _raw(b))


@functools.lru_cache(maxsize=None)
def _operand(fam, name, n_wide):
    """The packed operand on the device, built once per variant (every tile of a variant reads the same rows)."""
    from keypointfusion_amd.packs import Pack, PackedConv
    v = _variant(fam, name, n_wide)
    dev = _dev()
    mk = lambda w, b: PackedConv(w, b, dev, stride=v.stride, pad=v.pad, patchify=v.patch, prologue=None if v.pro is None else (v.pro[0].double(), v.pro[1].double()))
    if v.G == 1:
        pc = mk(v.w, v.bias)
    else:  # G operands of one shape, equally spaced (training.GroupedPack): x channel-stacked, weight and bias group-major, output channel-stacked
        parts = [mk(v.w[i * v.N:(i + 1) * v.N], None) for i in range(v.G)]
        if v.h16:
            big = torch.stack([p.as16(PREC[fam][0]).w for p in parts]).contiguous()
            pc = Pack(parts[0].geom, w16=big[0], b=v.bias.to(dev), groups=v.G, w_gstride=big[0].numel())
        else:
            big = torch.stack([p.w for p in parts]).contiguous()
            pc = Pack(parts[0].geom, w=big[0], b=v.bias.to(dev), groups=v.G, w_gstride=big[0].numel())
        pc.keep = big
    pc.split_allowed = fam == "w_split"
    return pc.as16(PREC[fam][0]) if v.h16 else pc


def _run(v, n_wide=200):
    """-> dict(out [M][G*N] (or the NCHW tensor), out2) on the CPU in the storage type, after the canary checks; raises lib.KpfError on a refusal."""
    from keypointfusion_amd import engine as E, engine16 as E16
    dev = _dev()
    op = _operand(v.fam, v.name, n_wide)
    st = lambda a: a.to(dev).to(PREC[v.fam][0]) if v.h16 else a.to(dev)
    rows_in = B * v.H * v.W
    xb = _canary(dev, v, rows_in, v.in_ld)  # pad columns are NaN: reading them does not stay unnoticed
    xs = v.x.reshape(rows_in, -1)
    xb[:, v.in_coff:] = st(to_split(xs) if v.fam == "in_split" else xs)
    xa = E.Act(xb.view(-1), B, v.H, v.W, v.cin, v.in_ld, v.in_coff, split=v.fam == "in_split")
    kw, side = dict(flags=v.flags), None
    if v.nchw:
        ob = torch.full((v.M * v.N + 64,), CANARY, dtype=torch.int32, device=dev).view(torch.float32)  # (fp32 planes also on the 16-bit path)
        kw["out_nchw"] = ob
    else:
        ob = _canary(dev, v, v.M + 1, v.out_ld)
        kw["out"] = E.Act(ob.view(-1), B, v.OH, v.OW, v.N, v.out_ld, v.out_coff)
    if v.res is not None or v.out2:
        side = ob if v.inplace else _canary(dev, v, v.M + 1, v.side_ld)
        if v.res is not None:
            side[:v.M, v.side_coff:v.side_coff + v.G * v.N] = st(v.res.reshape(v.M, -1))
        kw["out2" if v.out2 else "res"] = E.Act(side.view(-1), B, v.OH, v.OW, v.N, v.side_ld, v.side_coff)
    if v.gamma is not None:
        kw["gamma"] = v.gamma.to(dev)
    if v.out_split:
        kw["out_split"] = True
    if v.h16:
        E16.conv16(op, xa, E16.DTYPES[v.fam][1], **kw)
    else:
        E.conv(op, xa, **kw)
    torch.cuda.synchronize()
    got = {}
    if v.nchw:
        assert _kept(v, ob[v.M * v.N:]), "%s/%s: wrote behind the last plane" % (v.fam, v.name)
        got["out"] = ob[:v.M * v.N].view(B, v.N, v.OH, v.OW).cpu()
    else:
        lo, hi = v.out_coff, v.out_coff + v.G * v.N
        assert _kept(v, ob[v.M]) and _kept(v, ob[:v.M, :lo]) and _kept(v, ob[:v.M, hi:]), "%s/%s: wrote outside the output slice" % (v.fam, v.name)
        got["out"] = ob[:v.M, lo:hi].cpu()
    if side is not None and not v.inplace:
        lo, hi = v.side_coff, v.side_coff + v.G * v.N
        assert _kept(v, side[v.M]) and _kept(v, side[:v.M, :lo]) and _kept(v, side[:v.M, hi:]), "%s/%s: wrote outside the second slice" % (v.fam, v.name)
        if v.out2:
            got["out2"] = side[:v.M, lo:hi].cpu()
        else:
            assert _bits(side[:v.M, lo:hi].cpu(), st(v.res.reshape(v.M, -1)).cpu()), "%s/%s: the residual was written" % (v.fam, v.name)
    for k_, t in got.items():
        t = from_split(t) if (v.out_split and k_ == "out") else t
        assert bool(torch.isfinite(t.float()).all()), "%s/%s: %s is not finite" % (v.fam, v.name, k_)
    return got


def _nhwc(v, got):
    """the kernel's output as float64 [B][OH][OW][G*N], whatever its layout"""
    t = got.permute(0, 2, 3, 1) if v.nchw else (from_split(got) if v.out_split else got).view(B, v.OH, v.OW, -1)
    return t.double()


def _accuracy(v, got, problems, who="library"):
    """assertion 1 on one result; prints the ERR lines and appends what misses its bound to `problems`"""
    tag = "%s %s [%s] " % (v.fam, v.name, who)
    pairs = [("out", _nhwc(v, got["out"]), v.ref, v.plain)]
    if v.out2:
        z = got["out2"].view(B, v.OH, v.OW, -1).double()
        pairs.append(("out2", z, v.ref2, v.plain2))
        if v.h16:  # GELU of the pre-activation as stored
            pairs[0] = ("out", pairs[0][1], F.gelu(z), None)
    for what, g_, ref, plain in pairs:
        den = float(ref.abs().max())
        ek = float((g_ - ref).abs().max()) / den
        if v.h16:
            kind = "nchw" if v.nchw else ("gelu" if (what == "out" and v.flags & _flag("KPF_ACT_GELU")) else "rounding")
            excess, bound = h16_excess(g_, ref, PREC[v.fam][1], kind)
            ok = excess <= 0 if bound == "gelu" else excess < 0
            print("ERR %-44s e_kernel %.3e  bound %-8s excess %+.3e%s" % (tag + what, ek, bound, excess, "" if ok else "  MISSES"))
        elif v.round_to is not None:
            ok = ek < 2e-5
            print("ERR %-44s e_kernel %.3e  against products of rounded operands, bound 2e-5%s" % (tag + what, ek, "" if ok else "  MISSES"))
        else:
            ep = float((plain.double() - ref).abs().max()) / den
            ok = ek <= 4 * ep + FLOOR
            print("ERR %-44s e_kernel %.3e  e_plain %.3e  ratio to bound %.3f%s" % (tag + what, ek, ep, ek / (4 * ep + FLOOR), "" if ok else "  MISSES"))
        if not ok:
            problems.append("%s%s misses its bound (e_kernel %.3e)" % (tag, what, ek))


def _refused(e):
    text = str(e)
    hits = [r for r in REFUSALS if r in text]
    return hits[0] if hits else None


def _sweep(v, tiles, force, problems, expect_refusal=lambda c: False, n_wide=200):
    """assertions 1-3 for one variant: the library's choice against float64, then every forced tile against the library's bits"""
    from keypointfusion_amd import lib as L
    force(0)
    try:
        base = _run(v, n_wide)
    except L.KpfError as e:  # refused whatever the tile: every forced tile must refuse for the same documented reason
        why = _refused(e)
        print("TILE %-10s %-12s library    refused: %s" % (v.fam, v.name, why or str(e)))
        assert why and all(expect_refusal(c) for c in tiles), (v.fam, v.name, str(e))
        base = None
    else:
        _accuracy(v, base, problems)
    for c in tiles:
        force(c + 1)
        try:
            got = _run(v, n_wide)
        except L.KpfError as e:
            why = _refused(e)
            print("TILE %-10s %-12s cfg %-2d     refused: %s" % (v.fam, v.name, c, why or str(e)))
            if not (why and expect_refusal(c)):
                problems.append("%s/%s cfg %d: unexpected refusal: %s" % (v.fam, v.name, c, e))
            continue
        finally:
            force(0)
        if expect_refusal(c) or base is None:
            problems.append("%s/%s cfg %d: ran where a refusal is documented" % (v.fam, v.name, c))
            continue
        diff = [k_ for k_ in base if not _bits(base[k_], got[k_])]
        if diff:
            n_ = int((_raw(base[diff[0]]) != _raw(got[diff[0]])).sum())
            print("TILE %-10s %-12s cfg %-2d     DIFFERS in %s: %d of %d elements" % (v.fam, v.name, c, diff, n_, got[diff[0]].numel()))
            _accuracy(v, got, [], "cfg %d" % c)
            problems.append("%s/%s cfg %d: bits differ from the library's choice (%s, %d elements)" % (v.fam, v.name, c, diff, n_))
        else:
            print("TILE %-10s %-12s cfg %-2d     bits equal" % (v.fam, v.name, c))


def _forcer(monkeypatch, mod, attr):
    return lambda c: monkeypatch.setattr(mod, attr, c)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the tests
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
def test_f32_tiles(name, monkeypatch):
    """fp32 arithmetic (v_mfma_f32_16x16x4_f32), configurations 0-8 and 17.  The GELU epilogue (gelu_erf) meets the plain bound on every tile: no extra term."""
    from keypointfusion_amd import engine as E
    problems = []
    _sweep(_variant("f32", name), F32_ARITH, _forcer(monkeypatch, E, "FORCE_TILE"), problems)
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_f32_tiles_with_16bit_products(prec, monkeypatch):
    """KPF_MMA_BF16 / _F16 on fp32 storage: a permission.  Each tile gives the fp32-product bits (those of the same launch without the flag) or the bits of the
    products of the rounded operands, and the latter on exactly the tile shapes launch_cfg names."""
    from keypointfusion_amd import engine as E
    force = _forcer(monkeypatch, E, "FORCE_TILE")
    v = _variant("f32", "mma_" + prec)
    v32 = SimpleNamespace(**{**vars(v), "flags": 0, "round_to": None})
    v32.ref, v32.ref2 = _restate(v32, torch.float64)
    v32.plain, v32.plain2 = _restate(v32, torch.float32)
    force(0)
    fp32_bits = _run(v32)["out"]
    problems, rounded, first = [], set(), None
    _accuracy(v32, {"out": fp32_bits}, problems, "no flag")
    for c in F32_ARITH:
        force(c + 1)
        got = _run(v)["out"]
        force(0)
        if _bits(got, fp32_bits):
            print("TILE %-10s %-12s cfg %-2d     fp32-product bits" % (v.fam, v.name, c))
            continue
        rounded.add(c)
        if first is None:
            first = got
            _accuracy(v, {"out": got}, problems, "cfg %d" % c)
            far = float((_nhwc(v, got) - v32.ref).abs().max() / v32.ref.abs().max())
            assert far > 1e-4, far  # (the rounded products are two orders of magnitude from the fp32 ones: the 16-bit kernel did run)
        same = _bits(got, first)
        print("TILE %-10s %-12s cfg %-2d     rounded-product bits%s" % (v.fam, v.name, c, "" if same else "  DIFFERS from the first rounded tile"))
        if not same:
            problems.append("cfg %d: neither the fp32-product bits nor the rounded-product bits" % c)
    assert rounded == F32_ROUNDED, (rounded, F32_ROUNDED)
    # the library's own choice under the flag is one of the two
    lib_bits = _run(v)["out"]
    assert _bits(lib_bits, fp32_bits) or _bits(lib_bits, first)
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("fam,name", [(f, n) for f in ("in_split", "w_split") for n in SPLIT_VARIANTS if (f, n) != ("in_split", "pro")])
def test_split_tiles(fam, name, monkeypatch):
    """3 x f16 MFMA on split operands (KPF_IN_SPLIT: rows pre-split in memory; KPF_W_SPLIT: fp32 activations split in registers), all 18 configurations.
    KPF_ACT_GELU_SAVE and KPF_RES_GELU_GRAD exist in fp32 arithmetic only: refused on every tile; a prologue goes with KPF_W_SPLIT only."""
    from keypointfusion_amd import engine as E
    monkeypatch.setattr(E, "GEMM_MODE", "split")
    problems = []
    _sweep(_variant(fam, name), list(range(len(F32_TILES))), _forcer(monkeypatch, E, "FORCE_TILE"), problems,
           expect_refusal=lambda c: name in ("gelu_save", "ggrad"))
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_h16_tiles(prec, name, monkeypatch):
    """16-bit storage, the igemm cases of kpf_conv2d_h16 (cases 0 and 6 are the one-stage `occ` kernels without a residual or prologue, the two-stage ones with).
    N = 264 where the variant has a 264-wide form, so that the 256-wide tile has its interior and ragged workgroups.  The GELU-gradient epilogue exists on
    the two-stage tiles only.  Case 30 is asked for as well: none of these shapes is one gemm16_8ph_kernel takes (g8_applies: N % 256, Cin % 128), and the
    dispatcher then keeps its own choice: status 0 and the same bits, not a refusal."""
    from keypointfusion_amd import engine16 as E16
    problems = []
    wide = 264 if not (name.startswith("u_") or name.startswith("nchw")) else 200
    _sweep(_variant(prec, name, wide), H16_IGEMM + [30], _forcer(monkeypatch, E16, "FORCE_TILE16"), problems,
           expect_refusal=lambda c: name.endswith("ggrad") and H16_TILES[c][2] > 2, n_wide=wide)
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lin", "gelu", "res"])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_h16_eight_phase_kernel(prec, kind, monkeypatch):
    """gemm16_8ph_kernel (case 30) on a shape it accepts with a ragged last pixel tile: M = 300, Cin = 256, N = 512.  Held to the float64 bounds; whether its
    bits equal the igemm tiles' is printed, not asserted (the kernel has its own k order; g8_preferred selects it from M * N / 65536 >= 224 tiles on)."""
    from keypointfusion_amd import engine as E, engine16 as E16, lib as L
    from keypointfusion_amd.packs import PackedConv
    dev = _dev()
    tdt, eps = PREC[prec]
    g = torch.Generator().manual_seed(30 + len(kind))
    Mp, K, N = 300, 256, 512
    r16 = lambda t: t.to(tdt).float()
    x, w, bias, res = r16(torch.randn(Mp, K, generator=g)), r16(torch.randn(N, K, generator=g) / K ** 0.5), torch.randn(N, generator=g) * 0.1, r16(torch.randn(Mp, N, generator=g))
    ref = x.double() @ w.double().t() + bias.double()
    ref = F.gelu(ref) if kind == "gelu" else (ref + res.double() if kind == "res" else ref)
    p16 = PackedConv(w, bias, dev).as16(tdt)
    v = SimpleNamespace(h16=True, fam=prec)

    def run(cfg):
        monkeypatch.setattr(E16, "FORCE_TILE16", cfg)
        ob = _canary(dev, v, Mp + 1, N)
        kw = dict(flags=L.KPF_ACT_GELU if kind == "gelu" else 0)
        if kind == "res":
            kw["res"] = E.Act(res.to(dev).to(tdt).view(-1), Mp, 1, 1, N)
        E16.conv16(p16, E.Act(x.to(dev).to(tdt).view(-1), Mp, 1, 1, K), E16.DTYPES[prec][1], out=E.Act(ob.view(-1), Mp, 1, 1, N), **kw)
        torch.cuda.synchronize()
        monkeypatch.setattr(E16, "FORCE_TILE16", 0)
        assert _kept(v, ob[Mp]), "wrote behind the last pixel"
        return ob[:Mp].cpu()

    d = L.ConvDesc()
    d.B, d.IH, d.IW, d.OH, d.OW, d.Cin, d.in_ld, d.N, d.Kp, d.out_ld, d.res_ld = Mp, 1, 1, 1, 1, K, K, N, K, N, N
    d.KH = d.KW = d.sh = d.sw = 1
    d.flags = (L.KPF_ACT_GELU if kind == "gelu" else 0) | (L.KPF_RES_ADD if kind == "res" else 0)
    assert not L.load().kpf_conv2d_h16_uses_8ph(E.C.byref(d), 0)  # the library's own choice at this size is an igemm tile: the force is what selects case 30
    got8, goti = run(31), run(0)
    for who, got in (("case 30", got8), ("library", goti)):
        assert bool(torch.isfinite(got.float()).all())
        excess, bound = h16_excess(got.double(), ref, eps, "gelu" if kind == "gelu" else "rounding")
        print("ERR %-44s e_kernel %.3e  bound %-8s excess %+.3e" % ("%s 8ph_%s [%s]" % (prec, kind, who), float((got.double() - ref).abs().max() / ref.abs().max()), bound, excess))
        assert excess <= 0 if bound == "gelu" else excess < 0, (who, excess)
    n_ = int((_raw(got8) != _raw(goti)).sum())
    print("TILE %-10s %-12s case 30    %s" % (prec, "8ph_" + kind, "bits equal to the igemm tile" if n_ == 0 else "differs from the igemm tile in %d of %d elements (recorded, not asserted)" % (n_, got8.numel())))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["res_inplace", "gelu"])
def test_autotuner_returns_the_untuned_bits(name, monkeypatch):
    """engine.AUTOTUNE: the tuned call returns the bits of the untuned one; the timing runs of an in-place residual layer go to a scratch output (the residual
    is added once); the remembered configuration is one of the candidates."""
    from keypointfusion_amd import engine as E
    v = _variant("f32", name)
    op = _operand("f32", name, 200)
    monkeypatch.setattr(E, "FORCE_TILE", 0)
    monkeypatch.setattr(E, "AUTOTUNE", False)
    base = _run(v)
    monkeypatch.setattr(E, "AUTOTUNE", True)
    monkeypatch.setattr(op, "tuned", {})
    tuned = _run(v)     # times the candidates, then launches
    again = _run(v)     # from the cache
    assert len(op.tuned) == 1 and set(op.tuned.values()) <= {c + 1 for c in F32_ARITH}, op.tuned
    print("TILE %-10s %-12s autotuned  cfg %d" % ("f32", name, list(op.tuned.values())[0] - 1))
    assert _bits(tuned["out"], base["out"]) and _bits(again["out"], base["out"])
    problems = []
    _accuracy(v, tuned, problems, "autotuned")
    assert not problems, problems
