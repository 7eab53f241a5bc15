"""CPU tests of the implicit GEMM's operand (packs.ConvGeom / Pack and its constructors) and of the one launch-descriptor builder (engine.conv_desc).
Every expected tuple, descriptor field and flag word is a literal worked out by hand from the formulas the constructors replaced; nothing here calls the
code under test to learn what to expect, and nothing touches a device.  Further down: PackCache's descriptor table and pack calls (literals recorded from
the cache as it was before its entries became named records, under the same stand-in library), its behaviour under a faked graph capture, and
Conv2dNHWC's argument positions and autograd-context fields."""
import ctypes as C
import inspect
import re
import types

import pytest
import torch

from keypointfusion_amd import lib as L
from keypointfusion_amd import training as T
from keypointfusion_amd.engine import Act, conv_desc
from keypointfusion_amd.packs import ConvGeom, Pack, Packed16, PackedConv

# geometry literals: (KH, KW, Cin, sh, sw, ph, pw, merge, N, K), Kp (K rounded up to 32), Kp16 (K rounded up to 64)
GEOMS = {
    "conv3x3_s1_p1": (lambda: ConvGeom.forward(64, 32, 3, 3, 1, 1), (3, 3, 32, 1, 1, 1, 1, 1, 64, 288), 288, 320),
    "stem7x7_s2_p3_cin4": (lambda: ConvGeom.forward(64, 4, 7, 7, 2, 3), (7, 7, 4, 2, 2, 3, 3, 1, 64, 196), 224, 256),
    "patchify4x4_s4": (lambda: ConvGeom.forward(96, 3, 4, 4, 4, 0, True), (4, 1, 12, 4, 1, 0, 0, 4, 96, 48), 64, 64),
    "patchify2x2_s2": (lambda: ConvGeom.forward(192, 96, 2, 2, 2, 0, True), (2, 1, 192, 2, 1, 0, 0, 2, 192, 384), 384, 384),
    "linear_k131": (lambda: ConvGeom.forward(128, 131, 1, 1), (1, 1, 131, 1, 1, 0, 0, 1, 128, 131), 160, 192),
    "dgrad_3x3_p1_npad32": (lambda: ConvGeom.dgrad(16, 32, 3, 3, 1), (3, 3, 32, 1, 1, 1, 1, 1, 16, 288), 288, 320),
    "dgrad_5x5_p0": (lambda: ConvGeom.dgrad(8, 16, 5, 5, 0), (5, 5, 16, 1, 1, 4, 4, 1, 8, 400), 416, 448),
    "dgrad_rows_patchify2x2": (lambda: ConvGeom.dgrad_rows(96, 192, 2, 2), (1, 1, 192, 1, 1, 0, 0, 1, 384, 192), 192, 192),
    "depthwise_tap_table": (lambda: ConvGeom.dgrad_rows(1, 96, 7, 7), (1, 1, 96, 1, 1, 0, 0, 1, 49, 96), 96, 128),
    "rows_in_kernel_order": (lambda: ConvGeom.rows(8, 3, 3, 4, 1), (3, 3, 4, 1, 1, 1, 1, 1, 8, 36), 64, 64),
    "odd_width_view": (lambda: ConvGeom.forward(128, 131, 1, 1).widened(132), (1, 1, 132, 1, 1, 0, 0, 1, 128, 132), 160, 192),
}


def test_every_geometry_constructor_gives_the_literal_tuple_and_both_paddings():
    for name, (make, want, kp, kp16) in GEOMS.items():
        g = make()
        assert tuple(g) == want and (g.Kp, g.Kp16) == (kp, kp16), (name, tuple(g), g.Kp, g.Kp16)
    assert ConvGeom.forward(64, 32, 3, 3, 1, 1).flops(10) == 2.0 * 10 * 64 * 288 == 368640.0
    assert ConvGeom.forward(64, 4, 7, 7, 2, 3).out_hw(128, 128) == (64, 64) and ConvGeom.forward(192, 96, 2, 2, 2, 0, True).out_hw(8, 4) == (4, 4)


def _ungrouped(pc):
    return pc.groups == 0 and pc.w_gstride == 0 and pc.split_allowed is False and pc.tuned == {} and isinstance(pc, Pack)


def test_packedconv_on_cpu_is_the_float64_fold_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    W, b = torch.randn(6, 4, 3, 3, generator=g), torch.randn(6, generator=g)
    s, t = torch.rand(6, generator=g, dtype=torch.float64) + 0.5, torch.randn(6, generator=g, dtype=torch.float64)
    ps, pt = torch.rand(4, generator=g, dtype=torch.float64) + 0.5, torch.randn(4, generator=g, dtype=torch.float64)
    pc = PackedConv(W, b, "cpu", pad=1, fold_bn=(s, t), prologue=(ps, pt))
    want = torch.zeros(6, 64, dtype=torch.float64)  # K = 36 -> Kp = 64
    want[:, :36] = (W.double() * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(6, 36)  # conv -> BN: W' = W s, rows in (ky, kx, c) order
    assert tuple(pc.geom) == (3, 3, 4, 1, 1, 1, 1, 1, 6, 36) and (pc.N, pc.K, pc.Kp, pc.Kp16) == (6, 36, 64, 64)
    assert pc.w.dtype == torch.float32 and torch.equal(pc.w, want.float())
    assert torch.equal(pc.b, (b.double() * s + t).float())
    assert torch.equal(pc.ps, ps.float()) and torch.equal(pc.pt, pt.float()) and pc.w16 is None and _ungrouped(pc)
    # the ResNet stem: three image channels padded to four, no bias (zeros), two zero output channels appended
    W7 = torch.randn(6, 3, 7, 7, generator=g)
    st = PackedConv(W7, None, "cpu", stride=2, pad=3, fold_bn=(s, t), cin_pad=4, n_pad=8)
    w4 = torch.zeros(8, 7, 7, 4, dtype=torch.float64)
    w4[:6, :, :, :3] = (W7.double() * s[:, None, None, None]).permute(0, 2, 3, 1)
    want = torch.zeros(8, 224, dtype=torch.float64)  # K = 196 -> Kp = 224
    want[:, :196] = w4.reshape(8, 196)
    assert tuple(st.geom) == (7, 7, 4, 2, 2, 3, 3, 1, 8, 196) and torch.equal(st.w, want.float())
    assert torch.equal(st.b, torch.cat([t, torch.zeros(2, dtype=torch.float64)]).float()) and st.ps is None and st.pt is None
    # patchify 2x2/s2: same (ky, kx, c) rows, read as KH x 1 over the merged view
    W2 = torch.randn(8, 4, 2, 2, generator=g)
    pp = PackedConv(W2, b[:1].repeat(8), "cpu", stride=2, patchify=True)
    want = torch.zeros(8, 32, dtype=torch.float64)
    want[:, :16] = W2.double().permute(0, 2, 3, 1).reshape(8, 16)
    assert tuple(pp.geom) == (2, 1, 8, 2, 1, 0, 0, 2, 8, 16) and torch.equal(pp.w, want.float())
    # the 16-bit image: K padded to 64, rounded from the fp32 pack
    p16 = Packed16(pc, torch.bfloat16)
    assert p16.pc is pc and p16.Kp == 64 and torch.equal(p16.w, pc.w.to(torch.bfloat16)) and type(pc.as16(torch.bfloat16)) is Packed16


def test_device_pack_constructors_on_host_tensors():
    g = torch.Generator().manual_seed(4)
    W = torch.randn(128, 131, generator=g)  # Linear K = 131: Kp = 160, Kp16 = 192
    pc = T.DevPack(W, torch.randn(128, generator=g))
    assert tuple(pc.geom) == (1, 1, 131, 1, 1, 0, 0, 1, 128, 131) and tuple(pc.w.shape) == (128, 160) and pc.w16 is None and _ungrouped(pc)
    assert torch.equal(pc.w[:, :131], W) and not pc.w[:, 131:].any()
    p16 = pc.as16(torch.bfloat16)
    assert type(p16) is Packed16 and p16.pc is pc and p16.Kp == 192 and tuple(p16.w.shape) == (128, 192)
    assert torch.equal(p16.w[:, :131], W.to(torch.bfloat16)) and not p16.w[:, 131:].any()
    p = T.DevPack(W.to(torch.bfloat16), None)  # 16-bit shadow rows: the 16-bit operand directly, no fp32 one
    assert p.w is None and tuple(p.w16.shape) == (128, 192) and p.b is None and p.as16(torch.bfloat16).w is p.w16 and _ungrouped(p)
    odd = T._OddPack(pc, 132)
    assert tuple(odd.geom) == (1, 1, 132, 1, 1, 0, 0, 1, 128, 132) and (odd.Kp, odd.Kp16) == (160, 192) and odd.w is pc.w and odd.b is pc.b and _ungrouped(odd)
    assert odd.flops(3) == 2.0 * 3 * 128 * 132 and pc.flops(3) == 2.0 * 3 * 128 * 131 and tuple(pc.geom)[2] == 131  # (the base pack keeps its own width)
    rows = torch.randn(8, 36, generator=g)
    fr = T.DevPack.from_rows(rows, 3, 3, 4, 1)
    assert tuple(fr.geom) == (3, 3, 4, 1, 1, 1, 1, 1, 8, 36) and tuple(fr.w.shape) == (8, 64) and torch.equal(fr.w[:, :36], rows) and fr.b is None and _ungrouped(fr)
    pw = T.DevPack(torch.randn(8, 4, 2, 2, generator=g), None, stride=2, patchify=True)
    assert tuple(pw.geom) == (2, 1, 8, 2, 1, 0, 0, 2, 8, 16) and tuple(pw.w.shape) == (8, 32)
    big = torch.zeros(2, 8, 32)
    gp = T.GroupedPack([Pack(ConvGeom.plain(8, 32, 1, 1), w=big[i]) for i in range(2)], torch.zeros(16))
    assert (gp.groups, gp.w_gstride) == (2, 256) and tuple(gp.geom) == (1, 1, 32, 1, 1, 0, 0, 1, 8, 32) and gp.w.data_ptr() == big.data_ptr()
    sp = T.StackedPack(ConvGeom.plain(96, 32, 1, 1), torch.zeros(96, 32), torch.zeros(96), Pack(ConvGeom.plain(32, 96, 1, 1), w=torch.zeros(32, 96)))
    assert _ungrouped(sp) and _ungrouped(sp.dgrad) and (sp.dgrad.N, sp.dgrad.K, sp.dgrad.Kp) == (32, 96, 96) and sp.flops(2) == sp.dgrad.flops(2) == 2.0 * 2 * 96 * 32


def test_devpack_packed_hands_the_pack_kernel_the_same_arguments(monkeypatch):
    """DevPack.packed is one kpf_pack_conv_weight launch: on a stand-in library (no device) the arguments after the pointers and the
    shape / type of the destination are pinned for every mode: (N, Cin, KH, KW, mode, n_pad, row length)."""
    calls = []
    fake = types.SimpleNamespace(kpf_pack_conv_weight=lambda src, sdt, dst, ddt, *a: calls.append((sdt, ddt) + a[:-1]) or 0)
    monkeypatch.setattr(L, "load", lambda: fake)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))
    F32, BF16 = L.KPF_DT_F32, L.KPF_DT_BF16
    W = torch.zeros(30, 16, 3, 3)
    cases = [
        (dict(weight=W, bias=None, mode=0, prec="f32", stride=1, pad=1), (3, 3, 16, 1, 1, 1, 1, 1, 30, 144), (30, 160), torch.float32, (F32, F32, 30, 16, 3, 3, 0, 30, 160)),
        (dict(weight=W, bias=None, mode=1, prec="f32", pad=1, n_pad=32), (3, 3, 32, 1, 1, 1, 1, 1, 16, 288), (16, 288), torch.float32, (F32, F32, 30, 16, 3, 3, 1, 32, 288)),
        (dict(weight=W, bias=None, mode=1, prec="bf16", pad=1, n_pad=32), (3, 3, 32, 1, 1, 1, 1, 1, 16, 288), (16, 320), torch.bfloat16, (F32, BF16, 30, 16, 3, 3, 1, 32, 320)),
        (dict(weight=torch.zeros(192, 96, 2, 2), bias=None, mode=0, prec="bf16", stride=2, pad=0, patchify=True), (2, 1, 192, 2, 1, 0, 0, 2, 192, 384), (192, 384), torch.bfloat16,
         (F32, BF16, 192, 96, 2, 2, 0, 192, 384)),
        (dict(weight=torch.zeros(192, 96, 2, 2), bias=None, mode=2, prec="f32", n_pad=192), (1, 1, 192, 1, 1, 0, 0, 1, 384, 192), (384, 192), torch.float32, (F32, F32, 192, 96, 2, 2, 2, 192, 192)),
        (dict(weight=torch.zeros(96, 1, 7, 7), bias=None, mode=3, prec="bf16", n_pad=96), (1, 1, 96, 1, 1, 0, 0, 1, 49, 96), (49, 128), torch.bfloat16, (F32, BF16, 96, 1, 7, 7, 3, 96, 128)),
        (dict(weight=torch.zeros(128, 131), bias=torch.ones(128), mode=0, prec="f32", stride=1, pad=0, patchify=False), (1, 1, 131, 1, 1, 0, 0, 1, 128, 131), (128, 160), torch.float32,
         (F32, F32, 128, 131, 1, 1, 0, 128, 160)),
    ]
    for kw, geom, shape, dt, args in cases:
        pc = T.DevPack.packed(**kw)
        buf = pc.w if dt == torch.float32 else pc.w16
        assert tuple(pc.geom) == geom and tuple(buf.shape) == shape and buf.dtype == dt and (pc.w is None) != (pc.w16 is None) and _ungrouped(pc), (kw["mode"], tuple(pc.geom))
        assert calls[-1] == args, (calls[-1], args)
        assert (pc.b is None) == (kw["bias"] is None) and pc.ps is None and pc.pt is None


DESC_FIELDS = [n for n, _ in L.ConvDesc._fields_]


def _fields(d):
    return {n: getattr(d, n) for n in DESC_FIELDS}


def _desc(**kw):
    base = dict.fromkeys(DESC_FIELDS, 0)
    base["w_unscale"] = 0.0
    assert set(kw) <= set(base)
    return dict(base, **kw)


def test_descriptor_builder_fills_every_field_for_both_row_lengths():
    z = lambda *s: torch.zeros(*s)
    for kp_name, tdt in (("Kp", torch.float32), ("Kp16", torch.bfloat16)):
        buf = lambda n: torch.zeros(n, dtype=tdt)
        # plain 3x3/p1 layer reading a channel slice of a wider row
        pc = PackedConv(z(64, 32, 3, 3), None, "cpu", pad=1)
        kp = {"Kp": 288, "Kp16": 320}[kp_name]
        assert getattr(pc, kp_name) == kp
        d, out, optr, res, mo = conv_desc(pc, Act(buf(2 * 16 * 16 * 48), 2, 16, 16, 32, ld=48, coff=8), kp, flags=L.KPF_ACT_RELU)
        assert _fields(d) == _desc(B=2, IH=16, IW=16, Cin=32, in_ld=48, in_coff=8, OH=16, OW=16, N=64, KH=3, KW=3, sh=1, sw=1, ph=1, pw=1, Kp=kp, out_ld=64, flags=1)
        assert mo == (512, 16, 16) and res is None and optr is out.buf and out.buf.dtype == tdt and (out.B, out.H, out.W, out.C, out.ld, out.coff) == (2, 16, 16, 64, 64, 0)
        # patchify 2x2/s2 over the merged [H, W/2, 2C] view
        pc = PackedConv(z(192, 96, 2, 2), z(192), "cpu", stride=2, patchify=True)
        d, out, optr, res, mo = conv_desc(pc, Act.empty(1, 8, 8, 96, "cpu", tdt), 384)
        assert _fields(d) == _desc(B=1, IH=8, IW=4, Cin=192, in_ld=192, OH=4, OW=4, N=192, KH=2, KW=1, sh=2, sw=1, Kp=384, out_ld=192) and mo == (16, 4, 4)
        # the 105-channel head written fp32 NCHW
        pc = PackedConv(z(105, 128), z(105), "cpu")
        nchw = z(2, 105, 4, 4)
        d, out, optr, res, mo = conv_desc(pc, Act.empty(2, 4, 4, 128, "cpu", tdt), 128, out_nchw=nchw)
        assert _fields(d) == _desc(B=2, IH=4, IW=4, Cin=128, in_ld=128, OH=4, OW=4, N=105, KH=1, KW=1, sh=1, sw=1, Kp=128, out_ld=105, flags=32)
        assert out is None and optr is nchw and mo == (32, 4, 4)
        # residual + layer scale, in place in a channel slice
        pc = PackedConv(z(96, 384), z(96), "cpu")
        o = Act(buf(16 * 128), 1, 4, 4, 96, ld=128, coff=32)
        d, out, optr, res, mo = conv_desc(pc, Act.empty(1, 4, 4, 384, "cpu", tdt), 384, out=o, res=o, gamma=z(96))
        assert _fields(d) == _desc(B=1, IH=4, IW=4, Cin=384, in_ld=384, OH=4, OW=4, N=96, KH=1, KW=1, sh=1, sw=1, Kp=384, out_ld=128, out_coff=32, res_ld=128, res_coff=32, flags=4 | 8)
        assert out is o and res is o and optr is o.buf
        # GELU with the pre-activation saved to a second buffer (rides in the residual's slot)
        pc = PackedConv(z(384, 96), z(384), "cpu")
        kp = {"Kp": 96, "Kp16": 128}[kp_name]
        o2 = Act(buf(16 * 512), 1, 4, 4, 384, ld=512, coff=64)
        d, out, optr, res, mo = conv_desc(pc, Act.empty(1, 4, 4, 96, "cpu", tdt), kp, flags=L.KPF_ACT_GELU, out2=o2)
        assert _fields(d) == _desc(B=1, IH=4, IW=4, Cin=96, in_ld=96, OH=4, OW=4, N=384, KH=1, KW=1, sh=1, sw=1, Kp=kp, out_ld=384, res_ld=512, res_coff=64, flags=2 | 2048)
        assert res is o2 and mo == (16, 4, 4)
        # two groups over channel-stacked rows: one descriptor, the second operand w_gstride elements behind the first
        kp = {"Kp": 32, "Kp16": 64}[kp_name]
        big = torch.zeros(2, 8, kp, dtype=tdt)
        gp = T.GroupedPack([Pack(ConvGeom.plain(8, 32, 1, 1), **{"w" if tdt == torch.float32 else "w16": big[i]}) for i in range(2)], None)
        d, out, optr, res, mo = conv_desc(gp, Act(buf(10 * 64), 1, 1, 10, 32, ld=64), kp, out=Act(buf(10 * 16), 1, 1, 10, 8, ld=16), flags=L.KPF_ACT_RELU)
        assert _fields(d) == _desc(B=1, IH=1, IW=10, Cin=32, in_ld=64, OH=1, OW=10, N=8, KH=1, KW=1, sh=1, sw=1, Kp=kp, out_ld=16, flags=1, groups=2, w_gstride=8 * kp) and mo == (10, 1, 10)


# --- PackCache: every descriptor field and every kpf_pack_conv_weight argument, pinned to what the cache of commit f0e96db (positional 12- / 13-tuples)
# produced under this same stand-in library; kpf_pack_desc_blocks is host code and is served by the real library.
PACK_CASES = [((96, 48, 3, 3), 0, {}), ((128, 256, 3, 3), 1, dict(pad=1, n_pad=128)), ((100, 40, 3, 3), 1, dict(pad=1, n_pad=104)), ((192, 96, 2, 2), 0, dict(stride=2)),
              ((192, 96, 2, 2), 2, dict(n_pad=192)), ((384, 1, 7, 7), 2, dict(n_pad=384)), ((200, 1, 7, 7), 3, dict(n_pad=200)), ((64, 8, 4, 4), 0, dict(stride=4)),
              ((384, 96, 1, 1), 0, {}), ((384, 96, 1, 1), 1, dict(n_pad=384)), ((3, 128, 1, 1), 1, dict(n_pad=4)), ((105, 128, 1, 1), 0, {}), ((64, 20, 5, 5), 0, dict(pad=2))]
# (src - source.data_ptr(), dst - operand.data_ptr(), N, Cin, KH, KW, mode, n_pad, Kp, rows, src_dtype, dst_dtype, first_block, reserved): the 13 cases, q | k | v
# stacked (forward rows, data-gradient columns, bias slot each), three re-homed group operands (group 2 was registered first)
PACK_DESCS = {
    "f32": (534, [(0, 0, 96, 48, 3, 3, 0, 96, 448, 96, 0, 0, 0, 0),
                 (0, 0, 128, 256, 3, 3, 1, 128, 1152, 256, 0, 0, 42, 0),
                 (0, 0, 100, 40, 3, 3, 1, 104, 960, 40, 0, 0, 170, 0),
                 (0, 0, 192, 96, 2, 2, 0, 192, 384, 192, 0, 0, 190, 0),
                 (0, 0, 192, 96, 2, 2, 2, 192, 192, 384, 0, 0, 262, 0),
                 (0, 0, 384, 1, 7, 7, 2, 384, 384, 49, 0, 0, 334, 0),
                 (0, 0, 200, 1, 7, 7, 3, 200, 224, 49, 0, 0, 353, 0),
                 (0, 0, 64, 8, 4, 4, 0, 64, 128, 64, 0, 0, 364, 0),
                 (0, 0, 384, 96, 1, 1, 0, 384, 96, 384, 0, 0, 372, 0),
                 (0, 0, 384, 96, 1, 1, 1, 384, 384, 96, 0, 0, 408, 0),
                 (0, 0, 3, 128, 1, 1, 1, 4, 32, 128, 0, 0, 420, 0),
                 (0, 0, 105, 128, 1, 1, 0, 105, 128, 105, 0, 0, 422, 0),
                 (0, 0, 64, 20, 5, 5, 0, 64, 512, 64, 0, 0, 436, 0),
                 (0, 0, 128, 128, 1, 1, 0, 128, 128, 128, 0, 0, 468, 0),
                 (0, 0, 128, 128, 1, 1, 1, 128, 128, 128, 0, 0, 484, 384),
                 (0, 0, 128, 1, 1, 1, 4, 128, 128, 1, 0, 0, 488, 0),
                 (0, 65536, 128, 128, 1, 1, 0, 128, 128, 128, 0, 0, 489, 0),
                 (0, 512, 128, 128, 1, 1, 1, 128, 128, 128, 0, 0, 505, 384),
                 (0, 512, 128, 1, 1, 1, 4, 128, 128, 1, 0, 0, 509, 0),
                 (0, 131072, 128, 128, 1, 1, 0, 128, 128, 128, 0, 0, 510, 0),
                 (0, 1024, 128, 128, 1, 1, 1, 128, 128, 128, 0, 0, 526, 384),
                 (0, 1024, 128, 1, 1, 1, 4, 128, 128, 1, 0, 0, 530, 0),
                 (4096, 4096, 16, 32, 1, 1, 0, 16, 32, 16, 0, 0, 531, 0),
                 (0, 0, 16, 32, 1, 1, 0, 16, 32, 16, 0, 0, 532, 0),
                 (2048, 2048, 16, 32, 1, 1, 0, 16, 32, 16, 0, 0, 533, 0)]),
    "bf16": (548, [(0, 0, 96, 48, 3, 3, 0, 96, 448, 96, 0, 1, 0, 0),
                  (0, 0, 128, 256, 3, 3, 1, 128, 1152, 256, 0, 1, 42, 0),
                  (0, 0, 100, 40, 3, 3, 1, 104, 960, 40, 0, 1, 170, 0),
                  (0, 0, 192, 96, 2, 2, 0, 192, 384, 192, 0, 1, 190, 0),
                  (0, 0, 192, 96, 2, 2, 2, 192, 192, 384, 0, 1, 262, 0),
                  (0, 0, 384, 1, 7, 7, 2, 384, 384, 49, 0, 1, 334, 0),
                  (0, 0, 200, 1, 7, 7, 3, 200, 256, 49, 0, 1, 353, 0),
                  (0, 0, 64, 8, 4, 4, 0, 64, 128, 64, 0, 1, 366, 0),
                  (0, 0, 384, 96, 1, 1, 0, 384, 128, 384, 0, 1, 374, 0),
                  (0, 0, 384, 96, 1, 1, 1, 384, 384, 96, 0, 1, 422, 0),
                  (0, 0, 3, 128, 1, 1, 1, 4, 64, 128, 0, 1, 434, 0),
                  (0, 0, 105, 128, 1, 1, 0, 105, 128, 105, 0, 1, 436, 0),
                  (0, 0, 64, 20, 5, 5, 0, 64, 512, 64, 0, 1, 450, 0),
                  (0, 0, 128, 128, 1, 1, 0, 128, 128, 128, 0, 0, 482, 0),
                  (0, 0, 128, 128, 1, 1, 1, 128, 128, 128, 0, 0, 498, 384),
                  (0, 0, 128, 1, 1, 1, 4, 128, 128, 1, 0, 0, 502, 0),
                  (0, 65536, 128, 128, 1, 1, 0, 128, 128, 128, 0, 0, 503, 0),
                  (0, 512, 128, 128, 1, 1, 1, 128, 128, 128, 0, 0, 519, 384),
                  (0, 512, 128, 1, 1, 1, 4, 128, 128, 1, 0, 0, 523, 0),
                  (0, 131072, 128, 128, 1, 1, 0, 128, 128, 128, 0, 0, 524, 0),
                  (0, 1024, 128, 128, 1, 1, 1, 128, 128, 128, 0, 0, 540, 384),
                  (0, 1024, 128, 1, 1, 1, 4, 128, 128, 1, 0, 0, 544, 0),
                  (4096, 4096, 16, 32, 1, 1, 0, 16, 64, 16, 0, 1, 545, 0),
                  (0, 0, 16, 32, 1, 1, 0, 16, 64, 16, 0, 1, 546, 0),
                  (2048, 2048, 16, 32, 1, 1, 0, 16, 64, 16, 0, 1, 547, 0)]),
}
# (src_dtype, dst_dtype, N, Cin, KH, KW, mode, n_pad, row length) of every kpf_pack_conv_weight call, in order
PACK_CALLS = {
    "f32": [(0, 0, 96, 48, 3, 3, 0, 96, 448),
            (0, 0, 128, 256, 3, 3, 1, 128, 1152),
            (0, 0, 100, 40, 3, 3, 1, 104, 960),
            (0, 0, 192, 96, 2, 2, 0, 192, 384),
            (0, 0, 192, 96, 2, 2, 2, 192, 192),
            (0, 0, 384, 1, 7, 7, 2, 384, 384),
            (0, 0, 200, 1, 7, 7, 3, 200, 224),
            (0, 0, 64, 8, 4, 4, 0, 64, 128),
            (0, 0, 384, 96, 1, 1, 0, 384, 96),
            (0, 0, 384, 96, 1, 1, 1, 384, 384),
            (0, 0, 3, 128, 1, 1, 1, 4, 32),
            (0, 0, 105, 128, 1, 1, 0, 105, 128),
            (0, 0, 64, 20, 5, 5, 0, 64, 512),
            (0, 0, 16, 32, 1, 1, 0, 16, 32),
            (0, 0, 16, 32, 1, 1, 0, 16, 32),
            (0, 0, 16, 32, 1, 1, 0, 16, 32)],
    "bf16": [(0, 1, 96, 48, 3, 3, 0, 96, 448),
             (0, 1, 128, 256, 3, 3, 1, 128, 1152),
             (0, 1, 100, 40, 3, 3, 1, 104, 960),
             (0, 1, 192, 96, 2, 2, 0, 192, 384),
             (0, 1, 192, 96, 2, 2, 2, 192, 192),
             (0, 1, 384, 1, 7, 7, 2, 384, 384),
             (0, 1, 200, 1, 7, 7, 3, 200, 256),
             (0, 1, 64, 8, 4, 4, 0, 64, 128),
             (0, 1, 384, 96, 1, 1, 0, 384, 128),
             (0, 1, 384, 96, 1, 1, 1, 384, 384),
             (0, 1, 3, 128, 1, 1, 1, 4, 64),
             (0, 1, 105, 128, 1, 1, 0, 105, 128),
             (0, 1, 64, 20, 5, 5, 0, 64, 512),
             (0, 1, 16, 32, 1, 1, 0, 16, 64),
             (0, 1, 16, 32, 1, 1, 0, 16, 64),
             (0, 1, 16, 32, 1, 1, 0, 16, 64)],
}


def _fake_pack_lib(monkeypatch):
    packs, multis, capturing = [], [], [False]
    fake = types.SimpleNamespace(kpf_pack_conv_weight=lambda src, sdt, dst, ddt, *a: packs.append((src, dst, (sdt, ddt) + a[:-1])) or 0,
                                 kpf_pack_conv_weights_multi=lambda table, n, blk, st: multis.append((n, blk)) or 0,
                                 kpf_pack_desc_blocks=L.load().kpf_pack_desc_blocks)
    monkeypatch.setattr(L, "load", lambda: fake)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    return packs, multis, capturing


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_pack_cache_table_and_pack_calls_are_the_literals_of_the_tuple_era(monkeypatch, prec):
    packs, multis, capturing = _fake_pack_lib(monkeypatch)
    cache, bases = T.PackCache(), []
    for i, (shape, mode, kw) in enumerate(PACK_CASES):
        w = torch.zeros(shape)
        pc = cache.get(("k%d" % i, mode), w, None, mode, prec, **kw)
        bases.append((w, pc.w if pc.w is not None else pc.w16))
    qkv, bqkv = [torch.zeros(128, 128) for _ in range(3)], [torch.zeros(128) for _ in range(3)]
    sp = cache.get_stacked(["q", "k", "v"], qkv, bqkv)
    assert multis == [(9, 63)] and cache.get_stacked(["q", "k", "v"], qkv, bqkv) is sp and multis == [(9, 63)]  # (filled by one launch of its own table, once)
    for w, b in zip(qkv, bqkv):
        bases += [(w, sp.w), (w, sp.dgrad.w), (b, sp.b)]
    wg = torch.zeros(3 * 16, 32, 1, 1)
    cache.get(("grp", 0, 2), wg[32:48], None, 0, prec, stride=1, pad=0, patchify=False)  # (group 2 first: the three allocations cannot come out equally spaced)
    gp = T._operand(cache, "grp", wg, torch.zeros(48), 0, prec, 3, stride=1, pad=0, patchify=False)
    home = gp.w if prec == "f32" else gp.w16
    assert (gp.groups, gp.w_gstride) == (3, 16 * home.shape[1]) and all((pc.w if prec == "f32" else pc.w16).data_ptr() == home.data_ptr() + 2048 * g for g, pc in enumerate(gp.pcs))
    bases += [(wg, home)] * 3
    assert cache.dirty and cache.table is None
    cache.build_table()
    total, want = PACK_DESCS[prec]
    arr = (L.PackDesc * len(want)).from_buffer_copy(bytes(cache.table.numpy()))
    assert len(cache.entries) == len(want) == len(bases) == 25 and cache.table.numel() == 25 * C.sizeof(L.PackDesc) and not cache.dirty
    got = [((d.src or 0) - s.data_ptr(), (d.dst or 0) - t.data_ptr()) + tuple(getattr(d, n) for n, _ in L.PackDesc._fields_[2:]) for d, (s, t) in zip(arr, bases)]
    assert got == want and cache.total_blocks == total
    assert [e.desc.first_block for e in cache.entries.values()] == [r[12] for r in want]  # (the records carry what the table holds)
    assert [p[2] for p in packs] == PACK_CALLS[prec] and [p[:2] for p in packs[:13]] == [(s.data_ptr(), t.data_ptr()) for s, t in bases[:13]]
    capturing[0] = True  # a current table: the refresh inside a capture is the one table launch
    cache.refresh()
    assert multis == [(9, 63), (25, total)] and len(packs) == 16


def test_pack_cache_refresh_inside_a_capture_and_the_refusals(monkeypatch):
    packs, multis, capturing = _fake_pack_lib(monkeypatch)
    cache, regs = T.PackCache(), []
    for i, (shape, mode, kw) in enumerate(PACK_CASES[:3]):
        w = torch.zeros(shape)
        regs.append((w.data_ptr(), cache.get(("k%d" % i, mode), w, None, mode, "f32", **kw).w.data_ptr()))
    capturing[0] = True  # registered, no table yet: one kpf_pack_conv_weight per operand, the registration's own arguments again
    cache.refresh()
    assert multis == [] and [p[2] for p in packs[3:]] == PACK_CALLS["f32"][:3] and [p[:2] for p in packs[3:]] == regs == [p[:2] for p in packs[:3]]
    qkv, bqkv = [torch.zeros(128, 128) for _ in range(3)], [torch.zeros(128) for _ in range(3)]
    with pytest.raises(AssertionError, match="eager iteration"):
        cache.get_stacked(["q", "k", "v"], qkv, bqkv)
    capturing[0] = False
    cache.get_stacked(["q", "k", "v"], qkv, bqkv)
    capturing[0] = True  # a stacked operand without a table: its column-range / bias-slot forms exist in the table launch only
    with pytest.raises(RuntimeError, match="stacked operand was registered during a graph capture"):
        cache.refresh()
    params = [torch.zeros(4) for _ in range(2)]
    with pytest.raises(AssertionError, match="run one eager iteration after moving / re-homing parameters"):
        T.BertStack21.param_table(params)
    capturing[0] = False
    t = T.BertStack21.param_table(params)
    capturing[0] = True
    assert T.BertStack21.param_table(params) is t and t.tolist() == [p.data_ptr() for p in params]  # (a table that exists is found inside a capture)
    del T.BertStack21._tables[tuple(t.tolist())]
    del packs[:]
    T._dw_taps(torch.zeros(200, 1, 7, 7), True)  # the un-cached depthwise tap table keeps its own row length (C, not C rounded up to 32)
    assert packs[0][2] == (0, 0, 200, 1, 7, 7, 3, 200, 200)


class _OnDevice(torch.Tensor):
    """A host tensor that passes Conv2dNHWC.forward's device check (the GEMM itself is stubbed)."""
    is_cuda = True


class _Ctx:
    """What a forward does to its autograd context: attribute writes plus the three calls, recorded."""

    def __init__(self, needs):
        self.needs_input_grad = needs

    def save_for_backward(self, *ts):
        self.saved_tensors = ts

    def mark_non_differentiable(self, *ts):
        pass

    def set_materialize_grads(self, on):
        pass


def test_conv2d_nhwc_positions_come_from_the_signature_and_every_exit_records_what_backward_reads(monkeypatch):
    Fn = T.Conv2dNHWC
    assert tuple(inspect.signature(Fn.forward).parameters)[1:] == Fn.ARGS  # (an argument added to forward without moving ARGS fails here)
    assert Fn._grads() == (None,) * 15
    assert Fn._grads("dx", "dw", "db", "dres") == ("dx", "dw", "db") + (None,) * 7 + ("dres",) + (None,) * 4
    assert Fn._grads(dx="a") == ("a",) + (None,) * 14 and Fn._grads("dx", "dw", "db") == ("dx", "dw", "db") + (None,) * 12
    assert [Fn.ARGS.index(a) for a in ("x", "weight", "bias", "res")] == [0, 1, 2, 10]
    # the fields backward reads, from its source; the three forward exits, run on host tensors with the lookup and the GEMM stubbed
    reads = set(re.findall(r"\bctx\.(\w+)", inspect.getsource(Fn.backward) + inspect.getsource(Fn._backward))) - {"needs_input_grad"}
    assert {"saved_tensors", "mma16", "alias", "gelu_out", "res_dtype", "odd", "pack", "groups", "conf", "w16", "x_dtype", "bias_ptr"} <= reads
    assert "getattr(ctx" not in inspect.getsource(Fn.backward) + inspect.getsource(Fn._backward)
    monkeypatch.setattr(T, "_operand", lambda cache, key, w, b, mode, prec, groups=1, **kw: Pack(ConvGeom.plain(w.shape[0], w.shape[1], 1, 1), w=torch.zeros(1)))
    monkeypatch.setattr(T, "_conv_any", lambda pc, x4, prec, **kw: torch.zeros(x4.shape[0], 1, 1, pc.N))
    monkeypatch.setattr(T, "pad_rows", lambda src, width, dtype=None: torch.zeros(src.shape[:-1] + (width,), dtype=dtype))
    x = torch.zeros(6, 1, 1, 8).as_subclass(_OnDevice)
    w, b, res = torch.zeros(16, 8, 1, 1), torch.zeros(16), torch.zeros(6, 1, 1, 16, dtype=torch.bfloat16)
    exits = {"odd-width": (torch.zeros(6, 1, 1, 7).as_subclass(_OnDevice), torch.zeros(3, 7, 1, 1), None, 1, 0),
             "gelu_out": (x, w, b, 1, 0, "f32", None, "k", None, 1, None, False, True, True),
             "plain": (x, w, b, 1, 0, "f32", None, "k", None, 1, res, False, True, False)}
    seen = {}
    for name, args in exits.items():
        ctx = _Ctx((True,) * 15)
        with T.head_mma(5):
            Fn.forward(ctx, *args)
        assert reads <= set(vars(ctx)), (name, reads - set(vars(ctx)))
        seen[name] = {k: v for k, v in vars(ctx).items() if k not in ("saved_tensors", "needs_input_grad")}
    assert seen["odd-width"] == dict(mma16=5, groups=1, odd=(7, 8, 4), pack=(None, None), alias=False, gelu_out=False, res_dtype=None, w16=None, x_dtype=torch.float32,
                                     conf=(1, 0, False, "f32"), bias_ptr=None)
    assert seen["gelu_out"] == dict(mma16=5, groups=1, odd=None, pack=("k", None), alias=True, gelu_out=True, res_dtype=None, w16=None, x_dtype=torch.float32,
                                    conf=(1, 0, True, "f32"), bias_ptr=b.data_ptr())
    assert seen["plain"] == dict(seen["gelu_out"], gelu_out=False, res_dtype=torch.bfloat16)
