"""The operand of the implicit GEMM (kpf_conv2d_f32 / kpf_conv2d_h16): one geometry value, one pack type, one 16-bit image.

Everything a launch reads from a weight operand is declared here: the geometry (ConvGeom), the packed rows `w` (fp32 [N][Kp]) and / or `w16`
(16-bit [N][Kp16]), the fp32 bias `b`, the input prologue `ps` / `pt`, `groups` / `w_gstride` of a grouped launch, `split_allowed` and the
autotuning cache `tuned`.  The ways of building one (host fold: PackedConv here; device packs: training.DevPack and its relatives) are
constructors of Pack, not look-alikes of it."""
import math
from operator import attrgetter
from typing import NamedTuple

import torch


class ConvGeom(NamedTuple):
    """What the kernel convolves: KH x KW taps over Cin channels (k = (ky,kx,c), K = KH*KW*Cin of them) -> N outputs; merge > 1: the input is
    read as a [H, W/merge, merge*C] view of the same memory."""
    KH: int
    KW: int
    Cin: int
    sh: int
    sw: int
    ph: int
    pw: int
    merge: int
    N: int
    K: int

    @property
    def Kp(self):
        """row length of the fp32 operand (K padded to 32)"""
        return (self.K + 31) // 32 * 32

    @property
    def Kp16(self):
        """row length of the 16-bit operand (K padded to 64)"""
        return (self.K + 63) // 64 * 64

    def flops(self, M):
        return 2.0 * M * self.N * self.K

    def out_hw(self, IH, IW):
        return (IH + 2 * self.ph - self.KH) // self.sh + 1, (IW + 2 * self.pw - self.KW) // self.sw + 1

    @classmethod
    def plain(cls, N, Cin, KH, KW, stride=1, pad=0):
        return cls(KH, KW, Cin, stride, stride, pad, pad, 1, N, KH * KW * Cin)

    @classmethod
    def patchify(cls, N, Cin, KH, KW, stride, pad=0):
        """kernel == stride, pad 0: (kx, c) merged into the channel axis of a [H, W/KW, KW*C] view, executed as KH x 1"""
        assert stride == KH == KW and pad == 0
        return cls(KH, 1, KW * Cin, KH, 1, 0, 0, KW, N, KH * KW * Cin)

    @classmethod
    def forward(cls, N, Cin, KH, KW, stride=1, pad=0, patchify=False):
        return (cls.patchify if patchify else cls.plain)(N, Cin, KH, KW, stride, pad)

    @classmethod
    def dgrad(cls, Cin, n_pad, KH, KW, pad):
        """data gradient of a stride-1 (or dilated) convolution: Cin output rows, n_pad input channels, mirrored taps, padding KH-1-pad"""
        return cls(KH, KW, n_pad, 1, 1, KH - 1 - pad, KW - 1 - pad, 1, Cin, KH * KW * n_pad)

    @classmethod
    def dgrad_rows(cls, Cin, n_pad, KH, KW):
        """data-gradient rows of a patchify convolution, dY @ [(ky,kx,c)][n] (Cin = 1: the depthwise tap table [KH*KW][C])"""
        return cls(1, 1, n_pad, 1, 1, 0, 0, 1, KH * KW * Cin, n_pad)

    @classmethod
    def rows(cls, N, KH, KW, Cin, pad):
        """stride-1 convolution whose rows [N][(ky,kx,c)] are already in kernel order"""
        return cls.plain(N, Cin, KH, KW, 1, pad)

    def widened(self, cin_pad):
        """a Linear of odd input width seen at the padded width: the packed rows are zero beyond K anyway, only the descriptor changes"""
        g = self._replace(Cin=cin_pad, K=cin_pad)
        assert self.KH == self.KW == self.merge == 1 and cin_pad >= self.K and (g.Kp, g.Kp16) == (self.Kp, self.Kp16), (self, cin_pad)
        return g


class Pack:
    """One weight operand of the implicit GEMM; every launch (engine.conv, engine16.conv16) takes this type."""

    def __init__(self, geom, w=None, w16=None, b=None, ps=None, pt=None, groups=0, w_gstride=0):
        self.geom = geom
        self.w, self.w16 = w, w16  # fp32 rows [N][Kp] / 16-bit rows [N][Kp16] (either may be None)
        self.b, self.ps, self.pt = b, ps, pt  # fp32 bias [N] (None: nothing is added), input prologue (scale, shift) [Cin]
        self.groups, self.w_gstride = groups, w_gstride  # grouped launch: G operands w_gstride elements apart (0 = one convolution)
        # split (3 x f16) arithmetic only where the caller has proven |activation| < 65504 at pack time (ConvNeXtBlockPlan, the
        # downsample LayerNorms): everywhere else a large activation would saturate silently, so the default is the f32 MFMA
        self.split_allowed = False
        self.tuned = {}  # (shape, epilogue) -> tile configuration index + 1 (autotuning cache)
        self._ws = None

    def flops(self, M):
        return self.geom.flops(M)

    def as16(self, tdt):
        """The operand engine16.conv16() takes: the 16-bit rows as they are, or the fp32 rows rounded to `tdt`."""
        assert self.w16 is not None or not self.groups
        return Packed16(self, tdt, self.w16)

    def split_weights(self):
        """(w_split, w_unscale): rows of [Kp/32][hi 32 | lo 32] f16 of w * 2^s (s keeps the lo halves out of the f16 subnormals),
        viewed as fp32 [N][Kp]; built once from the fp32 pack (exactly representable inputs: the split is of the fp32 weights)."""
        if self._ws is None:
            ws, self._wus = split_pack(self.w)
            self._ws = ws.to(self.w.device)
        return self._ws, self._wus

    def row_l1(self):
        return float(self.w.abs().sum(1).max())


for _f in ConvGeom._fields + ("Kp", "Kp16"):  # pc.N, pc.K, ... read through to the geometry
    setattr(Pack, _f, property(attrgetter("geom." + _f)))


class Packed16:
    """16-bit image of a Pack: rows [N][Kp], Kp padded to 64 elements, in the storage dtype; bias stays fp32 (pc.b)."""

    def __init__(self, pc, tdt, rows=None):
        self.pc, self.Kp = pc, pc.geom.Kp16
        if rows is None:
            w = torch.zeros(pc.N, self.Kp, dtype=torch.float32, device=pc.w.device)
            w[:, :pc.K] = pc.w[:, :pc.K]
            rows = w.to(tdt).contiguous()
        assert rows.dtype == tdt and rows.shape[1] == self.Kp
        self.w = rows


def split_pack(w):
    """fp32/fp64 [N][K] (K % 32 == 0) -> (fp32-viewed [N][K] tensor holding [K/32][hi 32 | lo 32] f16 of w * 2^s, 2^-s): the split
    operand format of include/kpf.h; s keeps the lo halves out of the f16 subnormals."""
    w = w.double().cpu()
    N, K = w.shape
    assert K % 32 == 0
    amax = float(w.abs().max())
    s = 7 - math.floor(math.log2(amax)) if amax > 0 else 0
    ws = w * (2.0 ** s)
    hi = ws.half()
    lo = (ws - hi.double()).half()
    blk = torch.stack([hi.view(N, K // 32, 32), lo.view(N, K // 32, 32)], 2).contiguous()  # N, K/32, 2, 32
    return blk.view(torch.float32).reshape(N, K).contiguous(), 2.0 ** (-s)


class PackedConv(Pack):
    """Weights of one convolution/linear packed on the host: w [N][Kp] with k = (ky,kx,c), bias [N], eval-BatchNorm folded in float64
    (fold_bn), optional input prologue (scale, shift) [Cin]; patchify: see ConvGeom.patchify."""

    def __init__(self, weight, bias, device, stride=1, pad=0, fold_bn=None, prologue=None, cin_pad=None, patchify=False, n_pad=None):
        w = weight.detach().double().cpu()
        if w.dim() == 2:
            w = w[:, :, None, None]
        elif w.dim() == 3:
            w = w[:, :, :, None]
        N, Cin, KH, KW = w.shape
        b = bias.detach().double().cpu() if bias is not None else torch.zeros(N, dtype=torch.float64)
        if fold_bn is not None:  # conv -> BN : W' = W*s, b' = b*s + t
            s, t = fold_bn
            w = w * s.cpu()[:, None, None, None]
            b = b * s.cpu() + t.cpu()
        if n_pad is not None and n_pad > N:  # extra output channels that are identically zero (zero rows, zero bias)
            w = torch.cat([w, torch.zeros(n_pad - N, Cin, KH, KW, dtype=w.dtype)], 0)
            b = torch.cat([b, torch.zeros(n_pad - N, dtype=b.dtype)])
            N = n_pad
        if cin_pad is not None and cin_pad > Cin:
            w = torch.cat([w, torch.zeros(N, cin_pad - Cin, KH, KW, dtype=w.dtype)], 1)
            Cin = cin_pad
        geom = ConvGeom.forward(N, Cin, KH, KW, stride, pad, patchify)
        assert geom.Cin % 4 == 0, "input channels (after view) must be a multiple of 4"
        wp = torch.zeros(N, geom.Kp, dtype=torch.float64)
        wp[:, :geom.K] = w.permute(0, 2, 3, 1).reshape(N, geom.K)  # N KH KW Cin
        super().__init__(geom, w=wp.float().to(device), b=b.float().to(device))
        if prologue is not None:
            s, t = prologue
            assert s.numel() == Cin
            self.ps, self.pt = s.float().to(device).contiguous(), t.float().to(device).contiguous()
