"""Shared by test_dw7_forms_gpu.py and dw7_forms_child.py: the shapes of the depthwise 7x7 family (csrc/kpf_elem.hip: kpf_dwconv7_ln_f32 / _split_f32 / _h16,
kpf_dwconv7_f32 / _add_f32; csrc/kpf_wgrad.hip: kpf_dwconv7_wgrad), seeded operands, the float64 / plain-fp32 results of torch on the CPU, and one guarded call
of each entry point through lib.load().

Data.  x ~ 2 N(0,1) + 0.3, taps N(0,1) / 7, bias 0.1 N(0,1) (+ 5 in the cases marked `shift`: |mean| >> sigma over the channels, where a one-pass variance
cancels), LayerNorm weight in [0.5, 1.5), LayerNorm bias 0.1 N(0,1); the activation of a 16-bit case is rounded to storage first (taps and parameters are fp32
in the interface).  Every device operand is a slice [GUARD, GUARD + n) of a buffer filled with a quiet NaN that carries a payload (16-byte aligned: GUARD
elements are 256 / 128 bytes); outputs and the workspace start as that NaN.  After a call every guard must hold its bits and the output must be finite: a store
past a ragged strip moves a guard, a read outside an operand or an output left unwritten leaves a NaN."""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from igemm_bounds import PREC, h16_excess
from test_igemm_tiles_gpu import CANARY16, from_split, to_split
from wgrad_forms import CANARY, FLOOR, GUARD, within

EPS = 1e-6
KINDS = ("f32", "split", "bf16", "f16")

#  kpf_dwconv7_ln_*: name -> (B, H, W, C, shift)
LN_CASES = {
    "tile96":     (2, 19, 37, 96, False),    # 3 x 2 tiles of 8 x 32: interior + ragged in both directions, halos crossing tiles
    "tile128":    (2, 19, 37, 128, True),
    "tile192":    (2, 19, 21, 192, False),   # 16-pixel tiles
    "wave40":     (2, 9, 13, 40, True),      # LG = 32, 10 of 32 lanes live
    "wave96":     (2, 9, 13, 96, False),
    "wave128":    (2, 9, 13, 128, False),
    "wave136":    (2, 9, 13, 136, True),     # LG = 64, 34 of 64 lanes live
    "wave192":    (2, 9, 13, 192, False),
    "wave256":    (2, 9, 13, 256, False),
    "wide320":    (2, 9, 13, 320, False),    # NT = 128
    "wide512":    (2, 9, 13, 512, False),
    "wide640":    (2, 9, 13, 640, True),     # NT = 192
    "wide768":    (2, 9, 13, 768, False),
    "wide800":    (2, 9, 13, 800, False),    # NT = 256
    "wide1024":   (2, 9, 13, 1024, False),
    "wide320r2":  (26, 9, 13, 320, False),   # 26 * 5 * 2 = 260 >= 256 workgroups: the two-row form
    "two1056":    (2, 9, 13, 1056, True),
    "tiny40":     (2, 3, 5, 40, False),
    "tiny96":     (2, 4, 4, 96, False),
    "tiny768":    (2, 2, 2, 768, True),
    "tiny1056":   (1, 4, 4, 1056, False),
    "tiny2048":   (1, 2, 2, 2048, False),
}
#  kpf_dwconv7_f32 / _add_f32 and kpf_dwconv7_wgrad: name -> (B, H, W, C)
TRAIN_CASES = {
    "c8":     (2, 7, 13, 8),
    "c100":   (2, 7, 13, 100),
    "c248":   (2, 7, 13, 248),    # the last width with the taps in LDS
    "c252":   (2, 7, 13, 252),    # the first with the taps from global memory
    "m4x4":   (2, 4, 4, 96),
    "m2x3":   (1, 2, 3, 8),
    "m1x1":   (1, 1, 1, 8),
}
WGRAD_ONLY = {
    "w20":    (3, 7, 20, 36),
    "w70":    (1, 3, 70, 12),
    "q32":    (2, 8, 8, 384),     # 32-quad channel blocks: 66.5 KB of LDS, the raised limit
    "w296":   (1, 2, 296, 8),     # 37 segments: the register-window kernel by shape alone
}
WGRAD_CASES = {**TRAIN_CASES, **WGRAD_ONLY}


def ln_kinds(name):
    return [k for k in KINDS if k != "split" or LN_CASES[name][3] % 32 == 0]


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def _store(t, kind):
    """fp32 values as the storage type of `kind` holds them"""
    return t.to(PREC[kind][0]).float() if kind in PREC else t


def _conv(x, w, b, dt):
    """NHWC x, weight [C][1][7][7], bias -> NCHW result in precision dt"""
    return F.conv2d(x.to(dt).permute(0, 3, 1, 2), w.to(dt), b.to(dt), padding=3, groups=x.shape[-1])


def taps(w, mirrored=False):
    """[C][1][7][7] -> the kernels' tap table [49][C]"""
    w = w.flip(2, 3) if mirrored else w
    return w.reshape(w.shape[0], 49).t().contiguous()


@functools.lru_cache(maxsize=None)
def ln_case(name, kind):
    """Operands and the float64 / plain-fp32 results of conv2d(groups = C) + layer_norm; built once and left unchanged.  "split" shares the operands of "f32"."""
    if kind == "split":
        return ln_case(name, "f32")
    Bn, H, W, Cc, shift = LN_CASES[name]
    g = _gen("ln/" + name)
    v = SimpleNamespace(name=name, B=Bn, H=H, W=W, C=Cc, shift=shift)
    v.x = _store(2 * torch.randn(Bn, H, W, Cc, generator=g) + 0.3, kind)
    v.w = torch.randn(Cc, 1, 7, 7, generator=g) / 7
    v.b = 0.1 * torch.randn(Cc, generator=g) + (5.0 if shift else 0.0)
    v.lw = torch.rand(Cc, generator=g) + 0.5
    v.lb = 0.1 * torch.randn(Cc, generator=g)
    ln = lambda dt: F.layer_norm(_conv(v.x, v.w, v.b, dt).permute(0, 2, 3, 1), (Cc,), v.lw.to(dt), v.lb.to(dt), EPS)
    v.ref, v.plain = ln(torch.float64), ln(torch.float32)
    assert bool(torch.isfinite(v.ref).all()) and float(v.ref.abs().max()) > 1.0
    return v


@functools.lru_cache(maxsize=None)
def train_case(name):
    """x, dy, weight, bias, the skip path's gradient; y, dx, dw, db of torch's conv2d and its backward in float64 and in plain fp32"""
    Bn, H, W, Cc = WGRAD_CASES[name]
    g = _gen("train/" + name)
    v = SimpleNamespace(name=name, B=Bn, H=H, W=W, C=Cc)
    v.x = 2 * torch.randn(Bn, H, W, Cc, generator=g) + 0.3
    v.dy = torch.randn(Bn, H, W, Cc, generator=g)
    v.add = torch.randn(Bn, H, W, Cc, generator=g)
    v.w = torch.randn(Cc, 1, 7, 7, generator=g) / 7
    v.b = 0.1 * torch.randn(Cc, generator=g)
    for tag, dt in (("ref", torch.float64), ("plain", torch.float32)):
        x = v.x.to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        w, b = v.w.to(dt).requires_grad_(True), v.b.to(dt).requires_grad_(True)
        y = F.conv2d(x, w, b, padding=3, groups=Cc)
        y.backward(v.dy.to(dt).permute(0, 3, 1, 2))
        dx = x.grad.permute(0, 2, 3, 1)
        setattr(v, tag, {"fwd": y.detach().permute(0, 2, 3, 1), "dgrad": dx, "dgrad_add": dx + v.add.to(dt), "dw": w.grad.reshape(Cc, 7, 7), "db": b.grad})
    return v


# ----------------------------------------------------------------------------------------------------------------------------------------
# bounds: one definition each
# ----------------------------------------------------------------------------------------------------------------------------------------
def rel_errors(got, ref, plain):
    """-> (e_kernel, e_plain), both relative to max|ref64|"""
    den = float(ref.abs().max())
    return float((got.double() - ref).abs().max()) / den, float((plain.double() - ref).abs().max()) / den


def ln_figures(v, kind, y):
    """y: the kernel's output as the CPU tensor of its storage type -> the figures the bound of `kind` is stated in.
      f32:    e_kernel <= 4 * e_plain + FLOOR (wgrad_forms.within)
      split:  the same on from_split(y), plus e_rt = what a to_split / from_split round trip does to the float64 reference itself
      16-bit: igemm_bounds.h16_excess(.., "rounding") <= 0 against float64 on the activation as stored (e_plain: the plain fp32 result rounded to storage)"""
    if kind in PREC:
        ek, ep = rel_errors(y.float(), v.ref, v.plain.to(PREC[kind][0]).float())
        return {"e_kernel": ek, "e_plain": ep, "excess": h16_excess(y.double(), v.ref, PREC[kind][1], "rounding")[0]}
    if kind == "split":
        ek, ep = rel_errors(from_split(y), v.ref, v.plain)
        return {"e_kernel": ek, "e_plain": ep, "e_rt": rel_errors(from_split(to_split(v.ref.float())), v.ref, v.plain)[0]}
    ek, ep = rel_errors(y, v.ref, v.plain)
    return {"e_kernel": ek, "e_plain": ep}


def misses(f):
    """the bound of the figures `f` (ln_figures, or {"e_kernel", "e_plain"} of an fp32 result) -> None, or what it misses by"""
    if "excess" in f:
        return None if f["excess"] <= 0 else "h16_excess(rounding) = %.3e > 0" % f["excess"]
    extra = f.get("e_rt", 0.0)
    if within(f["e_kernel"], f["e_plain"]) or f["e_kernel"] <= 4 * f["e_plain"] + FLOOR + extra:
        return None
    return "e_kernel %.3e > 4 * %.3e + %.3e%s" % (f["e_kernel"], f["e_plain"], FLOOR, " + %.3e" % extra if extra else "")


def line(op, fam, case, kind, f, note=""):
    """the record: DW7 <op> <family> <case> <type> e_kernel e_plain"""
    s = "DW7 %-9s %-14s %-9s %-5s e_kernel %.3e e_plain %.3e" % (op, fam, case, kind, f["e_kernel"], f["e_plain"])
    if "e_rt" in f:
        s += " e_rt %.3e" % f["e_rt"]
    if "excess" in f:
        s += " excess %+.3e" % f["excess"]
    return s + (" MISSES" if misses(f) else "") + ("  " + note if note else "")


def form(p):
    """the plan as the records name it: family and its parameters"""
    from keypointfusion_amd import lib as L
    fam = L.KPF_DW7_FAMILY[p.family]
    if fam == "tile":
        return "tile<%d,%d>" % (p.nchk, p.px)
    if fam == "wave":
        return "wave<%d>" % p.lg
    if fam == "wide":
        return "wide<%d,%d>" % (p.nt, p.rows)
    if fam == "two_launch":
        return "two<%d,%s>" % (p.px, "lds" if p.taps_lds else "glb")
    if fam == "tiny":
        return "tiny<%d,%d>" % (p.S, p.nt)
    if fam == "conv":
        return "conv<%d,%d,%s>" % (p.px, p.rows, "lds" if p.taps_lds else "glb")
    return "%s<%d,%dx%d>" % (fam[6:], p.cq, p.S, p.rows_per_chunk)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the plan query (no device call)
# ----------------------------------------------------------------------------------------------------------------------------------------
def plan(op, shape, kind="f32"):
    from keypointfusion_amd import lib as L
    p = L.Dw7Plan()
    dt = {"bf16": L.KPF_DT_BF16, "f16": L.KPF_DT_F16}.get(kind, L.KPF_DT_F32)
    L.check(L.load().kpf_dwconv7_plan(L.KPF_DW7_OP[op], dt, int(kind == "split"), *shape[:4], C.byref(p)), "kpf_dwconv7_plan")
    return p


def family(p):
    from keypointfusion_amd import lib as L
    return L.KPF_DW7_FAMILY[p.family]


# ----------------------------------------------------------------------------------------------------------------------------------------
# the device side
# ----------------------------------------------------------------------------------------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from keypointfusion_amd import lib
    lib.load()
    return torch.device("cuda:0")


class Slab:
    """n elements between two guards of GUARD elements, everything filled with the quiet NaN of the type; `t` (optional): what the n elements hold."""

    def __init__(self, n, kind="f32", t=None):
        self.n, self.kind = n, kind
        self.tdt = PREC[kind][0] if kind in PREC else torch.float32
        idt, self.fill = (torch.int16, CANARY16[kind]) if kind in PREC else (torch.int32, CANARY)
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=idt, device=dev())
        if t is not None:
            assert t.numel() == n
            self.buf[GUARD:GUARD + n] = t.reshape(-1).to(self.tdt).contiguous().view(idt).to(self.buf.device)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        assert self.ptr % 16 == 0

    def kept(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())

    def cpu(self, shape):
        return self.buf[GUARD:GUARD + self.n].cpu().view(self.tdt).view(*shape)


def _checked(tag, slabs, outs):
    for what, s in slabs.items():
        assert s.kept(), "%s: a guard of %s lost its bits" % (tag, what)
    for what, t in outs.items():
        assert bool(torch.isfinite(t.float()).all()), "%s: %s is not finite (an element left unwritten, or a read outside an operand)" % (tag, what)


def crc(t):
    return zlib.crc32(t.contiguous().view(torch.uint8).numpy().tobytes())


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _ln_operands(name, kind):
    v = ln_case(name, kind)
    return {"x": Slab(v.x.numel(), kind if kind in PREC else "f32", v.x), "w": Slab(49 * v.C, t=taps(v.w)), "b": Slab(v.C, t=v.b), "lw": Slab(v.C, t=v.lw),
            "lb": Slab(v.C, t=v.lb)}


def run_ln(name, kind):
    """One call of the entry point of `kind` -> (the output as the CPU tensor of its storage type, the plan) after the guard checks."""
    from keypointfusion_amd import lib as L
    lib = L.load()
    v = ln_case(name, kind)
    ops = _ln_operands(name, "f32" if kind == "split" else kind)
    y = Slab(v.x.numel(), kind if kind in PREC else "f32")
    p = plan("ln", (v.B, v.H, v.W, v.C), kind)
    args = [ops["x"].ptr, ops["w"].ptr, ops["b"].ptr, ops["lw"].ptr, ops["lb"].ptr, y.ptr, v.B, v.H, v.W, v.C, EPS]
    if kind in PREC:
        L.check(lib.kpf_dwconv7_ln_h16(*args, L.KPF_DT_BF16 if kind == "bf16" else L.KPF_DT_F16, _stream()), "kpf_dwconv7_ln_h16")
    else:
        fn = lib.kpf_dwconv7_ln_split_f32 if kind == "split" else lib.kpf_dwconv7_ln_f32
        L.check(fn(*args, _stream()), "kpf_dwconv7_ln_f32")
    torch.cuda.synchronize()
    out = y.cpu((v.B, v.H, v.W, v.C))
    shown = from_split(out) if kind == "split" else out
    _checked("ln %s/%s %s" % (name, kind, form(p)), {**ops, "y": y}, {"y": shown})
    return out, p


@functools.lru_cache(maxsize=None)
def _train_operands(name):
    v = train_case(name)
    return {"x": Slab(v.x.numel(), t=v.x), "dy": Slab(v.x.numel(), t=v.dy), "add": Slab(v.x.numel(), t=v.add), "w": Slab(49 * v.C, t=taps(v.w)),
            "wm": Slab(49 * v.C, t=taps(v.w, mirrored=True)), "b": Slab(v.C, t=v.b), "zb": Slab(v.C, t=torch.zeros(v.C))}


def run_conv(name, op):
    """op = fwd: kpf_dwconv7_f32(x, taps, bias);  dgrad: the same kernel on dy with the taps mirrored and a zero bias;  dgrad_add: kpf_dwconv7_add_f32 with the skip
    path's gradient (training.DwConv7NHWC.backward) -> (y, the plan)"""
    from keypointfusion_amd import lib as L
    lib = L.load()
    v = train_case(name)
    ops = _train_operands(name)
    y = Slab(v.x.numel())
    p = plan("fwd", (v.B, v.H, v.W, v.C))
    if op == "fwd":
        L.check(lib.kpf_dwconv7_f32(ops["x"].ptr, ops["w"].ptr, ops["b"].ptr, y.ptr, v.B, v.H, v.W, v.C, _stream()), "kpf_dwconv7_f32")
    elif op == "dgrad":
        L.check(lib.kpf_dwconv7_f32(ops["dy"].ptr, ops["wm"].ptr, ops["zb"].ptr, y.ptr, v.B, v.H, v.W, v.C, _stream()), "kpf_dwconv7_f32")
    else:
        L.check(lib.kpf_dwconv7_add_f32(ops["dy"].ptr, ops["wm"].ptr, ops["zb"].ptr, ops["add"].ptr, y.ptr, v.B, v.H, v.W, v.C, _stream()), "kpf_dwconv7_add_f32")
    torch.cuda.synchronize()
    out = y.cpu((v.B, v.H, v.W, v.C))
    _checked("%s %s %s" % (op, name, form(p)), {**ops, "y": y}, {"y": out})
    return out, p


def run_wgrad(name):
    """kpf_dwconv7_wgrad on a workspace of exactly the size the plan names -> (dw [C][7][7], db [C], the plan)"""
    from keypointfusion_amd import lib as L
    lib = L.load()
    v = train_case(name)
    ops = _train_operands(name)
    p = plan("wgrad", (v.B, v.H, v.W, v.C))
    assert 0 < p.ws_floats <= lib.kpf_dwconv7_wgrad_ws_floats(v.B, v.H, v.C), (name, p.ws_floats)  # what callers allocate covers the call
    dw, db, ws = Slab(49 * v.C), Slab(v.C), Slab(p.ws_floats)
    L.check(lib.kpf_dwconv7_wgrad(ops["dy"].ptr, ops["x"].ptr, dw.ptr, db.ptr, ws.ptr, p.ws_floats, v.B, v.H, v.W, v.C, None, _stream()), "kpf_dwconv7_wgrad")
    torch.cuda.synchronize()
    gw, gb = dw.cpu((v.C, 7, 7)), db.cpu((v.C,))
    _checked("wgrad %s %s" % (name, form(p)), {**ops, "dw": dw, "db": db, "ws": ws}, {"dw": gw, "db": gb})
    return gw, gb, p
