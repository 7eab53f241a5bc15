"""Shared by test_wgrad_forms_gpu.py and wgrad_forms_child.py: the shapes, the float64 / plain-fp32 references and one canary-guarded call of
kpf_conv2d_wgrad through lib.load() (the caller owns dw, db and ws).

Geometry.  B = 2, OH = 13, OW = 11: M = 286 pixels = eight whole 32-pixel stages + 30 (two whole 128-pixel stages + 30 for wgrad_h16s_kernel).  N = 200: a whole
and a ragged tile at both tile widths (64, 128), and so is every K below.  Both operands are column slices [16, 16 + G * C) of wider rows whose other columns
hold NaN; the strides are multiples of 8 (of 4 where an fp32 operand has 4 channels) and the sliced pointers are 16-byte aligned."""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

FLOOR = 8 * 2.0 ** -24
CANARY = 0x7FC0BEEF  # a quiet NaN with a payload
GUARD = 64           # canary floats behind dw, db and ws
COFF = 16            # first column of the operand slices
N = 200
STAGE_PIXELS = {"f32": 32, "r16": 32, "direct": 32, "h16": 32, "h16s": 128}
TILE = {"h16s": (64, 64), "h16": (128, 128)}  # the fp32 families: (32 vn, 32 vk)

#            B  H   W   OH  OW  Cin (fp32, 16-bit)  k  s  p  G  cin_valid n_valid db
SHAPES = {
    "lin":    (2, 13, 11, 13, 11, (200, 200), 1, 1, 0, 1, 0, 0, True),
    "k3":     (2, 13, 11, 13, 11, (24, 24), 3, 1, 1, 1, 0, 0, True),     # K = 216: a tile boundary falls inside a tap
    "k3s2":   (2, 26, 22, 13, 11, (24, 24), 3, 2, 1, 1, 0, 0, True),
    "patch":  (2, 26, 22, 13, 11, (56, 56), 2, 2, 0, 1, 0, 0, True),     # K = 224
    "stem":   (2, 26, 22, 13, 11, (4, 8), 7, 2, 3, 1, 0, 0, True),       # one granule per tap, most taps partly outside the image
    "trim":   (2, 13, 11, 13, 11, (132, 136), 1, 1, 0, 1, 131, 197, True),
    "nodb":   (2, 13, 11, 13, 11, (200, 200), 1, 1, 0, 1, 0, 0, False),
    "tiny":   (1, 3, 5, 3, 5, (200, 200), 1, 1, 0, 1, 0, 0, True),       # a single ragged stage, S = 1
    "direct": (1, 9, 11, 9, 11, (200, 200), 1, 1, 0, 1, 0, 0, True),     # M = 99: the one-workgroup shortcut of fp32 operands
    "lin_g2": (2, 13, 11, 13, 11, (200, 200), 1, 1, 0, 2, 0, 0, True),
    "k3_g2":  (2, 13, 11, 13, 11, (24, 24), 3, 1, 1, 2, 0, 0, True),
}
VARIANTS = list(SHAPES)
UNSPLIT = ("tiny", "direct")
# kind -> (storage type of the operands, what the products are taken on (None: the operands as stored), KPF_DT_* name)
KINDS = {"f32": (torch.float32, None, "KPF_DT_F32"), "bf16": (torch.bfloat16, None, "KPF_DT_BF16"), "f16": (torch.float16, None, "KPF_DT_F16"),
         "r_bf16": (torch.float32, torch.bfloat16, "KPF_DT_F32_MMA_BF16"), "r_f16": (torch.float32, torch.float16, "KPF_DT_F32_MMA_F16")}


def _grads(x, dy, v, dt):
    """-> dw [G][n_valid][cin_valid][k][k], db [G][n_valid] in precision dt: torch's conv2d backward on the CPU, group by group (x, dy NHWC, the used channels)."""
    dws, dbs = [], []
    for g in range(v.G):
        xg = x[..., g * v.cin:g * v.cin + v.cin_valid].to(dt).permute(0, 3, 1, 2)
        dg = dy[..., g * N:g * N + v.n_valid].to(dt).permute(0, 3, 1, 2)
        w = torch.zeros(v.n_valid, v.cin_valid, v.k, v.k, dtype=dt, requires_grad=True)
        b = torch.zeros(v.n_valid, dtype=dt, requires_grad=True)
        y = F.conv2d(xg, w, b, stride=v.stride, padding=v.pad)
        assert y.shape == dg.shape, (y.shape, dg.shape)
        y.backward(dg)
        dws.append(w.grad)
        dbs.append(b.grad)
    return torch.stack(dws), torch.stack(dbs)


@functools.lru_cache(maxsize=None)
def variant(name, kind):
    """Operands (fp32 tensors holding storage-precision values), geometry and the float64 / plain-fp32 gradients; built once and left unchanged."""
    Bn, H, W, OH, OW, cins, k, s, p, G, cv, nv, want_db = SHAPES[name]
    tdt, round_to, dt_name = KINDS[kind]
    sixteen = tdt != torch.float32
    cin = cins[1] if sixteen else cins[0]
    v = SimpleNamespace(name=name, kind=kind, B=Bn, H=H, W=W, OH=OH, OW=OW, cin=cin, k=k, stride=s, pad=p, G=G, cin_valid=cv or cin, n_valid=nv or N,
                        want_db=want_db, tdt=tdt, dt_name=dt_name, M=Bn * OH * OW, K=k * k * cin, one=k == 1, trimmed=bool(cv or nv))
    al = 8 if sixteen or cin % 8 == 0 else 4
    v.ldx = (COFF + G * cin + 8 + al - 1) // al * al
    v.ldy = COFF + G * N + 8
    assert v.ldx > G * cin and v.ldy > G * N and v.ldx % al == 0 and v.ldy % 8 == 0 and (COFF * tdt.itemsize) % 16 == 0
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (name, kind)).encode()))
    q = lambda t: t.to(tdt).float()
    v.x = q(torch.randn(Bn, H, W, G * cin, generator=g))
    v.dy = q(torch.randn(Bn, OH, OW, G * N, generator=g))
    if v.trimmed:  # the operands carry zero channels behind the valid ones (include/kpf.h)
        v.x[..., v.cin_valid:] = 0
        v.dy[..., v.n_valid:] = 0
    # 16-bit storage: the operands as stored; KPF_DT_F32_MMA_*: the products are taken on the rounded operands, the bias gradient is the sum of dy as given
    xr, dyr = (v.x.to(round_to).float(), v.dy.to(round_to).float()) if round_to is not None else (v.x, v.dy)
    v.ref_dw, v.ref_db = _grads(xr, dyr, v, torch.float64)
    v.plain_dw, v.plain_db = _grads(xr, dyr, v, torch.float32)
    if round_to is not None:
        v.ref_db, v.plain_db = _grads(v.x, v.dy, v, torch.float64)[1], _grads(v.x, v.dy, v, torch.float32)[1]
    assert bool(torch.isfinite(v.ref_dw).all()) and float(v.ref_dw.abs().max()) > 1.0
    return v


def errors(v, dw, db):
    """-> {"dw": (e_kernel, e_plain), "db": ...}: both relative to max|ref64|"""
    out = {}
    for what, got, ref, plain in (("dw", dw, v.ref_dw, v.plain_dw), ("db", db, v.ref_db, v.plain_db)):
        if got is None:
            continue
        den = float(ref.abs().max())
        out[what] = (float((got.double() - ref).abs().max()) / den, float((plain.double() - ref).abs().max()) / den)
    return out


def within(ek, ep):
    return ek <= 4 * ep + FLOOR


def line(form, v, errs):
    """the record: form, variant, type, then e_kernel / e_plain of dw and of db"""
    s = "WGRAD %-8s %-7s %-6s" % (form, v.name, v.kind)
    for what in ("dw", "db"):
        if what in errs:
            ek, ep = errs[what]
            s += "  %s e_kernel %.3e e_plain %.3e%s" % (what, ek, ep, "" if within(ek, ep) else " MISSES")
    return s


# ----------------------------------------------------------------------------------------------------------------------------------------
# the device side
# ----------------------------------------------------------------------------------------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from keypointfusion_amd import lib
    lib.load()
    return torch.device("cuda:0")


def plan(v, groups=None):
    """kpf_conv2d_wgrad_plan for this variant under the force in effect (no device call)"""
    from keypointfusion_amd import lib as L
    p = L.WgradPlan()
    L.check(L.load().kpf_conv2d_wgrad_plan(getattr(L, v.dt_name), v.G if groups is None else groups, v.M, N, v.K, int(v.one), int(v.trimmed), C.byref(p)), "kpf_conv2d_wgrad_plan")
    return p


def family(p):
    from keypointfusion_amd import lib as L
    return L.KPF_WGRAD_FAMILY[p.family]


@functools.lru_cache(maxsize=None)
def _operands(name, kind):
    """the two wide rows on the device, NaN outside the slices"""
    v = variant(name, kind)
    d = dev()
    nan = float("nan")
    xb = torch.full((v.B * v.H * v.W, v.ldx), nan, dtype=v.tdt, device=d)
    yb = torch.full((v.M, v.ldy), nan, dtype=v.tdt, device=d)
    xb[:, COFF:COFF + v.G * v.cin] = v.x.reshape(-1, v.G * v.cin).to(v.tdt).to(d)
    yb[:, COFF:COFF + v.G * N] = v.dy.reshape(-1, v.G * N).to(v.tdt).to(d)
    return xb, yb


def _canaries(n, d):
    return torch.full((n + GUARD,), CANARY, dtype=torch.int32, device=d)


def _kept(t):
    return bool((t == CANARY).all())


def run(v, form=0, defer=False, group=None):
    """One call under kpf_conv2d_wgrad_force_form(form) on canary-filled dw / db / ws, ws at exactly the queried size.  group = g: group g of a channel-stacked variant as a
    call of its own on the channel slices.  defer: with a descriptor and kpf_wgrad_reduce_multi.  -> (dw, db or None, the plan) after the canary checks."""
    from keypointfusion_amd import lib as L
    lib = L.load()
    d = dev()
    xb, yb = _operands(v.name, v.kind)
    G = v.G if group is None else 1
    g0 = 0 if group is None else group
    es = v.tdt.itemsize
    n_dw, n_db = G * v.n_valid * v.cin_valid * v.k * v.k, G * v.n_valid
    L.check(lib.kpf_conv2d_wgrad_force_form(form), "kpf_conv2d_wgrad_force_form")
    try:
        p = plan(v, G)
        n_ws = G * p.ws_floats
        dw, db, ws = _canaries(n_dw, d), _canaries(n_db, d), _canaries(n_ws, d)
        desc = L.WgradReduceDesc()
        L.check(lib.kpf_conv2d_wgrad(yb.data_ptr() + (COFF + g0 * N) * es, xb.data_ptr() + (COFF + g0 * v.cin) * es, getattr(L, v.dt_name), dw.data_ptr(),
                                     db.data_ptr() if v.want_db else None, ws.data_ptr(), n_ws, G, v.B, v.H, v.W, v.cin, v.ldx, v.OH, v.OW, N, v.ldy, v.k, v.k,
                                     v.stride, v.stride, v.pad, v.pad, v.cin_valid if v.trimmed else 0, v.n_valid if v.trimmed else 0,
                                     C.byref(desc) if defer else None, torch.cuda.current_stream().cuda_stream), "kpf_conv2d_wgrad")
        if defer:
            assert (desc.kind < 0) == bool(p.writes_dw), (desc.kind, p.writes_dw)  # nothing pending exactly when the plan says the kernel writes dw itself
            if desc.kind >= 0:
                assert desc.S == p.S, (desc.S, p.S)
            arr = (L.WgradReduceDesc * 1)(desc)
            L.check(lib.kpf_wgrad_reduce_multi(arr, 1, torch.cuda.current_stream().cuda_stream), "kpf_wgrad_reduce_multi")
        torch.cuda.synchronize()
    finally:
        lib.kpf_conv2d_wgrad_force_form(0)
    tag = "%s/%s form %d" % (v.name, v.kind, form)
    assert _kept(dw[n_dw:]), tag + ": wrote behind dw"
    assert _kept(db[n_db:]) and (v.want_db or _kept(db)), tag + ": wrote behind db (or a db that was not asked for)"
    assert _kept(ws[n_ws:]), tag + ": wrote behind the workspace"
    if p.writes_dw:
        assert _kept(ws), tag + ": the direct form touched the workspace"
    dwf = dw[:n_dw].view(torch.float32).cpu().view(G, v.n_valid, v.cin_valid, v.k, v.k)
    dbf = db[:n_db].view(torch.float32).cpu().view(G, v.n_valid) if v.want_db else None
    assert bool(torch.isfinite(dwf).all()) and (dbf is None or bool(torch.isfinite(dbf).all())), tag + ": not finite (an unwritten output, or a pad column was read)"
    return dwf, dbf, p


def bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
