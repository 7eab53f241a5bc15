"""The train-mode BatchNorm kernels of csrc/kpf_wgrad.hip (section 3) — kpf_bn_train_*, kpf_bn2_add_relu_*, kpf_bn_relu_gmax_*, kpf_bn_ssr_* and the statistics,
finalize and elementwise kernels they share — each called through its C entry point on the tensors of tests/bn_cases.py and pinned to the float64 restatement there.

Tolerance: the rule of tests/test_fusion_head_kernels_gpu.py (whose helpers are used here), no constant invented —
    e_kernel = max|got - ref64| / max|ref64| <= 4 * e_plain + 8 * 2**-24,   e_plain: the same restatement in plain fp32 torch on the CPU,
over the whole tensor and, where a case plants channels, once more over the planted channels alone and over the others alone, the denominator floored at 2^-20 of
the tensor's.  y / dx in 16-bit storage: igemm_bounds.h16_excess(.., "rounding") against float64 on the stored operands.  Every comparison prints a line starting
with "ERR"; the table of one run on the MI355X is profiles/bn_kernel_errors.txt.  Winners and masks are compared for equality (tests/test_bn_cases_host.py asserts
that no entry lies inside a decision margin, and the regime of every case).

Every output and workspace starts as a NaN pattern and the workspace has exactly the size its query names: what a kernel owns must end finite; the guard row behind
the last row and the 64 elements behind every buffer must keep their bits.  Every call is made twice and must give the same bits.  A backward is given y / out /
arg, mean and invstd as the float64 reference rounded to fp32: it is judged on its own."""
import pytest
import torch

import bn_cases as BC
from igemm_bounds import PREC, h16_excess
from test_fusion_head_kernels_gpu import _bits, _call, _canary, _dev, _errs, _kept
from test_train_head_kernels_gpu import BYTE, GUARD, _errs_slice, _twice

pytestmark = pytest.mark.gpu

DT = {None: 0, "bf16": 1, "f16": 2}                    # KPF_DT_*
NAN16 = {"bf16": 0x7FC1, "f16": 0x7E01}                # a NaN of each 16-bit type


def _buf(dev, n, dt=None):
    """n + GUARD elements of the NaN pattern in the storage type dt."""
    if dt is None:
        return _canary(dev, n + GUARD)
    return torch.full((n + GUARD,), NAN16[dt], dtype=torch.int16, device=dev).view(BC.TORCH_DT[dt])


def _guard_kept(buf, n):
    if buf.dtype == torch.float32:
        return _kept(buf[n:])
    if buf.dtype == torch.uint8:
        return bool((buf[n:] == BYTE).all())
    pat = NAN16["bf16" if buf.dtype == torch.bfloat16 else "f16"]
    return bool((buf[n:].view(torch.int16) == pat).all())


def _rows(dev, rows, C, dt=None):
    """[rows][C] with a guard row and GUARD elements behind it -> (buffer, the [rows][C] view)."""
    buf = _buf(dev, (rows + 1) * C, dt)
    return buf, buf[:rows * C].view(rows, C)


def _ws(dev, lib_query, *args):
    from keypointfusion_amd import lib as L
    n = getattr(L.load(), lib_query)(*args)
    assert n > 0
    return _buf(dev, n), n


def _owned(what, *pairs):
    """pairs of (buffer, owned elements): the guards kept their bits, what the kernel owns is finite.  (kpf_bn_train_*: the workspace is owned too, the forward's part being all but the backward's 2 C
    coefficients; the fused forms' queries return the larger of two directions' needs, and there only the guard is looked at.)"""
    for i, (buf, n) in enumerate(pairs):
        assert _guard_kept(buf, n), "%s: buffer %d written behind its end" % (what, i)
        if buf.dtype != torch.uint8:
            assert bool(torch.isfinite(buf[:n].float()).all()), "%s: buffer %d not finite" % (what, i)


def _rule(label, got, ref, plain, planted=None):
    """The rule over the tensor, and with planted channels (the last dimension) over them alone and over the others alone.  A reference that is exactly 0: so is
    the kernel's."""
    got = got.detach().cpu()
    if float(ref.abs().max()) == 0:
        assert float(plain.abs().max()) == 0 and float(got.abs().max()) == 0, label + ": the reference is exactly 0"
        print("ERR %-64s exactly 0" % label)
        return
    _errs(label, got, ref, plain)
    if planted is not None and len(planted) < ref.shape[-1]:
        others = [i for i in range(ref.shape[-1]) if i not in set(planted)]
        _errs_slice(label + ", planted", got, ref, plain, (Ellipsis, planted))
        _errs_slice(label + ", the others", got, ref, plain, (Ellipsis, others))


def _h16(label, got, ref, dt):
    """16-bit storage: the stored values against float64, to the output rounding."""
    excess, _ = h16_excess(got.detach().cpu().double(), ref, PREC[dt][1], "rounding")
    print("ERR %-64s rounding bound %+.3e (%s)" % (label, excess, dt))
    assert excess <= 0, "%s: %.3e above the rounding bound of %s" % (label, excess, dt)


def _stored(label, got, ref, plain, dt, planted=None):
    if dt is None:
        _rule(label, got, ref, plain, planted)
    else:
        _h16(label, got, ref, dt)


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn_train_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
def _train_forward(dev, c, relu, running=True, xdt=None, ydt=None):
    M, C = c["x"].shape
    x, w, b = c["x"].to(dev), c["w"].to(dev), c["b"].to(dev)

    def run():
        ybuf, y = _rows(dev, M, C, ydt)
        mean, invstd = _buf(dev, C), _buf(dev, C)
        rm, rv = (_buf(dev, C), _buf(dev, C)) if running else (None, None)
        if running:
            rm[:C], rv[:C] = c["rm"].to(dev), c["rv"].to(dev)
        ws, nws = _ws(dev, "kpf_bn_ws_floats", M, C)
        _call("kpf_bn_train_forward", x, DT[xdt], w, b, y, DT[ydt], mean, invstd, rm, rv, BC.MOMENTUM, BC.EPS, relu, ws, nws, M, C)
        _owned("kpf_bn_train_forward", (ybuf, M * C), (mean, C), (invstd, C), (ws, nws - 2 * C), *(((rm, C), (rv, C)) if running else ()))
        assert _guard_kept(ws, nws)  # (the last 2 C floats are the backward's coefficients)
        return (y, mean[:C], invstd[:C]) + ((rm[:C], rv[:C]) if running else ())

    return _twice(run)


def _train_backward(dev, c, relu, with_addend=False, with_dwdb=True, xdt=None, ydt=None):
    M, C = c["x"].shape
    dy, x, y = c["dy"].to(dev), c["x"].to(dev), c["y_in"].to(dev) if relu else None
    mean, invstd, w = c["mean_in"].to(dev), c["invstd_in"].to(dev), c["w"].to(dev)
    addend = c["addend"].to(dev) if with_addend else None

    def run():
        dxbuf, dx = _rows(dev, M, C, xdt)
        dw, db = (_buf(dev, C), _buf(dev, C)) if with_dwdb else (None, None)
        ws, nws = _ws(dev, "kpf_bn_ws_floats", M, C)
        _call("kpf_bn_train_backward", dy, x, y, DT[xdt], DT[ydt], mean, invstd, w, addend, dx, dw, db, relu, ws, nws, M, C)
        _owned("kpf_bn_train_backward", (dxbuf, M * C), (ws, nws), *(((dw, C), (db, C)) if with_dwdb else ()))
        return (dx,) + ((dw[:C], db[:C]) if with_dwdb else ())

    return _twice(run)


@pytest.mark.parametrize("M,C,regime", BC.TRAIN_CASES)
def test_bn_train(M, C, regime):
    c = BC.train_case(M, C, regime)
    ref, plain, pl = c["ref"], c["plain"], c["planted"]
    dev = _dev()
    for relu in (0, 1):
        tag = "bn_train %dx%d %s relu=%d " % (M, C, regime, relu)
        y, mean, invstd, rm, rv = _train_forward(dev, c, relu)
        _rule(tag + "y", y, ref["y%d" % relu], plain["y%d" % relu], pl)
        if relu == 0:
            for name, got in (("mean", mean), ("invstd", invstd), ("rmean", rm), ("rvar", rv)):
                _rule(tag + name, got, ref[name], plain[name], pl)
            if regime == "constant":  # exactly constant: the mean is the constant and y the bias, to the bit
                for ch in pl:
                    assert float(mean[ch]) == float(c["x"][0, ch]) and bool((y[:, ch].cpu() == c["b"][ch]).all())
        y2, mean2, invstd2 = _train_forward(dev, c, relu, running=False)
        assert _bits(y, y2) and _bits(mean, mean2) and _bits(invstd, invstd2), "null running statistics change the batch's"
        dx, dw, db = _train_backward(dev, c, relu)
        for name, got in (("dx", dx), ("dw", dw), ("db", db)):
            _rule(tag + name, got, ref["%s%d" % (name, relu)], plain["%s%d" % (name, relu)], pl)
        assert _bits(dx, _train_backward(dev, c, relu, with_dwdb=False)[0]), "null dw / db change dx"
        dxa, dwa, dba = _train_backward(dev, c, relu, with_addend=True)
        _rule(tag + "dx + addend", dxa, ref["dxa%d" % relu], plain["dxa%d" % relu], pl)
        assert _bits(dw, dwa) and _bits(db, dba)


@pytest.mark.parametrize("xdt,ydt", BC.H16_PAIRS)
@pytest.mark.parametrize("M,C", BC.H16_SHAPES)
def test_bn_train_16bit_storage(M, C, xdt, ydt):
    c = BC.train_h16_case(M, C, xdt, ydt)
    ref, plain = c["ref"], c["plain"]
    dev = _dev()
    for relu in (0, 1):
        tag = "bn_train %dx%d x=%s y=%s relu=%d " % (M, C, xdt or "f32", ydt or "f32", relu)
        y, mean, invstd, rm, rv = _train_forward(dev, c, relu, xdt=xdt, ydt=ydt)
        _stored(tag + "y", y, ref["y%d" % relu], plain["y%d" % relu], ydt)
        if relu == 0:
            for name, got in (("mean", mean), ("invstd", invstd), ("rmean", rm), ("rvar", rv)):
                _rule(tag + name, got, ref[name], plain[name])
        for with_addend in (False, True):
            dx, dw, db = _train_backward(dev, c, relu, with_addend=with_addend, xdt=xdt, ydt=ydt)
            name = "dxa%d" % relu if with_addend else "dx%d" % relu
            _stored(tag + ("dx + addend" if with_addend else "dx"), dx, ref[name], plain[name], xdt)
        _rule(tag + "dw", dw, ref["dw%d" % relu], plain["dw%d" % relu])
        _rule(tag + "db", db, ref["db%d" % relu], plain["db%d" % relu])


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn2_add_relu_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
def _bn2_forward(dev, c, running=True):
    M, C = c["xa"].shape
    d = {k: c[k].to(dev) for k in ("xa", "xb", "wa", "ba", "wb", "bb")}

    def run():
        obuf, out = _rows(dev, M, C)
        stats = _buf(dev, 4 * C)
        rs = [_buf(dev, C) for _ in range(4)] if running else [None] * 4
        if running:
            for r, k in zip(rs, ("rma", "rva", "rmb", "rvb")):
                r[:C] = c[k].to(dev)
        ws, nws = _ws(dev, "kpf_bn2_ws_floats", M, C)
        _call("kpf_bn2_add_relu_forward", d["xa"], d["xb"], d["wa"], d["ba"], d["wb"], d["bb"], out, stats, *rs, BC.MOMENTUM, BC.EPS, ws, nws, M, C)
        _owned("kpf_bn2_add_relu_forward", (obuf, M * C), (stats, 4 * C), *([(r, C) for r in rs] if running else []))
        assert _guard_kept(ws, nws)
        return (out, stats[:4 * C].view(4, C)) + (tuple(r[:C] for r in rs) if running else ())

    return _twice(run)


@pytest.mark.parametrize("M,C", BC.BN2_SHAPES)
def test_bn2_add_relu(M, C):
    c = BC.bn2_case(M, C)
    ref, plain = c["ref"], c["plain"]
    dev = _dev()
    tag = "bn2_add_relu %dx%d " % (M, C)
    out, stats, *rs = _bn2_forward(dev, c)
    _rule(tag + "out", out, ref["out"], plain["out"])
    assert bool(torch.equal(out.cpu() > 0, c["mask"])), "a ReLU decision outside every margin"
    _rule(tag + "stats", stats, ref["stats"], plain["stats"])
    for got, name in zip(rs, ("rma", "rva", "rmb", "rvb")):
        _rule(tag + name, got, ref[name], plain[name])
    out2, stats2 = _bn2_forward(dev, c, running=False)
    assert _bits(out, out2) and _bits(stats, stats2), "null running statistics change the batch's"
    d = {k: c[k].to(dev) for k in ("dy", "out_in", "xa", "xb", "stats_in", "wa", "wb")}

    def bwd():
        (abuf, dxa), (bbuf, dxb) = _rows(dev, M, C), _rows(dev, M, C)
        vec = [_buf(dev, C) for _ in range(4)]
        ws, nws = _ws(dev, "kpf_bn2_ws_floats", M, C)
        _call("kpf_bn2_add_relu_backward", d["dy"], d["out_in"], d["xa"], d["xb"], d["stats_in"], d["wa"], d["wb"], dxa, dxb, *vec, ws, nws, M, C)
        _owned("kpf_bn2_add_relu_backward", (abuf, M * C), (bbuf, M * C), *[(v, C) for v in vec])
        assert _guard_kept(ws, nws)
        return (dxa, dxb) + tuple(v[:C] for v in vec)

    for got, name in zip(_twice(bwd), ("dxa", "dxb", "dwa", "dba", "dwb", "dbb")):
        _rule(tag + name, got, ref[name], plain[name])


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn_relu_gmax_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
def _gmax_forward(dev, c, G, group, C, running=True):
    M = G * group
    x, w, b = c["x"].to(dev), c["w"].to(dev), c["b"].to(dev)

    def run():
        ybuf, y = _rows(dev, G, C)
        abuf = torch.full(((G + 1) * C + GUARD,), BYTE, dtype=torch.uint8, device=dev)
        stats = _buf(dev, 2 * C)
        rm, rv = (_buf(dev, C), _buf(dev, C)) if running else (None, None)
        if running:
            rm[:C], rv[:C] = c["rm"].to(dev), c["rv"].to(dev)
        ws, nws = _ws(dev, "kpf_bn_relu_gmax_ws_floats", M, C)
        _call("kpf_bn_relu_gmax_forward", x, w, b, y, abuf, stats, rm, rv, BC.MOMENTUM, BC.EPS, ws, nws, M, group, C)
        _owned("kpf_bn_relu_gmax_forward", (ybuf, G * C), (abuf, G * C), (stats, 2 * C), *(((rm, C), (rv, C)) if running else ()))
        assert _guard_kept(ws, nws)
        return (y, abuf[:G * C].view(G, C), stats[:2 * C].view(2, C)) + ((rm[:C], rv[:C]) if running else ())

    return _twice(run)


@pytest.mark.parametrize("G,group,C,ld", BC.GMAX_SHAPES)
def test_bn_relu_gmax(G, group, C, ld):
    c = BC.gmax_case(G, group, C, ld)
    ref, plain = c["ref"], c["plain"]
    M = G * group
    dev = _dev()
    tag = "bn_relu_gmax G=%d group=%d C=%d ld=%d " % (G, group, C, ld)
    y, arg, stats, rm, rv = _gmax_forward(dev, c, G, group, C)
    assert bool(torch.equal(arg.cpu(), c["arg"])), "winners (the first maximum; member 0 where no member is positive)"
    assert bool(torch.equal(y.cpu() > 0, c["mask"]))
    for name, got in (("y", y), ("stats", stats), ("rmean", rm), ("rvar", rv)):
        _rule(tag + name, got, ref[name], plain[name])
    y2, arg2, stats2 = _gmax_forward(dev, c, G, group, C, running=False)
    assert _bits(y, y2) and bool(torch.equal(arg, arg2)) and _bits(stats, stats2), "null running statistics change the batch's"
    dmax = _canary(dev, G, ld)  # the pad columns of the wider matrix are NaN: not read
    dmax[:, :C] = c["dmax"][:, :C].to(dev)
    d = {k: c[k].to(dev) for k in ("y_in", "arg", "x", "stats_in", "w")}

    def bwd():
        dxbuf, dx = _rows(dev, M, C)
        dw, db = _buf(dev, C), _buf(dev, C)
        ws, nws = _ws(dev, "kpf_bn_relu_gmax_ws_floats", M, C)
        _call("kpf_bn_relu_gmax_backward", dmax, ld, d["y_in"], d["arg"], d["x"], d["stats_in"], d["w"], dx, dw, db, ws, nws, M, group, C)
        _owned("kpf_bn_relu_gmax_backward", (dxbuf, M * C), (dw, C), (db, C))
        assert _guard_kept(ws, nws)
        return dx, dw[:C], db[:C]

    for got, name in zip(_twice(bwd), ("dx", "dw", "db")):
        _rule(tag + name, got, ref[name], plain[name])


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn_ssr_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
def _ssr_forward(dev, c, running=True):
    rows, C, n1, n2 = c["shape"]
    nC = (n1 + n2) * C
    x, w, b = c["x"].to(dev), c["w"].to(dev), c["b"].to(dev)

    def run():
        obuf, out = _rows(dev, rows, C)
        stats = _buf(dev, 2 * nC)
        rm, rv = (_buf(dev, nC), _buf(dev, nC)) if running else (None, None)
        if running:
            rm[:nC], rv[:nC] = c["rm"].to(dev), c["rv"].to(dev)
        ws, nws = _ws(dev, "kpf_bn_ssr_ws_floats", rows, C, n1 + n2)
        _call("kpf_bn_ssr_forward", x, w, b, out, stats, rm, rv, BC.MOMENTUM, BC.EPS, ws, nws, rows, C, n1, n2)
        _owned("kpf_bn_ssr_forward", (obuf, rows * C), (stats, 2 * nC), *(((rm, nC), (rv, nC)) if running else ()))
        assert _guard_kept(ws, nws)
        return (out, stats[:2 * nC].view(2, nC)) + ((rm[:nC], rv[:nC]) if running else ())

    return _twice(run)


@pytest.mark.parametrize("rows,C,n1,n2", BC.SSR_SHAPES)
def test_bn_ssr(rows, C, n1, n2):
    c = BC.ssr_case(rows, C, n1, n2)
    ref, plain = c["ref"], c["plain"]
    nC = (n1 + n2) * C
    dev = _dev()
    tag = "bn_ssr rows=%d C=%d n1=%d n2=%d " % (rows, C, n1, n2)
    out, stats, rm, rv = _ssr_forward(dev, c)
    assert bool(torch.equal(out.cpu() > 0, c["masks"][0])), "a ReLU decision outside every margin"
    for name, got in (("out", out), ("stats", stats), ("rmean", rm), ("rvar", rv)):
        _rule(tag + name, got, ref[name], plain[name])
    out2, stats2 = _ssr_forward(dev, c, running=False)
    assert _bits(out, out2) and _bits(stats, stats2), "null running statistics change the batch's"
    d = {k: c[k].to(dev) for k in ("dout", "out_in", "x", "stats_in", "w", "b")}

    def bwd():
        dxbuf, dx = _rows(dev, rows, nC)
        dw, db = _buf(dev, nC), _buf(dev, nC)
        ws, nws = _ws(dev, "kpf_bn_ssr_ws_floats", rows, C, n1 + n2)
        _call("kpf_bn_ssr_backward", d["dout"], d["out_in"], d["x"], d["stats_in"], d["w"], d["b"], dx, dw, db, ws, nws, rows, C, n1, n2)
        _owned("kpf_bn_ssr_backward", (dxbuf, rows * nC), (dw, nC), (db, nC))
        assert _guard_kept(ws, nws)
        return dx, dw[:nC], db[:nC]

    dx, dw, db = _twice(bwd)
    _rule(tag + "dx", dx, ref["dx"], plain["dx"])
    for k in range(n1 + n2):  # every slice on its own
        _errs_slice(tag + "dx, slice %d" % k, dx, ref["dx"], plain["dx"], (slice(None), slice(k * C, (k + 1) * C)))
    _rule(tag + "dw", dw, ref["dw"], plain["dw"])
    _rule(tag + "db", db, ref["db"], plain["db"])


# ----------------------------------------------------------------------------------------------------------------------------------------
# one set of statistics kernels under the four forms
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,regime", [(777, 48, "ordinary"), (1603, 256, "outlier"), (515, 576, "ordinary"), (16400, 256, "ordinary")])
def test_batch_statistics_are_the_same_bits_in_every_form(M, C, regime):
    """kpf_bn_train_forward, kpf_bn2_add_relu_forward (both branches), kpf_bn_relu_gmax_forward and kpf_bn_ssr_forward (C <= 256) on the same x: the batch mean and
    invstd are bit-identical, and so are the running statistics."""
    c = BC.train_case(M, C, regime)
    dev = _dev()
    _, mean, invstd, rm, rv = _train_forward(dev, c, 0)
    two = dict(xa=c["x"], xb=c["x"], wa=c["w"], ba=c["b"], wb=c["w"], bb=c["b"], rma=c["rm"], rva=c["rv"], rmb=c["rm"], rvb=c["rv"])
    _, stats, rma, rva, rmb, rvb = _bn2_forward(dev, two)
    assert _bits(stats[0], mean) and _bits(stats[1], invstd) and _bits(stats[2], mean) and _bits(stats[3], invstd)
    assert _bits(rma, rm) and _bits(rva, rv) and _bits(rmb, rm) and _bits(rvb, rv)
    _, _, stats, rmg, rvg = _gmax_forward(dev, c, M, 1, C)
    assert _bits(stats[0], mean) and _bits(stats[1], invstd) and _bits(rmg, rm) and _bits(rvg, rv)
    if C <= 256:
        _, stats, rms, rvs = _ssr_forward(dev, dict(c, shape=(M, C, 1, 0)))
        assert _bits(stats[0], mean) and _bits(stats[1], invstd) and _bits(rms, rm) and _bits(rvs, rv)
