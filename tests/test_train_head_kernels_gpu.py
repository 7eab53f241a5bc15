"""The training-side fusion-head kernels of csrc/kpf_train.hip, and kpf_ball_group_stacked_f32 of csrc/kpf_geom.hip, each called through its C entry point on
tensors built in tests/train_head_cases.py and pinned to the float64 restatement there: kpf_joint_heatmap_*, kpf_geom_gate_*, kpf_geom_gate_uvd_*,
kpf_pose_tokens_f32, kpf_gate_mix_*, kpf_group_max_train_*, kpf_ball_group_stacked_f32, kpf_ball_group_bwd_f32, kpf_row_gather_{fwd,cols,invert,accum,bwd},
kpf_attn21_*.

Tolerance: the rule of tests/test_fusion_head_kernels_gpu.py (whose helpers are used here), no constant invented —
    e_kernel = max|got - ref64| / max|ref64| <= 4 * e_plain + 8 * 2**-24,   e_plain: the same restatement in plain fp32 torch on the CPU,
over the whole output tensor, and once more over the planted entries alone with the denominator floored at 2^-20 of the tensor's (`_errs_slice`).  Every comparison
prints a line starting with "ERR"; the table of one run on the MI355X is profiles/train_head_kernel_errors.txt.  Integers, masks, copies and zero pads are compared
for equality.  Mask decisions are compared where the float64 margin exceeds the distance stated in the case (tests/test_train_head_cases_host.py asserts that this
leaves out at most 1 %, and the regime of every case).

Every output, workspace and guard starts as the NaN pattern 0x7FC0BEEF (bytes: 0xA5): what a kernel owns must end finite, the guard row behind the last row, the
columns outside the kernel's slice and the 64 elements behind each buffer must keep their bits; input pads a kernel must not read are that NaN.  Every backward is
called twice and must give the same bits."""
import math

import pytest
import torch

import train_head_cases as TC
from test_fusion_head_kernels_gpu import CANARY, FLOOR, _bits, _call, _canary, _dev, _errs, _kept

pytestmark = pytest.mark.gpu

GUARD = 64
BYTE = 0xA5


def _errs_slice(label, got, ref, plain, sel):
    """The rule over the planted entries `sel` alone."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and plain.dtype == torch.float32 and bool(torch.isfinite(got[sel]).all()), label + ": not finite"
    ek, ep = TC.rel_err(got, ref, sel), TC.rel_err(plain, ref, sel)
    print("ERR %-64s e_kernel %.3e  e_plain %.3e" % (label, ek, ep))
    assert ek <= 4 * ep + FLOOR, "%s: e_kernel %.3e > 4 * e_plain (%.3e) + 8 * 2^-24" % (label, ek, ep)


def _flat(dev, *shape):
    """A canary buffer of `shape` with GUARD canary elements behind it -> (the whole buffer, its view of `shape`)."""
    n = math.prod(shape)
    buf = _canary(dev, n + GUARD)
    return buf, buf[:n].view(*shape)


def _rows(dev, rows, ld):
    """[rows + 1][ld] (a guard row) + GUARD -> (the whole buffer, the 2-d view with the guard row, what lies behind the last row)."""
    buf = _canary(dev, (rows + 1) * ld + GUARD)
    return buf, buf[:(rows + 1) * ld].view(rows + 1, ld), buf[rows * ld:]


def _padded(dev, t, ld):
    """t [rows][C] at row stride ld, the pad columns NaN."""
    rows, C = t.shape
    buf = _canary(dev, rows, ld)
    buf[:, :C] = t.to(dev)
    return buf


def _ints(dev, n):
    return torch.full((n + GUARD,), CANARY, dtype=torch.int32, device=dev)


def _bytes(dev, n):
    return torch.full((n + GUARD,), BYTE, dtype=torch.uint8, device=dev)


def _twice(run):
    """run() -> tuple of device tensors, on fresh canary buffers each time: the second call's bits equal the first's."""
    a, b = run(), run()
    assert all(_bits(x, y) for x, y in zip(a, b)), "two calls on the same operands differ"
    return a


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. kpf_joint_heatmap_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std,sigma", TC.HEATMAP_STD_SIGMA)
@pytest.mark.parametrize("B,J,Fs", TC.HEATMAP_SHAPES)
def test_joint_heatmap(B, J, Fs, std, sigma):
    c = TC.heatmap_case(B, J, Fs, std, sigma)
    dev = _dev()
    uvd, dhm = c["uvd"].to(dev), c["dhm"].to(dev)
    buf, hm = _flat(dev, B, J, Fs, Fs)
    _call("kpf_joint_heatmap_forward", uvd, hm, B, J, Fs, std, sigma)
    assert _kept(buf[hm.numel():]), "wrote past the last map"
    tag = "joint_heatmap B=%d J=%d F=%d std=%g sigma=%g " % (B, J, Fs, std, sigma)
    _errs(tag + "hm", hm, c["ref"]["hm"], c["plain"]["hm"])

    def bwd():
        buf, duvd = _flat(dev, B, J, 3)
        _call("kpf_joint_heatmap_backward", uvd, dhm, duvd, B, J, Fs, std, sigma)
        assert _kept(buf[duvd.numel():]), "wrote past the last joint"
        return (duvd,)

    duvd = _twice(bwd)[0]
    assert bool((duvd[..., 2] == 0).all())
    _errs(tag + "duvd", duvd, c["ref"]["duvd"], c["plain"]["duvd"])
    for name in ("centre", "border", "off", "far"):
        sel = (slice(None), c[name])
        _errs_slice(tag + "hm, joint %s" % name, hm, c["ref"]["hm"], c["plain"]["hm"], sel)
        _errs_slice(tag + "duvd, joint %s" % name, duvd, c["ref"]["duvd"], c["plain"]["duvd"], sel)
    if c["underflows"]:
        assert bool((hm[:, c["far"]] == 0).all()) and bool((duvd[:, c["far"]] == 0).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. kpf_geom_gate_forward / _backward, kpf_geom_gate_uvd_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
def _gate_checks(tag, c, gam, dj, dname, J, P):
    _errs(tag + "gam", gam, c["ref"]["gam"], c["plain"]["gam"])
    _errs(tag + dname, dj, c["ref"][dname], c["plain"][dname])
    if c["planted"]:
        for what, sel, jsel in (("the pixel on joint 0", (slice(None), 0, 0), (slice(None), 0)), ("the pixel at distance 30", (slice(None), J - 1, P - 1), (slice(None), J - 1))):
            _errs_slice(tag + "gam, " + what, gam, c["ref"]["gam"], c["plain"]["gam"], sel)
            _errs_slice(tag + dname + ", its joint", dj, c["ref"][dname], c["plain"][dname], jsel)


@pytest.mark.parametrize("B,J,P", TC.GATE_SHAPES)
def test_geom_gate(B, J, P):
    c = TC.geom_gate_case(B, J, P)
    dev = _dev()
    pix, joint, dgam = (c[k].to(dev) for k in ("pix", "joint", "dgam"))
    buf, gam = _flat(dev, B, J, P)
    _call("kpf_geom_gate_forward", pix, joint, gam, B, J, P)
    assert _kept(buf[gam.numel():]), "wrote past the last pixel"
    if c["planted"]:
        assert bool((gam[:, 0, 0] == 1.0).all())

    def bwd():
        buf, dj = _flat(dev, B, J, 3)
        _call("kpf_geom_gate_backward", pix, joint, dgam, dj, B, J, P)
        assert _kept(buf[dj.numel():]), "wrote past the last joint"
        return (dj,)

    _gate_checks("geom_gate B=%d J=%d P=%d " % (B, J, P), c, gam, _twice(bwd)[0], "djoint", J, P)


@pytest.mark.parametrize("half_size", [64.0, 128.0])
@pytest.mark.parametrize("flip", [1.0, -1.0])
@pytest.mark.parametrize("B,J,P", TC.GATE_SHAPES)
def test_geom_gate_uvd(B, J, P, flip, half_size):
    c = TC.geom_gate_uvd_case(B, J, P, flip, half_size)
    dev = _dev()
    pix, uvd, dgam, par = (c[k].to(dev) for k in ("pix", "uvd", "dgam", "par"))
    buf, gam = _flat(dev, B, J, P)
    _call("kpf_geom_gate_uvd_forward", pix, uvd, par, gam, B, J, P, half_size, flip)
    assert _kept(buf[gam.numel():]), "wrote past the last pixel"

    def bwd():
        buf, dj = _flat(dev, B, J, 3)
        _call("kpf_geom_gate_uvd_backward", pix, uvd, par, dgam, dj, B, J, P, half_size, flip)
        assert _kept(buf[dj.numel():]), "wrote past the last joint"
        return (dj,)

    _gate_checks("geom_gate_uvd B=%d J=%d P=%d flip=%+d half=%d " % (B, J, P, flip, half_size), c, gam, _twice(bwd)[0], "duvd", J, P)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. kpf_pose_tokens_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0.8, 0.6])
@pytest.mark.parametrize("B,N,J,ld,with_pw", TC.POSE_SHAPES)
def test_pose_tokens(B, N, J, ld, with_pw, kernel):
    c = TC.pose_case(B, N, J, kernel)
    dev = _dev()
    buf, out, behind = _rows(dev, B * N, ld)
    _call("kpf_pose_tokens_f32", c["pw"].to(dev) if with_pw else None, c["joint"].to(dev), c["pcl"].to(dev), out, B, N, J, ld, kernel)
    assert _kept(behind), "wrote past the last point"
    o = out[:B * N].cpu().view(B, N, ld)
    assert bool(torch.isfinite(o).all())
    base = J if with_pw else 0
    if with_pw:
        assert _bits(o[..., :J], c["pw"]), "the weight logits are a copy"
    assert bool((o[..., base + 4 * J:] == 0).all()), "zero pad"
    off = o[..., base:base + 4 * J]
    cmp_, keep = c["compared"], c["keep"]
    assert torch.equal(c["mask_of"](off)[cmp_], c["mask64"][cmp_]), "mask decisions (left out: %.4f %% of the entries)" % (100 * c["left_out"])
    z = lambda t: torch.where(keep, t, torch.zeros_like(t))
    tag = "pose_tokens B=%d N=%d J=%d ld=%d pw=%d r=%.1f " % (B, N, J, ld, with_pw, kernel)
    _errs(tag + "offsets+closeness", z(off), z(c["ref"]["off"]), z(c["plain"]["off"]))
    planted = torch.zeros(B, N, 4 * J, dtype=torch.bool)
    for b, n, j in c["inside"] + c["outside"] + c["on_joint"]:
        planted[b, n, 3 * j:3 * j + 3] = True
        planted[b, n, 3 * J + j] = True
    for b, n in c["z_masked"] + c["z_kept"]:
        planted[b, n] = True
    _errs_slice(tag + "planted ring / joint / z entries", off, c["ref"]["off"], c["plain"]["off"], planted)
    for b, n, j in c["on_joint"]:
        assert float(off[b, n, 3 * J + j]) == 1.0 and not bool(off[b, n, 3 * j:3 * j + 3].any()), "a point on a joint"
    for b, n in c["z_masked"]:
        assert not bool(off[b, n].any()), "z >= 0.99 masks the point"
    for b, n in c["z_kept"]:
        assert float(off[b, n, 3 * J + c["z_joint"]]) > 0.3, "z just below 0.99 is kept"


# ----------------------------------------------------------------------------------------------------------------------------------------
# 5. kpf_gate_mix_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,J,P,wdis,with_dsw", TC.GATE_MIX_CASES)
def test_gate_mix(B, J, P, wdis, with_dsw):
    c = TC.gate_mix_case(B, J, P, wdis, with_dsw)
    dev = _dev()
    logits, gam, wd, w_fc, d_gw, sw_in = (c[k].to(dev) for k in ("logits", "gam", "wd", "w_fc", "d_gw", "sw_in"))
    d_sw = c["d_sw"].to(dev) if with_dsw else None
    (bs, sw), (bg, gw) = _flat(dev, B, J, P), _flat(dev, B, J, P)
    _call("kpf_gate_mix_forward", logits, gam, wd, w_fc, sw, gw, B, J, P)
    assert _kept(bs[sw.numel():]) and _kept(bg[gw.numel():]), "wrote past the last pixel"
    tag = "gate_mix B=%d J=%d P=%d weight_dis=%g d_sw=%d " % (B, J, P, wdis, with_dsw)
    ref, plain = c["ref"], c["plain"]
    _errs(tag + "sw", sw, ref["sw"], plain["sw"])
    _errs(tag + "gw", gw, ref["gw"], plain["gw"])
    sat = c["saturated"]
    sat_bjp = sat.view(B, P, J).permute(0, 2, 1)
    _errs_slice(tag + "sw, saturated", sw, ref["sw"], plain["sw"], sat_bjp)

    def bwd():
        outs = [_flat(dev, B, J, P), _flat(dev, B * P, J), _flat(dev, P), _flat(dev, 1), _flat(dev, B * J)]
        _call("kpf_gate_mix_backward", sw_in, gam, wd, w_fc, d_sw, d_gw, *[v for _, v in outs], B, J, P)
        assert all(_kept(b[v.numel():]) for b, v in outs), "wrote past the end of an output"
        assert bool(torch.isfinite(outs[4][1]).all()), "workspace"
        return tuple(v for _, v in outs[:4])

    got = dict(zip(("d_gam", "d_logits", "d_w_fc", "d_weight_dis"), _twice(bwd)))
    for name, g in got.items():
        _errs(tag + name, g, ref[name], plain[name])
    _errs_slice(tag + "d_logits, saturated", got["d_logits"], ref["d_logits"], plain["d_logits"], sat)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 6. kpf_group_max_train_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,group,C,dy_ld", TC.GROUP_MAX_SHAPES)
def test_group_max_train(rows, group, C, dy_ld):
    c = TC.group_max_case(rows, group, C)
    dev = _dev()
    x = c["x"].to(dev)
    by, y = _flat(dev, rows, C)
    arg = _bytes(dev, rows * C)
    _call("kpf_group_max_train_forward", x, y, arg, rows, group, C)
    assert _kept(by[rows * C:]) and bool((arg[rows * C:] == BYTE).all()), "wrote past the last row"
    assert _bits(y.cpu(), c["y"]), "y is the maximum, bit for bit"
    assert torch.equal(arg[:rows * C].cpu().view(rows, C), c["arg"]), "arg is the first index of the maximum"
    dy = _padded(dev, c["dy"], dy_ld)  # the pad columns behind C are NaN: never read

    def bwd():
        bx, dx = _flat(dev, rows, group, C)
        _call("kpf_group_max_train_backward", dy, dy_ld, arg, dx, rows, group, C)
        assert _kept(bx[dx.numel():]), "wrote past the last row"
        return (dx,)

    assert _bits(_twice(bwd)[0].cpu(), c["dx"]), "dx: dy at the winner, +0 elsewhere"
    print("ERR %-64s bit-equal (y, arg, dx)" % ("group_max_train rows=%d group=%d C=%d dy_ld=%d" % (rows, group, C, dy_ld)))


# ----------------------------------------------------------------------------------------------------------------------------------------
# 7. kpf_ball_group_stacked_f32, kpf_ball_group_bwd_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", TC.BALL_NS)
def test_ball_group_stacked(N):
    c = TC.ball_group_case(N)
    dev = _dev()
    B, J = c["B"], TC.BALL_J
    rows = B * J * 64
    JF = _padded(dev, c["JF"].view(B * J, 128), 132)
    (bf, GF, behind_f), (bx, GX, behind_x) = _rows(dev, rows, 384), _rows(dev, rows, 12)
    idx = _ints(dev, 3 * rows)
    _call("kpf_ball_group_stacked_f32", c["pcl"].to(dev), c["joint"].to(dev), c["X"].to(dev), JF, 132, GF, GX, idx, B, N, *TC.RADII)
    assert _kept(behind_f) and _kept(behind_x) and bool((idx[3 * rows:] == CANARY).all()), "wrote past the last row"
    assert torch.equal(idx[:3 * rows].cpu().view(3, B, J, 64), c["idx"]), "index sets (no pair within %.0e of a radius: margin %.2e)" % (TC.BALL_MARGIN, c["margin"])
    tag = "ball_group_stacked B=%d N=%d " % (B, N)
    _errs(tag + "GF", GF[:rows], c["ref"]["GF"], c["plain"]["GF"])
    _errs(tag + "GX", GX[:rows], c["ref"]["GX"], c["plain"]["GX"])
    assert bool((GX[:rows, 3::4] == 0).all()), "the fourth offset channel is 0"
    own = torch.zeros(B, J, 64, dtype=torch.bool)
    own[:, :3] = True  # the lonely joint, the crowded one, the one with points next to each radius
    _errs_slice(tag + "GX, balls of joints 0..2", GX[:rows], c["ref"]["GX"], c["plain"]["GX"], own.view(rows))


@pytest.mark.parametrize("ld3", TC.BALL_BWD_LD3)
def test_ball_group_bwd(ld3):
    from keypointfusion_amd import lib as L
    c = TC.ball_bwd_case(ld3)
    dev = _dev()
    B, N, Jn, P, R = (c[k] for k in ("B", "N", "Jn", "P", "R"))
    idx = c["idx"].to(dev)
    nws = int(L.load().kpf_row_gather_ws_ints(3 * B, P, R, 1))
    assert nws == 3 * B * (P + 1) + 3 * B * R
    ws = _ints(dev, nws)
    _call("kpf_row_gather_invert", idx, ws, nws, 3 * B, P, R, 1)
    assert bool((ws[nws:] == CANARY).all()), "the inversion wrote past its workspace"
    start, lst = ws[:3 * B * (P + 1)], ws[3 * B * (P + 1):nws]
    s_ref, l_ref = TC.stable_inverse(c["idx"].view(3 * B, R), P)
    assert torch.equal(start.cpu().view(3 * B, P + 1), s_ref) and torch.equal(lst.cpu().view(3 * B, R), l_ref), "start / list: a stable sort by source row"
    d3 = _padded(dev, c["d3"], ld3)

    def bwd():
        (bx, dX), (bn, dnode) = _flat(dev, B, N, 128), _flat(dev, B, Jn, 128)
        _call("kpf_ball_group_bwd_f32", d3, ld3, start, lst, dX, dnode, B, N, Jn)
        assert _kept(bx[dX.numel():]) and _kept(bn[dnode.numel():]), "wrote past the last row"
        return dX, dnode

    dX, dnode = _twice(bwd)
    tag = "ball_group_bwd ld3=%d " % ld3
    _errs(tag + "dX", dX, c["ref"]["dX"], c["plain"]["dX"])
    _errs(tag + "dnode", dnode, c["ref"]["dnode"], c["plain"]["dnode"])
    total = c["counts"].sum(0)  # [B][P]
    for b in range(B):  # the heaviest point row and the heaviest joint row of each sample, and the lightest point row
        hp, hj, lp = int(total[b, :N].argmax()), int(total[b, N:].argmax()), int(total[b, :N].argmin())
        _errs_slice(tag + "dX, sample %d row %d (%d entries)" % (b, hp, total[b, hp]), dX, c["ref"]["dX"], c["plain"]["dX"], (b, hp))
        _errs_slice(tag + "dX, sample %d row %d (%d entries)" % (b, lp, total[b, lp]), dX, c["ref"]["dX"], c["plain"]["dX"], (b, lp))
        _errs_slice(tag + "dnode, sample %d joint %d (%d entries)" % (b, hj, total[b, N + hj]), dnode, c["ref"]["dnode"], c["plain"]["dnode"], (b, hj))


# ----------------------------------------------------------------------------------------------------------------------------------------
# 8. kpf_row_gather_fwd_f32, _cols_f32, _invert, _accum_f32, _bwd_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,R,G,C,with_w", TC.GATHER_CASES)
def test_row_gather(B, P, R, G, C, with_w):
    from keypointfusion_amd import lib as L
    c = TC.gather_case(B, P, R, G, C, with_w)
    dev = _dev()
    E = R * G
    src, idx, dout = (c[k].to(dev) for k in ("src", "idx", "dout"))
    w = c["w"].to(dev) if with_w else None
    tag = "row_gather B=%d P=%d R=%d G=%d C=%d w=%d " % (B, P, R, G, C, with_w)
    bo, out = _flat(dev, B, R, C)
    _call("kpf_row_gather_fwd_f32", src, idx, w, out, B, P, R, G, C)
    assert _kept(bo[out.numel():]), "forward wrote past the last row"
    _errs(tag + "out", out, c["ref"]["out"], c["plain"]["out"])
    nws = int(L.load().kpf_row_gather_ws_ints(B, P, R, G))
    assert nws == B * (P + 1) + B * E
    ws = _ints(dev, nws)
    _call("kpf_row_gather_invert", idx, ws, nws, B, P, R, G)
    assert bool((ws[nws:] == CANARY).all()), "the inversion wrote past its workspace"
    start, lst = ws[:B * (P + 1)], ws[B * (P + 1):nws]
    assert torch.equal(start.cpu().view(B, P + 1), c["start"]) and torch.equal(lst.cpu().view(B, E), c["list"]), "start / list: a stable sort by source row"

    def accum():
        bd, dsrc = _flat(dev, B, P, C)
        _call("kpf_row_gather_accum_f32", dout, start, lst, w, dsrc, B, P, R, G, C)
        assert _kept(bd[dsrc.numel():]), "accumulation wrote past the last row"
        return (dsrc,)

    def bwd():
        bd, dsrc = _flat(dev, B, P, C)
        ws2 = _ints(dev, nws)
        _call("kpf_row_gather_bwd_f32", dout, idx, w, dsrc, ws2, nws, B, P, R, G, C)
        assert _kept(bd[dsrc.numel():]) and torch.equal(ws2, ws), "backward: guard, or another inversion"
        return (dsrc,)

    dsrc = _twice(accum)[0]
    assert _bits(_twice(bwd)[0], dsrc), "bwd is invert + accum, bit for bit"
    _errs(tag + "dsrc", dsrc, c["ref"]["dsrc"], c["plain"]["dsrc"])
    assert bool((dsrc.cpu()[c["counts"] == 0] == 0).all()), "a row that owns nothing is +0"
    heavy = int(c["counts"][B - 1].argmax())
    for what, sel in (("last row", (slice(None), P - 1)), ("row %d of the last sample (%d entries)" % (heavy, c["counts"][B - 1, heavy]), (B - 1, heavy))):
        _errs_slice(tag + "dsrc, " + what, dsrc, c["ref"]["dsrc"], c["plain"]["dsrc"], sel)


@pytest.mark.parametrize("with_w", [True, False])
def test_row_gather_cols(with_w):
    c = TC.gather_cols_case(with_w)
    B, P, R, G, C = TC.GATHER_COLS
    dev = _dev()
    bo, out = _flat(dev, B, R, C)
    _call("kpf_row_gather_cols_f32", c["planes"].to(dev), C * P, 1, P, c["idx"].to(dev), c["w"].to(dev) if with_w else None, out, B, P, R, G, C)
    assert _kept(bo[out.numel():]), "wrote past the last row"
    _errs("row_gather_cols NCHW B=%d P=%d R=%d G=%d C=%d w=%d" % (B, P, R, G, C, with_w), out, c["ref"]["out"], c["plain"]["out"])


# ----------------------------------------------------------------------------------------------------------------------------------------
# 9. kpf_attn21_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
T_, HD = TC.ATTN_T, TC.ATTN_HD


def _attn_operands(dev, c, B, H, ld, ldc):
    """q, k, v at row stride ld: column slices of one [rows][3 C] buffer when ld == 3 C, dense tensors otherwise; dctx at row stride ldc with NaN pads."""
    rows, C = B * T_, H * HD
    if ld == 3 * C:
        qkv = torch.cat((c["q"], c["k"], c["v"]), 1).to(dev).view(-1)
        q, k, v = qkv, qkv[C:], qkv[2 * C:]
    else:
        q, k, v = (_padded(dev, c[n], ld) for n in ("q", "k", "v"))
    return q, k, v, _padded(dev, c["dctx"], ldc)


def _attn_forward(dev, q, k, v, B, H, ld, ldc, scale, p_drop, rng, call_id):
    rows, C, n = B * T_, H * HD, B * H * T_ * T_
    bc, ctx, behind = _rows(dev, rows, ldc)
    bp, P = _flat(dev, B, H, T_, T_)
    M = _bytes(dev, n)
    _call("kpf_attn21_forward", q, k, v, ctx, P, M, B, T_, H, HD, ld, ldc, scale, p_drop, rng, call_id)
    assert _kept(behind) and _kept(ctx[:rows, C:]), "ctx: wrote outside its columns or past the last row"
    assert _kept(bp[n:]) and bool((M[n:] == BYTE).all()), "P / M: wrote past the end"
    return ctx[:rows, :C], P, M


def _attn_backward(dev, dctx, q, k, v, P, M, B, H, ld, ldc, scale, p_drop):
    rows, C = B * T_, H * HD

    def bwd():
        if ld == 3 * C:
            b3, d3, behind = _rows(dev, rows, ld)
            flat = d3.view(-1)
            dq, dk, dv = flat, flat[C:], flat[2 * C:]
            outs = (d3[:rows, :C], d3[:rows, C:2 * C], d3[:rows, 2 * C:])
            guards = [behind]
        else:
            bufs = [_rows(dev, rows, ld) for _ in range(3)]
            dq, dk, dv = (b[1] for b in bufs)
            outs = tuple(b[1][:rows, :C] for b in bufs)
            guards = [b[2] for b in bufs] + [b[1][:rows, C:] for b in bufs]
        _call("kpf_attn21_backward", dctx, q, k, v, P, M, dq, dk, dv, B, T_, H, HD, ld, ldc, scale, p_drop)
        assert all(_kept(g) for g in guards), "dq / dk / dv: wrote outside their columns or past the last row"
        return outs

    return _twice(bwd)


@pytest.mark.parametrize("kind", ["soft", "sharp"])
@pytest.mark.parametrize("scale", TC.ATTN_SCALES)
@pytest.mark.parametrize("B,H,ld,ldc", TC.ATTN_SHAPES)
def test_attn21(B, H, ld, ldc, scale, kind):
    c = TC.attn_case(B, H, scale, kind)
    dev = _dev()
    q, k, v, dctx = _attn_operands(dev, c, B, H, ld, ldc)
    ctx, P, M = _attn_forward(dev, q, k, v, B, H, ld, ldc, scale, 0.0, None, 0)
    n = B * H * T_ * T_
    assert bool((M[:n] == 1).all()), "without dropout every probability is kept"
    tag = "attn21 B=%d H=%d ld=%d ldc=%d scale=%.3f %s " % (B, H, ld, ldc, scale, kind)
    ref, plain = c["ref"], c["plain"]
    _errs(tag + "P", P, ref["P"], plain["P"])
    _errs(tag + "ctx", ctx, ref["ctx"], plain["ctx"])
    dq, dk, dv = _attn_backward(dev, dctx, q, k, v, c["P_in"].to(dev), M, B, H, ld, ldc, scale, 0.0)
    for name, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        _errs(tag + name, g, ref[name], plain[name])


@pytest.mark.parametrize("kind", ["soft", "sharp"])
@pytest.mark.parametrize("B,H,ld,ldc", TC.ATTN_SHAPES)
def test_attn21_dropout(B, H, ld, ldc, kind):
    """p_drop = 0.25: the keep mask is read back and the float64 restatement replayed with it."""
    p, scale = 0.25, TC.ATTN_SCALES[0]
    c = TC.attn_case(B, H, scale, kind)
    dev = _dev()
    q, k, v, dctx = _attn_operands(dev, c, B, H, ld, ldc)
    n = B * H * T_ * T_
    rng = torch.tensor([20260, 7], dtype=torch.int64, device=dev)
    ctx, P, M = _attn_forward(dev, q, k, v, B, H, ld, ldc, scale, p, rng, 3)
    keep = M[:n].cpu()
    assert bool((keep <= 1).all())
    share = float(keep.double().mean())
    assert abs(share - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), "kept share %.4f of %d" % (share, n)
    assert torch.equal(_attn_forward(dev, q, k, v, B, H, ld, ldc, scale, p, rng, 3)[2], M), "the same (seed, counter, call) gives the same mask"
    assert not torch.equal(_attn_forward(dev, q, k, v, B, H, ld, ldc, scale, p, torch.tensor([20260, 8], dtype=torch.int64, device=dev), 3)[2], M), "another counter, another mask"
    assert not torch.equal(_attn_forward(dev, q, k, v, B, H, ld, ldc, scale, p, rng, 4)[2], M), "another call id, another mask"
    ref, plain = TC.attn_dropout_refs(B, H, scale, kind, keep.view(B, H, T_, T_), p)
    tag = "attn21 p_drop=0.25 B=%d H=%d ld=%d ldc=%d %s " % (B, H, ld, ldc, kind)
    print("ERR %-64s kept %.4f of %d" % (tag + "mask", share, n))
    _errs(tag + "P (before dropout)", P, ref["P"], plain["P"])
    _errs(tag + "ctx", ctx, ref["ctx"], plain["ctx"])
    dq, dk, dv = _attn_backward(dev, dctx, q, k, v, c["P_in"].to(dev), M, B, H, ld, ldc, scale, p)
    for name, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        _errs(tag + name, g, ref[name], plain[name])
