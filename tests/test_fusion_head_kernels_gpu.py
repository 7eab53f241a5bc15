"""The seven fp32 inference kernels of Block_KPFusion, each called through its C entry point on tensors built here and pinned to a float64
restatement of the same operation (oracle/kpf_oracle.py where it has the function, plain torch float64 otherwise): kpf_point_assemble_f32,
kpf_softmax_pool_f32, kpf_group_max_f32, kpf_heat_gam_gate_f32, kpf_gate_reduce_f32, kpf_tr_encoder_f32, kpf_xattn_layer_f32.

Tolerance.  No constant is invented: for every float comparison
    e_kernel = max|got - ref64| / max|ref64|        (the kernel)
    e_plain  = the same for the same restatement evaluated in plain fp32 torch on the CPU
and the assertion is  e_kernel <= 4 * e_plain + 8 * 2**-24  (4: MFMA chains and fixed-order LDS combines against torch's blocked sums; the floor:
cases where the plain evaluation happens to be exact).  Both numbers are printed per case (lines starting with "ERR"; the table of one run on the
MI355X is profiles/fusion_head_kernel_errors.txt).  Copies (pcl xyz, joint xyz, zero pads) and integer / mask decisions are compared for
equality.

Every case builder (`_*_case`) runs on the CPU alone and asserts, from the reference alone, that the case is in the regime it is named for (a
"sharp" case is sharp, a decision comparison leaves out at most the stated share of entries), before the kernel is looked at.

Outputs and the pad columns a kernel must not read are pre-filled with one NaN bit pattern: what a kernel writes must be finite, what it must not
write (guard rows behind the last row, columns outside [coff, coff + C)) must keep those bits."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import kpf_oracle as O

pytestmark = pytest.mark.gpu

J = 21
CANARY = 0x7FC0BEEF  # a quiet NaN with a payload
FLOOR = 8 * 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from keypointfusion_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _call(name, *args):
    from keypointfusion_amd import engine as E, lib as L
    L.check(getattr(L.load(), name)(*[E._ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], E._stream()), name)
    torch.cuda.synchronize()


def _canary(dev, *shape):
    return torch.full(shape, CANARY, dtype=torch.int32, device=dev).view(torch.float32)


def _kept(t):
    return bool((t.view(torch.int32) == CANARY).all())


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _errs(label, got, ref, plain):
    """Prints e_kernel and e_plain against the float64 reference and asserts the bound of the module docstring."""
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), label + ": not finite"
    den = float(ref.abs().max())
    assert den > 0 and ref.dtype == torch.float64 and plain.dtype == torch.float32 and got.dtype == torch.float32
    ek = float((got.double() - ref).abs().max()) / den
    ep = float((plain.double() - ref).abs().max()) / den
    print("ERR %-64s e_kernel %.3e  e_plain %.3e" % (label, ek, ep))
    assert ek <= 4 * ep + FLOOR, "%s: e_kernel %.3e > 4 * e_plain (%.3e) + 8 * 2^-24" % (label, ek, ep)
    return ek, ep


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_point_assemble_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
def _assemble_case(B, N, P, kernel, seed):
    g = torch.Generator().manual_seed(seed)
    k32 = float(torch.tensor(kernel, dtype=torch.float32))  # the radius as the entry point receives it
    feat_d = torch.randn(B, P, 128, generator=g)
    feat_rgb = torch.randn(B, P, 128, generator=g)
    offset = torch.randn(B, 5 * J, P, generator=g)
    joint = (torch.rand(B, J, 3, generator=g) - 0.5) * 1.2
    joint[:, 5] = torch.tensor([0.1, 0.1, 0.7])  # 0.29 below the z = 0.99 plane: the points planted there are inside both radii
    pcl = (torch.rand(B, N, 3, generator=g) * 2 - 1) * 0.9
    idx = torch.randint(0, P, (B, N, 4), generator=g, dtype=torch.int32)
    clos = torch.rand(B, N, 4, generator=g) + 0.05
    clos = clos / clos.sum(-1, keepdim=True)
    idx[:, 0] = torch.tensor([0, 0, P - 1, P - 1], dtype=torch.int32)  # first and last pixel, each twice within one point
    idx[:, 1] = 5 % P                                                 # four times the same pixel
    # planted points: (b, n, joint or None) -> what they are
    on_joint, z_masked, z_kept, inside, outside = [], [], [], [], []
    z99 = torch.tensor(0.99, dtype=torch.float32)
    for b in range(B):
        slots = iter(range(N - 1, -1, -1))  # from the back of the sample: the samples' last points sit in the straddling workgroup of (2, 502, .)

        def ring(j, f, ang):  # a point at distance kernel * f from joint j, in the joint's z plane (z stays below 0.99)
            n = next(slots)
            d = torch.tensor([math.cos(ang), math.sin(ang), 0.0], dtype=torch.float64) * (k32 * f)
            pcl[b, n] = (joint[b, j].double() + d).float()
            return b, n, j

        inside.append(ring(3, 1 - 3e-5, 0.3))
        outside.append(ring(3, 1 + 3e-5, 0.3))
        n = next(slots)
        pcl[b, n] = joint[b, 0]
        on_joint.append((b, n, 0))
        n = next(slots)
        pcl[b, n] = torch.tensor([0.1, 0.1, z99])
        z_masked.append((b, n))
        if N >= 16:
            inside += [ring(20, 1 - 1e-3, 2.0), ring(16, 1 - 3e-5, 4.0)]
            outside += [ring(20, 1 + 1e-3, 2.0), ring(16, 1 + 3e-5, 4.0)]
            n = next(slots)
            pcl[b, n] = joint[b, 20]
            on_joint.append((b, n, 20))
            for z, lst in ((torch.nextafter(z99, torch.tensor(2.0)), z_masked), (torch.tensor(1.0), z_masked), (torch.nextafter(z99, torch.tensor(0.0)), z_kept)):
                n = next(slots)
                pcl[b, n] = torch.tensor([0.1 + 0.01 * len(lst), 0.1, z])
                lst.append((b, n))
    d64 = lambda t: t.double()
    gi = lambda f, c: (O.gather_interp(d64(f), idx.long(), d64(clos)), O.gather_interp(f, idx.long(), clos))
    ref, plain = {}, {}
    ref["pf"], plain["pf"] = gi(feat_d.permute(0, 2, 1), clos)
    ref["pf_rgb"], plain["pf_rgb"] = gi(feat_rgb.permute(0, 2, 1), clos)
    ref["pw"], plain["pw"] = gi(offset[:, 4 * J:], clos)
    ref["off"], plain["off"] = O.pcl_joint2offset(d64(joint), d64(pcl), k32), O.pcl_joint2offset(joint, pcl, kernel)
    # conditions, from the reference alone
    dis = torch.sqrt(((d64(joint).unsqueeze(2) - d64(pcl).unsqueeze(1)) ** 2).sum(-1))  # B J N
    clos_unmasked = ((k32 - dis) / k32).permute(0, 2, 1)  # B N J
    compared = clos_unmasked.abs() > 1e-6  # the 0/1 mask is a decision: entries closer to the radius than this are left out
    left_out = 1.0 - float(compared.double().mean())
    assert left_out <= 1e-3, left_out
    mask_of = lambda o: (o[..., :63].reshape(B, N, J, 3) != 0).any(-1) | (o[..., 63:] != 0)  # B N J
    m64, m32 = mask_of(ref["off"]), mask_of(plain["off"])
    assert bool((m64 == m32)[compared].all())  # away from the radius the decision does not depend on the precision
    for b, n, j in inside + outside + on_joint:
        assert bool(compared[b, n, j]), (b, n, j)
    for b, n in z_masked + z_kept:
        assert bool(compared[b, n].all())
    assert all(bool(m32[b, n, j]) for b, n, j in inside) and not any(bool(m32[b, n, j]) for b, n, j in outside)
    assert all(abs(float(clos_unmasked[b, n, j])) < 2e-3 for b, n, j in inside + outside)  # both sides of the radius, close to it
    for b, n, j in on_joint:
        assert float(dis[b, j, n]) == 0.0 and float(ref["off"][b, n, 63 + j]) == 1.0 and not bool(ref["off"][b, n, 3 * j:3 * j + 3].any())
    assert not any(bool(m32[b, n].any()) for b, n in z_masked) and all(bool(m32[b, n, 5]) for b, n in z_kept)
    assert all(bool((clos_unmasked[b, n, 5] > 0.3)) for b, n in z_masked)  # only their z masks them
    return dict(feat_d=feat_d, feat_rgb=feat_rgb, offset=offset, joint=joint, pcl=pcl, idx=idx, clos=clos, ref=ref, plain=plain,
                compared=compared, mask32=m32, mask_of=mask_of, left_out=left_out)


@pytest.mark.parametrize("kernel", [0.8, 0.6])
@pytest.mark.parametrize("B,N,P", [(2, 1024, 1024), (1, 4, 16), (2, 502, 4096)])
def test_point_assemble(B, N, P, kernel):
    c = _assemble_case(B, N, P, kernel, 11 * N + P)
    dev = _dev()
    A1, A2 = _canary(dev, B * N + 1, 240), _canary(dev, B * N + 1, 128)
    d = {k: c[k].to(dev) for k in ("feat_d", "feat_rgb", "offset", "pcl", "joint", "clos", "idx")}
    _call("kpf_point_assemble_f32", d["feat_d"], d["feat_rgb"], d["offset"], d["pcl"], d["joint"], d["clos"], d["idx"], A1, A2, B, N, P, kernel)
    assert _kept(A1[B * N]) and _kept(A2[B * N]), "wrote past the last point"
    a1, a2 = A1[:B * N].cpu().view(B, N, 240), A2[:B * N].cpu().view(B, N, 128)
    assert bool(torch.isfinite(a1).all()) and bool(torch.isfinite(a2).all())
    tag = "point_assemble B=%d N=%d P=%d r=%.1f " % (B, N, P, kernel)
    _errs(tag + "pf", a1[..., :128], c["ref"]["pf"], c["plain"]["pf"])
    _errs(tag + "pf_rgb", a2, c["ref"]["pf_rgb"], c["plain"]["pf_rgb"])
    assert _bits(a1[..., 128:131], c["pcl"]), "pcl xyz is a copy"
    _errs(tag + "pw", a1[..., 131:152], c["ref"]["pw"], c["plain"]["pw"])
    assert bool((a1[..., 236:] == 0).all())
    off = a1[..., 152:236]
    cmp_ = c["compared"]
    assert torch.equal(c["mask_of"](off)[cmp_], c["mask32"][cmp_]), "mask decisions (left out: %.4f %% of the entries)" % (100 * c["left_out"])
    keep = torch.cat((cmp_.unsqueeze(-1).expand(B, N, J, 3).reshape(B, N, 63), cmp_), -1)
    z = lambda t: torch.where(keep, t, torch.zeros_like(t))
    _errs(tag + "offsets+closeness", z(off), z(c["ref"]["off"]), z(c["plain"]["off"]))


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_softmax_pool_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
def _pool_case(B, N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, N, 128, generator=g)
    joint = torch.randn(B, J, 3, generator=g)
    if kind == "normal":
        pw = torch.randn(B, N, J, generator=g)
    elif kind == "wide":
        pw = torch.randn(B, N, J, generator=g) * 30
        pw[0, N // 2, 0] = 200.0
        pw[B - 1, N - 1, 3] = -200.0
        assert bool(torch.isinf(torch.exp(pw)).any())  # a kernel without the max subtraction overflows here
    elif kind == "equal":
        pw = torch.full((B, N, J), 3.25)
    else:
        pw = torch.randn(B, N, J, generator=g)
        at = torch.randint(0, N, (B, J), generator=g)
        pw.scatter_add_(1, at.unsqueeze(1), torch.full((B, 1, J), 50.0))
    att = torch.softmax(pw.double().permute(0, 2, 1), -1)
    if kind == "equal":
        assert float(att.max()) == float(att.min()) == 1.0 / N
    if kind == "dominant":
        assert float(att.amax(-1).min()) > 0.999
    ref = att @ X.double()
    plain = torch.softmax(pw.permute(0, 2, 1), -1) @ X
    return X, joint, pw, ref, plain


@pytest.mark.parametrize("kind", ["normal", "wide", "equal", "dominant"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [4, 120, 124, 128, 1024, 2048])  # 120 / 124 / 128: around the 16-rows-in-flight loop; 2048: more than 64 KiB of LDS
def test_softmax_pool(N, B, kind):
    X, joint, pw, ref, plain = _pool_case(B, N, kind, 7 * N + B)
    dev = _dev()
    A1 = _canary(dev, B * N, 240)  # only the weight-logit columns are set
    A1[:, 131:152] = pw.view(B * N, J).to(dev)
    JA = _canary(dev, B * J + 1, 132)
    _call("kpf_softmax_pool_f32", A1, X.to(dev), joint.to(dev), JA, B, N)
    assert _kept(JA[B * J]), "wrote past the last joint"
    ja = JA[:B * J].cpu().view(B, J, 132)
    _errs("softmax_pool N=%d B=%d %s" % (N, B, kind), ja[..., :128], ref, plain)
    assert _bits(ja[..., 128:131], joint) and bool((ja[..., 131] == 0).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_group_max_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,group,C,out_ld,out_coff", [(42, 64, 128, 512, 128),   # as the engine calls it
                                                          (7, 5, 132, 132, 0),       # 33 channel quads: seven member subgroups, 25 idle threads
                                                          (5, 1, 1024, 1024, 0),
                                                          (42, 64, 6, 8, 1),         # scalar kernel (C % 4)
                                                          (3, 3, 128, 130, 2)])      # scalar kernel (row stride and offset not 16-byte aligned)
def test_group_max(rows, group, C, out_ld, out_coff):
    g = torch.Generator().manual_seed(rows * C + group)
    x = torch.randn(rows, group, C, generator=g)
    x[0] = -x[0].abs() - 0.5        # an all-negative group
    x[rows - 1] = -float("inf")     # a group of -inf
    x[1, :, 0] = -float("inf")      # a -inf channel
    x[1, group // 2, 1:3] = float("inf")
    ref = torch.amax(x, 1)
    assert bool((ref[0] < 0).all()) and bool(torch.isinf(ref[rows - 1]).all())
    dev = _dev()
    out = _canary(dev, rows + 1, out_ld)
    _call("kpf_group_max_f32", x.to(dev), out, rows, group, C, out_ld, out_coff)
    assert _kept(out[rows]) and _kept(out[:rows, :out_coff]) and _kept(out[:rows, out_coff + C:]), "wrote outside the slice"
    assert _bits(out[:rows, out_coff:out_coff + C].cpu(), ref)
    print("ERR %-64s bit-equal to torch.amax" % ("group_max rows=%d group=%d C=%d ld=%d coff=%d" % (rows, group, C, out_ld, out_coff)))


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_heat_gam_gate_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
def _gate_case(B, Fs, wdis, seed):
    import numpy as np
    from keypointfusion_amd.weights import synthetic_batch
    P = Fs * Fs
    img_size = 256 if Fs == 64 else 128
    g = torch.Generator().manual_seed(seed)
    geo = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synthetic_batch(B, img_size, seed=seed).items() if k in ("center", "M", "cube", "cam_para")}
    r3d = torch.cat(((torch.rand(B, J, 2, generator=g) * 2 - 1) * 0.9, torch.rand(B, J, 1, generator=g) - 0.5), -1)
    r3d[:, 0, :2] = torch.tensor([1.0, -1.0])   # on the crop's border
    r3d[:, 1, :2] = torch.tensor([-1.0, 1.0])
    r3d[:, 2, 0] = 3.0                          # outside the crop
    r3d[:, 3, 1] = -3.0
    img_xyz = torch.rand(B, P, 3, generator=g) * 2 - 1
    sf = torch.randn(B, P, J, generator=g) * 2
    plus = [(0, 5), (P - 1, 6), (P // 2, 2)]    # (pixel, joint) whose logit is +100 / -100
    minus = [(0, 7), (P - 1, 20), (P // 3, 3)]
    for p, j in plus:
        sf[:, p, j] = 100.0
    for p, j in minus:
        sf[:, p, j] = -100.0
    Wh = torch.randn(J, J, generator=g) * 0.3
    bias = torch.randn(J, generator=g)
    wfc = torch.randn(P, generator=g)
    wd_ = torch.tensor([wdis], dtype=torch.float32)
    assert bool((wfc > 0).any()) and bool((wfc < 0).any())

    def restate(t):  # t: cast to the precision of the restatement
        r, c, M, cube, cam = t(r3d), t(geo["center"]), t(geo["M"]), t(geo["cube"]), t(geo["cam_para"])
        hm = O.joint2heatmap(r[:, :, :2], 0.8, Fs, sigma=1).reshape(B, J, P)
        s = t(sf).permute(0, 2, 1) + torch.einsum("jk,bkp->bjp", t(Wh), hm) + t(bias).view(1, J, 1)
        sw = torch.sigmoid(s)
        jx = O.uvd2xyz(r, c, M, cube, cam, img_size, 1)
        dist = ((t(img_xyz).unsqueeze(1) - jx.unsqueeze(2)) ** 2).sum(-1)
        gam = 1 / (10 * dist + 1)
        wd = torch.sigmoid(t(wd_))
        return sw, (wd * gam + (1 - wd) * sw) * t(wfc).view(1, 1, P), s, hm

    sw64, gw64, s64, hm64 = restate(lambda v: v.double())
    sw32, gw32, _, _ = restate(lambda v: v.float())
    # conditions: the planted logits saturate the fp32 sigmoid, the joints outside the crop have no heat-map
    assert all(float(s64[:, j, p].min()) > 90 for p, j in plus) and all(float(s64[:, j, p].max()) < -90 for p, j in minus)
    assert float(hm64[:, 2:4].max()) < 1e-20 and (Fs < 20 or float(hm64[:, 2:4].max()) < 2.0 ** -150)
    assert float(hm64[:, :2].max()) > 0.5  # the border joints still light the corner pixels
    return dict(geo=geo, r3d=r3d, img_xyz=img_xyz, sf=sf, Wh=Wh, bias=bias, wfc=wfc, wd=wd_, img_size=img_size, plus=plus, minus=minus,
                sw64=sw64, gw64=gw64, sw32=sw32, gw32=gw32)


@pytest.mark.parametrize("wdis", [-20.0, 0.3, 20.0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Fs", [8, 20, 32, 64])  # P below one workgroup / not a multiple of 256 / the model's two sizes
def test_heat_gam_gate(Fs, B, wdis):
    from keypointfusion_amd import engine as E
    c = _gate_case(B, Fs, wdis, 100 * Fs + B)
    P = Fs * Fs
    dev = _dev()
    SF = _canary(dev, B * P, 24)  # columns 21..23 are padding
    SF[:, :J] = c["sf"].view(B * P, J).to(dev)
    sw, Gw = _canary(dev, B * J * P + 64), _canary(dev, B * J * P + 64)
    geo = {k: v.to(dev) for k, v in c["geo"].items()}
    Minv = E.crop_inverse(geo["M"])
    _call("kpf_heat_gam_gate_f32", c["r3d"].to(dev), c["img_xyz"].to(dev), SF, 24, c["Wh"].to(dev), c["bias"].to(dev), c["wd"].to(dev), c["wfc"].to(dev),
          geo["center"], Minv, geo["cube"], geo["cam_para"], sw, Gw, B, Fs, c["img_size"], 1)
    assert _kept(sw[B * J * P:]) and _kept(Gw[B * J * P:]), "wrote past the last pixel"
    sw, Gw = sw[:B * J * P].cpu().view(B, J, P), Gw[:B * J * P].cpu().view(B, J, P)
    tag = "heat_gam_gate F=%d B=%d weight_dis=%g " % (Fs, B, wdis)
    _errs(tag + "sw", sw, c["sw64"], c["sw32"])
    _errs(tag + "Gw", Gw, c["gw64"], c["gw32"])
    assert all(bool((sw[:, j, p] == 1.0).all()) for p, j in c["plus"]) and all(bool((sw[:, j, p] == 0.0).all()) for p, j in c["minus"]), "saturated sigmoid"


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_gate_reduce_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prev", [False, True], ids=["prev_null", "prev_given"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [32, 64, 1024, 4096])
def test_gate_reduce(P, B, with_prev):
    g = torch.Generator().manual_seed(3 * P + B)
    Gw = torch.randn(B, J, P, generator=g)      # both signs: the contract is Gw @ relu(feat) + b, the relu on the features
    feat = torch.randn(B, P, 128, generator=g)
    bfc = torch.randn(1, generator=g)
    prev = torch.randn(B, J, 128, generator=g) if with_prev else None

    def restate(t):
        v = torch.einsum("bjp,bpc->bjc", t(Gw), F.relu(t(feat))) + t(bfc)
        return F.relu((v + t(prev)) / 2) if with_prev else v

    ref, plain = restate(lambda v: v.double()), restate(lambda v: v.float())
    assert bool((Gw < 0).any()) and bool((feat < 0).any()) and (with_prev or bool((ref < 0).any()))
    dev = _dev()
    out = _canary(dev, B * J * 128 + 128)
    d = [Gw.to(dev), feat.to(dev), bfc.to(dev), prev.to(dev) if with_prev else None]
    _call("kpf_gate_reduce_f32", *d, out, B, P)
    assert _kept(out[B * J * 128:]), "wrote past joint 20 of the last sample"
    got = out[:B * J * 128].view(B, J, 128)
    _errs("gate_reduce P=%d B=%d prev=%d" % (P, B, with_prev), got, ref, plain)
    if B > 1:  # a sample's bits do not depend on its neighbours: the last sample alone, and the first with a NaN gate next to it
        alone = _canary(dev, J * 128)
        _call("kpf_gate_reduce_f32", d[0][B - 1], d[1][B - 1], d[2], d[3][B - 1] if with_prev else None, alone, 1, P)
        assert _bits(alone.view(J, 128), got[B - 1])
        d[0][1, 20] = float("nan")
        out2 = _canary(dev, B * J * 128)
        _call("kpf_gate_reduce_f32", *d, out2, B, P)
        out2 = out2.view(B, J, 128)
        assert _bits(out2[0], got[0]) and _bits(out2[2], got[2]) and _bits(out2[1, :20], got[1, :20]), "a NaN in joint 20's gate reached another row"


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_tr_encoder_f32 and kpf_xattn_layer_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
NMAX = 64  # samples drawn per case; a test with B < NMAX takes the first B


def _rand64(g):
    return lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * sc


def _sharpness(q, k):
    """q, k [B][T][128] (the logit scale folded into q) -> (largest |logit| per sample, share of peaked attention rows per sample)."""
    B = q.shape[0]
    lg = q.view(B, J, 4, 32).transpose(1, 2) @ k.view(B, J, 4, 32).transpose(1, 2).transpose(-1, -2)
    return lg.abs().amax((1, 2, 3)), (torch.softmax(lg, -1).amax(-1) > 0.9).double().mean((1, 2))


@functools.lru_cache(maxsize=None)
def _tr_weights(din, kind):
    """Random float64 weights at 1/sqrt(fan_in), LayerNorm weights in [0.5, 1.5], intermediate.dense x 3 (GELU arguments reach |x| ~ 10), query and key
    x 4 in the sharp set; rounded to fp32, which is what the kernel is given.  Inputs: NMAX samples of N(0, 1), ordered by their largest layer-0 logit."""
    g = torch.Generator().manual_seed(1000 * din + 10 + (kind == "sharp"))
    r = _rand64(g)
    qk = 4.0 if kind == "sharp" else 1.0
    sd = {"p.bert.img_embedding.weight": r(128, din, sc=din ** -0.5), "p.bert.img_embedding.bias": r(128, sc=0.1),
          "p.bert.position_embeddings.weight": r(32, 128, sc=0.5)}
    for l in range(4):
        q = "p.bert.encoder.layer.%d." % l
        for n in ("query", "key", "value"):
            sd[q + "attention.self.%s.weight" % n] = r(128, 128, sc=(qk if n != "value" else 1.0) * 128 ** -0.5)
            sd[q + "attention.self.%s.bias" % n] = r(128, sc=0.1)
        sd[q + "attention.output.dense.weight"] = r(128, 128, sc=128 ** -0.5)
        sd[q + "attention.output.dense.bias"] = r(128, sc=0.1)
        sd[q + "attention.output.LayerNorm.weight"] = 0.5 + torch.rand(128, generator=g, dtype=torch.float64)
        sd[q + "attention.output.LayerNorm.bias"] = r(128, sc=0.1)
        sd[q + "intermediate.dense.weight"] = r(16, 128, sc=3 * 128 ** -0.5)
        sd[q + "intermediate.dense.bias"] = r(16, sc=0.5)
        sd[q + "output.dense.weight"] = r(128, 16, sc=0.25)
        sd[q + "output.dense.bias"] = r(128, sc=0.1)
        sd[q + "output.LayerNorm.weight"] = 0.5 + torch.rand(128, generator=g, dtype=torch.float64)
        sd[q + "output.LayerNorm.bias"] = r(128, sc=0.1)
    sd["p.cls_head.weight"] = r(3, 128, sc=128 ** -0.5)
    sd["p.cls_head.bias"] = r(3, sc=0.1)
    sd["p.residual.weight"] = r(3, din, sc=din ** -0.5)
    sd["p.residual.bias"] = r(3, sc=0.1)
    sd32 = {k: v.float() for k, v in sd.items()}
    sd64 = {k: v.double() for k, v in sd32.items()}
    x = torch.randn(NMAX, J, din, generator=g)
    q0 = "p.bert.encoder.layer.0.attention.self."
    h0 = F.linear(x.double(), sd64["p.bert.img_embedding.weight"], sd64["p.bert.img_embedding.bias"]) + sd64["p.bert.position_embeddings.weight"][:J]
    lmax, peaked = _sharpness(F.linear(h0, sd64[q0 + "query.weight"], sd64[q0 + "query.bias"]) / math.sqrt(32), F.linear(h0, sd64[q0 + "key.weight"], sd64[q0 + "key.bias"]))
    order = torch.argsort(lmax, descending=True)
    return sd32, sd64, x[order].contiguous(), lmax[order], peaked[order]


@functools.lru_cache(maxsize=None)
def _tr_case(din, kind, B):
    sd32, sd64, x, lmax, peaked = _tr_weights(din, kind)
    x = x[:B]
    h64, s64 = O.kp_interaction_tr(sd64, "p", x.double())
    h32, s32 = O.kp_interaction_tr(sd32, "p", x)
    ep = max(float((h32.double() - h64).abs().max() / h64.abs().max()), float((s32.double() - s64).abs().max() / s64.abs().max()))
    if kind == "sharp":  # from the float64 reference: a layer-0 logit beyond exp's fp32 range, most attention rows peaked
        assert float(lmax[:B].max()) > 88, float(lmax[:B].max())
        assert float(peaked[:B].mean()) > 0.5, float(peaked[:B].mean())
        assert ep < 3e-4, ep  # the function itself stays well conditioned: the comparison means something
    return sd32, x, h64, s64, h32, s32


TR_DINS = [(128, 128), (131, 132), (3, 4), (20, 20), (208, 208)]  # (Din, ldx); 208 is the deepest embedding whose tokens fit the LDS


def _run_tr(dev, W, x, din, ldx, B, with_score2):
    X = _canary(dev, B * J, ldx)  # pad columns [Din, ldx) are NaN
    X[:, :din] = x.reshape(B * J, din).to(dev)
    h, score = _canary(dev, B * J + 1, 128), _canary(dev, B * J + 1, 3)
    score2 = _canary(dev, B * J + 1, 132) if with_score2 else None
    _call("kpf_tr_encoder_f32", X, ldx, din, W, h, score, score2, 132 if with_score2 else 0, B)
    assert _kept(h[B * J]) and _kept(score[B * J]), "wrote past the last token"
    if with_score2:
        assert _kept(score2[B * J]) and _kept(score2[:, 3:]), "score2: wrote outside columns 0..2"
        assert _bits(score2[:B * J, :3], score[:B * J])
    return h[:B * J].view(B, J, 128), score[:B * J].view(B, J, 3)


@pytest.mark.parametrize("with_score2", [False, True], ids=["score2_null", "score2_ld132"])
@pytest.mark.parametrize("kind", ["mild", "sharp"])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("din,ldx", TR_DINS)
def test_tr_encoder(din, ldx, B, kind, with_score2):
    from keypointfusion_amd import engine as E
    sd32, x, h64, s64, h32, s32 = _tr_case(din, kind, B)
    dev = _dev()
    h, score = _run_tr(dev, E.pack_tr(sd32, "p", din, dev), x, din, ldx, B, with_score2)
    tag = "tr_encoder Din=%d B=%d %s score2=%d " % (din, B, kind, with_score2)
    _errs(tag + "h", h, h64, h32)
    _errs(tag + "score", score, s64, s32)


@pytest.mark.parametrize("kind", ["mild", "sharp"])
@pytest.mark.parametrize("din,ldx", TR_DINS)
def test_tr_encoder_samples_are_independent(din, ldx, kind):
    """A sample's bits are the same alone and inside a batch of 64, and a NaN in sample 3's input stays in sample 3."""
    from keypointfusion_amd import engine as E
    sd32, x = _tr_weights(din, kind)[0], _tr_weights(din, kind)[2]
    dev = _dev()
    W = E.pack_tr(sd32, "p", din, dev)
    h, score = _run_tr(dev, W, x, din, ldx, NMAX, True)
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(score).all())
    for i in (0, 3, NMAX - 1):
        h1, s1 = _run_tr(dev, W, x[i:i + 1], din, ldx, 1, False)
        assert _bits(h1[0], h[i]) and _bits(s1[0], score[i]), i
    xn = x.clone()
    xn[3, 7, 0] = float("nan")
    hn, sn = _run_tr(dev, W, xn, din, ldx, NMAX, False)
    others = [i for i in range(NMAX) if i != 3]
    assert _bits(hn[others], h[others]) and _bits(sn[others], score[others])
    assert not bool(torch.isfinite(hn[3]).all())


@functools.lru_cache(maxsize=None)
def _xattn_weights(kind):
    g = torch.Generator().manual_seed(77 + (kind == "sharp"))
    r = _rand64(g)
    W = r(384, 128, sc=128 ** -0.5)
    if kind == "sharp":
        W[:256] *= 4.0  # the q and k rows
    sd = {"p.self_posembed.weight": r(32, 128, sc=0.5), "p.cross_posembed.weight": r(32, 128, sc=0.5),
          "p.multihead_attn.in_proj_weight": W, "p.multihead_attn.in_proj_bias": r(384, sc=0.1),
          "p.multihead_attn.out_proj.weight": r(128, 128, sc=128 ** -0.5), "p.multihead_attn.out_proj.bias": r(128, sc=0.1),
          "p.norm2.weight": 0.5 + torch.rand(128, generator=g, dtype=torch.float64), "p.norm2.bias": r(128, sc=0.1),
          "p.linear1.weight": r(128, 128, sc=128 ** -0.5), "p.linear1.bias": r(128, sc=0.5),
          "p.linear2.weight": r(128, 128, sc=128 ** -0.5), "p.linear2.bias": r(128, sc=0.1),
          "p.norm3.weight": 0.5 + torch.rand(128, generator=g, dtype=torch.float64), "p.norm3.bias": r(128, sc=0.1)}
    sd32 = {k: v.float() for k, v in sd.items()}
    sd64 = {k: v.double() for k, v in sd32.items()}
    query, key = torch.randn(NMAX, J, 128, generator=g), torch.randn(NMAX, J, 128, generator=g)
    Wi, bi = sd64["p.multihead_attn.in_proj_weight"], sd64["p.multihead_attn.in_proj_bias"]
    lmax, peaked = _sharpness(F.linear(query.double() + sd64["p.self_posembed.weight"][:J], Wi[:128], bi[:128]) / math.sqrt(32),
                              F.linear(key.double() + sd64["p.cross_posembed.weight"][:J], Wi[128:256], bi[128:256]))
    order = torch.argsort(lmax, descending=True)
    return sd32, sd64, query[order].contiguous(), key[order].contiguous(), lmax[order], peaked[order]


@functools.lru_cache(maxsize=None)
def _xattn_case(kind, B):
    sd32, sd64, query, key, lmax, peaked = _xattn_weights(kind)
    query, key = query[:B], key[:B]
    ref = O.decoder_layer(sd64, "p", query.double(), key.double())
    plain = O.decoder_layer(sd32, "p", query, key)
    if kind == "sharp":
        assert float(lmax[:B].max()) > 88, float(lmax[:B].max())
        assert float(peaked[:B].mean()) > 0.5, float(peaked[:B].mean())
        assert float((plain.double() - ref).abs().max() / ref.abs().max()) < 3e-4
    return sd32, query, key, ref, plain


def _run_xattn(dev, W, query, key, B, out_ld, out_coff):
    out = _canary(dev, B * J + 1, out_ld)
    _call("kpf_xattn_layer_f32", query.to(dev), key.to(dev), W, out, out_ld, out_coff, B)
    assert _kept(out[B * J]) and _kept(out[:, :out_coff]) and _kept(out[:, out_coff + 128:]), "wrote outside the slice"
    return out[:B * J, out_coff:out_coff + 128].reshape(B, J, 128)


@pytest.mark.parametrize("kind", ["mild", "sharp"])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("out_ld,out_coff", [(132, 3), (128, 0)])  # as the engine calls it; dense
def test_xattn_layer(out_ld, out_coff, B, kind):
    from keypointfusion_amd import engine as E
    sd32, query, key, ref, plain = _xattn_case(kind, B)
    dev = _dev()
    got = _run_xattn(dev, E.pack_xattn(sd32, "p", dev), query, key, B, out_ld, out_coff)
    _errs("xattn_layer ld=%d coff=%d B=%d %s" % (out_ld, out_coff, B, kind), got, ref, plain)


@pytest.mark.parametrize("kind", ["mild", "sharp"])
def test_xattn_layer_samples_are_independent(kind):
    from keypointfusion_amd import engine as E
    sd32, _, query, key = _xattn_weights(kind)[:4]
    dev = _dev()
    W = E.pack_xattn(sd32, "p", dev)
    full = _run_xattn(dev, W, query, key, NMAX, 132, 3)
    assert bool(torch.isfinite(full).all())
    for i in (0, 3, NMAX - 1):
        assert _bits(_run_xattn(dev, W, query[i:i + 1], key[i:i + 1], 1, 132, 3)[0], full[i]), i
    others = [i for i in range(NMAX) if i != 3]
    for which in (0, 1):  # a NaN in sample 3's query, then in its key
        qn, kn = query.clone(), key.clone()
        (qn, kn)[which][3, 7, 0] = float("nan")
        out = _run_xattn(dev, W, qn, kn, NMAX, 132, 3)
        assert _bits(out[others], full[others]), which
        assert not bool(torch.isfinite(out[3]).all())
