"""Seeded cases for the training-side fusion-head kernels (csrc/kpf_train.hip, and kpf_ball_group_stacked_f32 of csrc/kpf_geom.hip): inputs as fp32 CPU
tensors, the float64 restatement of each operation (oracle/kpf_oracle.py and oracle/train_oracle.py where they have the function, plain torch with autograd
otherwise) and the same restatement evaluated in plain fp32 on the CPU.  No GPU is touched here.

Every builder is cached (functools.lru_cache): tests/test_train_head_cases_host.py asserts the regime of each case from the reference alone, and
tests/test_train_head_kernels_gpu.py holds the kernels to  e_kernel <= 4 * e_plain + 8 * 2^-24  on the same objects, which no test modifies.

A case is a dict:  inputs by name,  "ref" (float64) and "plain" (fp32) results by output name,  and what was planted where."""
import functools
import math

import torch

from oracle import kpf_oracle as O
from oracle import train_oracle as T

FLOOR = 8 * 2.0 ** -24
SLICE_FLOOR = 2.0 ** -20  # a planted slice's denominator is at least this share of its tensor's: fp32 underflow is not judged


def rel_err(x, ref, sel=None):
    """max|x - ref| / max|ref| over the tensor; with `sel` over that slice, its denominator floored at 2^-20 of the whole tensor's."""
    assert ref.dtype == torch.float64
    den = float(ref.abs().max())
    if sel is not None:
        x, ref = x[sel], ref[sel]
        den = max(float(ref.abs().max()), SLICE_FLOOR * den)
    return float((x.double() - ref).abs().max()) / den


def bound(case, name, sel=None):
    """The right-hand side of the rule for output `name` of a case."""
    return 4 * rel_err(case["plain"][name], case["ref"][name], sel) + FLOOR


def _gen(*key):
    """A generator seeded by the case's integer parameters."""
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _leaf(t, v):
    """A fresh leaf of the restatement's precision (the case's own tensors never take part in autograd)."""
    return t(v).detach().clone().requires_grad_(True)


def _both(fn):
    """fn(t) with t the cast of the restatement's precision -> (float64 results, fp32 results)."""
    return fn(lambda v: v.double()), fn(lambda v: v.float())


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. kpf_joint_heatmap_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
HEATMAP_SHAPES = [(2, 21, 32), (1, 3, 5), (2, 5, 17)]  # (B, J, F): the workload's; P = 25 < 256 threads; P = 289 = 256 + 33
HEATMAP_STD_SIGMA = [(0.8, 1.0), (1.0, 1.5)]


@functools.lru_cache(maxsize=None)
def heatmap_case(B, J, Fs, std, sigma):
    """Planted joints per sample: 0 on a pixel centre, 1 at u = +-1 (the map's border), 2 at +-1.5 (off the map), 3 at +-4 (far off: with F >= 17 every fp32 value of
    its map underflows to 0).  J = 3 has no fourth joint: its joint 2 is at (u, v) = (+-1.5, -+4)."""
    g = _gen(B, J, Fs, int(10 * std), int(10 * sigma))
    uvd = (torch.rand(B, J, 3, generator=g) * 2 - 1) * 1.2
    for b in range(B):
        s = 1.0 if b % 2 == 0 else -1.0
        px, py = (Fs // 2 + b) % Fs, (Fs // 3) % Fs
        uvd[b, 0, 0], uvd[b, 0, 1] = (px + 0.5) / Fs * 2 - 1, (py + 0.5) / Fs * 2 - 1
        uvd[b, 1, 0], uvd[b, 1, 1] = s, -s
        uvd[b, 2, 0], uvd[b, 2, 1] = 1.5 * s, (-1.5 * s if J > 3 else -4.0 * s)
        if J > 3:
            uvd[b, 3, 0], uvd[b, 3, 1] = -4.0 * s, 4.0 * s
    dhm = torch.randn(B, J, Fs, Fs, generator=g)

    def run(t, j2h):
        u = _leaf(t, uvd)
        hm = j2h(u[:, :, :2], std, Fs, sigma=sigma)
        (hm * t(dhm)).sum().backward()
        return {"hm": hm.detach(), "duvd": u.grad.detach()}

    ref = run(lambda v: v.double(), O.joint2heatmap)     # (train_oracle's statement rounds the joint to fp32: its float64 form is kpf_oracle's)
    plain = run(lambda v: v.float(), T.joint2heatmap)
    return dict(uvd=uvd, dhm=dhm, ref=ref, plain=plain, centre=0, border=1, off=2, far=3 if J > 3 else 2, underflows=Fs >= 17)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. kpf_geom_gate_forward / _backward and kpf_geom_gate_uvd_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
GATE_SHAPES = [(2, 21, 300), (1, 1, 1), (2, 4, 255), (2, 4, 257)]  # (B, J, P): more than one trip with a tail; one thread; one short of / one beyond 256


def _gate(pix, jx):
    return 1 / (10 * ((pix.unsqueeze(1) - jx.unsqueeze(2)) ** 2).sum(-1) + 1)  # [B][J][P]


@functools.lru_cache(maxsize=None)
def geom_gate_case(B, J, P):
    """Planted (P >= 3): pixel 0 of every sample lies on joint 0 (gam == 1, no gradient from it); pixel P - 1 at distance 30 from joint J - 1 (gam ~ 1e-4)."""
    g = _gen(B, J, P, 2)
    pix = torch.rand(B, P, 3, generator=g) * 2 - 1
    joint = (torch.rand(B, J, 3, generator=g) * 2 - 1) * 0.6
    planted = P >= 3
    if planted:
        pix[:, 0] = joint[:, 0]
        pix[:, P - 1] = joint[:, J - 1] + 30.0 * torch.tensor([2.0, -1.0, 2.0]) / 3.0
    dgam = torch.randn(B, J, P, generator=g)

    def run(t):
        jx = _leaf(t, joint)
        gam = _gate(t(pix), jx)
        (gam * t(dgam)).sum().backward()
        return {"gam": gam.detach(), "djoint": jx.grad.detach()}

    ref, plain = _both(run)
    return dict(pix=pix, joint=joint, dgam=dgam, ref=ref, plain=plain, planted=planted)


def _uvd_restate(c, t, flip, swap=None):
    """The gate of joints given as crop coordinates: uvd2xyz (dataloader/loader.py:775-789), then the gate expression, gradient towards uvd.
    swap = "f": fx and fy exchanged, "cube": cube_x and cube_y exchanged (what a kernel that confused par16's positions would compute)."""
    cam, cube = t(c["cam"]).clone(), t(c["cube"]).clone()
    if swap == "f":
        cam[:, [0, 1]] = cam[:, [1, 0]]
    if swap == "cube":
        cube[:, [0, 1]] = cube[:, [1, 0]]
    u = _leaf(t, c["uvd"])
    jx = O.uvd2xyz(u, t(c["center"]), t(c["M"]), cube, cam, c["img_size"], flip)
    gam = _gate(t(c["pix"]), jx)
    (gam * t(c["dgam"])).sum().backward()
    return {"gam": gam.detach(), "duvd": u.grad.detach(), "xyz": jx.detach()}


@functools.lru_cache(maxsize=None)
def geom_gate_uvd_case(B, J, P, flip, half_size):
    """Per-sample camera and crop: fx != fy, u0 != v0, a cube of (250, 200, 300) mm, a centre off the optical axis, M^-1 with rotation, shear and a translation
    of more than 50 px.  The kernel is given M^-1 rounded to fp32 (par16); the reference inverts M = (that M^-1)^-1 as uvd2xyz does.  Planted as in
    geom_gate_case, the coinciding pixel at the float64 position of joint 0 rounded to fp32."""
    g = _gen(B, J, P, 3, flip + 1, int(half_size))
    img_size = int(2 * half_size)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    cam = torch.tensor([615.0, 580.0, 322.5, 243.75], dtype=torch.float64).repeat(B, 1) + (r(B, 4) - 0.5) * 8
    cube = torch.tensor([250.0, 200.0, 300.0], dtype=torch.float64).repeat(B, 1)
    center = torch.tensor([35.0, -25.0, 620.0], dtype=torch.float64).repeat(B, 1) + (r(B, 3) - 0.5) * 20
    Minv = torch.zeros(B, 3, 3, dtype=torch.float64)
    for b in range(B):
        th = 0.25 * (1 if b % 2 == 0 else -1) + 0.05 * float(r(1))
        k = float(cube[b, 0] * cam[b, 0] / center[b, 2]) / img_size  # source pixels per crop pixel
        A = k * torch.tensor([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]], dtype=torch.float64) @ torch.tensor([[1.0, 0.12], [0.0, 1.07]], dtype=torch.float64)
        cpix = torch.stack((cam[b, 2] + center[b, 0] * cam[b, 0] / center[b, 2], cam[b, 3] + flip * center[b, 1] * cam[b, 1] / center[b, 2])) + (r(2) - 0.5) * 6
        Minv[b, :2, :2] = A
        Minv[b, :2, 2] = cpix - A @ torch.full((2,), float(half_size), dtype=torch.float64)
        Minv[b, 2, 2] = 1.0
    cam, cube, center, Minv = cam.float(), cube.float(), center.float(), Minv.float()  # what the kernel is given
    M = torch.linalg.inv(Minv.double())
    par = torch.cat((Minv[:, :2].reshape(B, 6), cam, center, cube), 1).contiguous()
    uvd = (torch.rand(B, J, 3, generator=g) * 2 - 1) * 0.9
    pix = torch.rand(B, P, 3, generator=g) * 2 - 1
    dgam = torch.randn(B, J, P, generator=g)
    c = dict(cam=cam, cube=cube, center=center, M=M, Minv=Minv, par=par, uvd=uvd, pix=pix, dgam=dgam, img_size=img_size, flip=flip, half_size=half_size, planted=P >= 3)
    if c["planted"]:
        with torch.enable_grad():
            xyz = _uvd_restate(c, lambda v: v.double(), flip)["xyz"]
        pix[:, 0] = xyz[:, 0].float()
        pix[:, P - 1] = (xyz[:, J - 1] + 30.0 * torch.tensor([2.0, -1.0, 2.0], dtype=torch.float64) / 3.0).float()
    c["ref"], c["plain"] = _both(lambda t: _uvd_restate(c, t, flip))
    return c


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. kpf_pose_tokens_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
POSE_SHAPES = [(2, 37, 21, 108, True), (2, 37, 21, 105, True), (1, 50, 5, 20, False), (2, 13, 5, 24, False)]  # (B, N, J, ld, with pw); 24 - 4 * 5 = J - 1 pad columns
POSE_MARGIN = 1e-6  # a mask decision is compared where |(kernel - dis) / kernel| in float64 is larger than this


@functools.lru_cache(maxsize=None)
def pose_case(B, N, J, kernel):
    """Planted as in the inference test's point_assemble case: points on a ring at kernel * (1 +- 3e-5) (and, with N >= 16, * (1 +- 1e-3)) around a joint, a point
    on a joint (dis = 0, offsets 0, closeness 1), points with z = 0.99, nextafter(0.99, +-) and 1.0 next to joint 1."""
    g = _gen(B, N, J, int(10 * kernel))
    k32 = float(torch.tensor(kernel, dtype=torch.float32))
    joint = (torch.rand(B, J, 3, generator=g) - 0.5) * 1.2
    joint[:, 1] = torch.tensor([0.1, 0.1, 0.7])
    pcl = (torch.rand(B, N, 3, generator=g) * 2 - 1) * 0.9
    pw = torch.randn(B, N, J, generator=g)
    on_joint, z_masked, z_kept, inside, outside = [], [], [], [], []
    z99 = torch.tensor(0.99, dtype=torch.float32)
    for b in range(B):
        slots = iter(range(N - 1, -1, -1))

        def ring(j, f, ang):
            n = next(slots)
            d = torch.tensor([math.cos(ang), math.sin(ang), 0.0], dtype=torch.float64) * (k32 * f)
            pcl[b, n] = (joint[b, j].double() + d).float()
            return b, n, j

        inside.append(ring(3 % J, 1 - 3e-5, 0.3))
        outside.append(ring(3 % J, 1 + 3e-5, 0.3))
        n = next(slots)
        pcl[b, n] = joint[b, 0]
        on_joint.append((b, n, 0))
        n = next(slots)
        pcl[b, n] = torch.tensor([0.1, 0.1, z99])
        z_masked.append((b, n))
        if N >= 16:
            inside += [ring(J - 1, 1 - 1e-3, 2.0), ring(2, 1 - 3e-5, 4.0)]
            outside += [ring(J - 1, 1 + 1e-3, 2.0), ring(2, 1 + 3e-5, 4.0)]
            n = next(slots)
            pcl[b, n] = joint[b, J - 1]
            on_joint.append((b, n, J - 1))
            for z, lst in ((torch.nextafter(z99, torch.tensor(2.0)), z_masked), (torch.tensor(1.0), z_masked), (torch.nextafter(z99, torch.tensor(0.0)), z_kept)):
                n = next(slots)
                pcl[b, n] = torch.tensor([0.1 + 0.01 * len(lst), 0.1, z])
                lst.append((b, n))
    ref = {"off": O.pcl_joint2offset(joint.double(), pcl.double(), k32)}
    plain = {"off": O.pcl_joint2offset(joint, pcl, kernel)}
    dis = torch.sqrt(((joint.double().unsqueeze(2) - pcl.double().unsqueeze(1)) ** 2).sum(-1))  # B J N
    clos_unmasked = ((k32 - dis) / k32).permute(0, 2, 1)                                         # B N J
    compared = clos_unmasked.abs() > POSE_MARGIN
    mask_of = lambda o: (o[..., :3 * J].reshape(B, N, J, 3) != 0).any(-1) | (o[..., 3 * J:] != 0)
    keep = torch.cat((compared.unsqueeze(-1).expand(B, N, J, 3).reshape(B, N, 3 * J), compared), -1)
    return dict(joint=joint, pcl=pcl, pw=pw, kernel=kernel, k32=k32, ref=ref, plain=plain, compared=compared, keep=keep, mask_of=mask_of, mask64=mask_of(ref["off"]),
                mask32=mask_of(plain["off"]), left_out=1.0 - float(compared.double().mean()), clos_unmasked=clos_unmasked, dis=dis, on_joint=on_joint, z_masked=z_masked,
                z_kept=z_kept, inside=inside, outside=outside, z_joint=1)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 5. kpf_gate_mix_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
# (B, J, P, weight_dis, d_sw given): P < 8 and R = B * J = 21 < 32 row groups; 300 = 256 + 44 = 8 * 37 + 4; R = 15; the workload's P
GATE_MIX_CASES = [(1, 21, 5, 0.3, True), (1, 21, 5, -3.0, False), (2, 21, 300, -3.0, True), (2, 21, 300, 6.0, False), (3, 5, 64, 0.3, False), (3, 5, 64, 6.0, True),
                  (2, 21, 1024, 0.3, True)]


@functools.lru_cache(maxsize=None)
def gate_mix_case(B, J, P, wdis, with_dsw):
    """A tenth of the logits at +-30 (`saturated` marks them): the fp32 sigmoid is 1 or ~1e-13 there and d_logits goes to 0.  The backward is given sw as the
    float64 sigmoid rounded to fp32."""
    g = _gen(B, J, P, int(10 * wdis) + 100, int(with_dsw))
    logits = torch.randn(B * P, J, generator=g) * 2
    saturated = torch.rand(B * P, J, generator=g) < 0.1
    logits[saturated] = torch.where(torch.rand(int(saturated.sum()), generator=g) < 0.5, 30.0, -30.0)
    gam = torch.rand(B, J, P, generator=g) * 0.999 + 0.001
    w_fc = torch.randn(P, generator=g)
    wd_ = torch.tensor([wdis], dtype=torch.float32)
    d_gw = torch.randn(B, J, P, generator=g)
    d_sw = torch.randn(B, J, P, generator=g) if with_dsw else None

    def run(t):
        lg, ga, wd0, wf = (_leaf(t, v) for v in (logits, gam, wd_, w_fc))
        sw = torch.sigmoid(lg.view(B, P, J).permute(0, 2, 1))
        wd = torch.sigmoid(wd0)
        gw = (wd * ga + (1 - wd) * sw) * wf.view(1, 1, P)
        loss = (gw * t(d_gw)).sum()
        if with_dsw:
            loss = loss + (sw * t(d_sw)).sum()
        loss.backward()
        return {"sw": sw.detach(), "gw": gw.detach(), "d_gam": ga.grad, "d_logits": lg.grad, "d_w_fc": wf.grad, "d_weight_dis": wd0.grad}

    ref, plain = _both(run)
    return dict(logits=logits, gam=gam, w_fc=w_fc, wd=wd_, d_gw=d_gw, d_sw=d_sw, sw_in=ref["sw"].float().contiguous(), saturated=saturated, ref=ref, plain=plain)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 6. kpf_group_max_train_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
GROUP_MAX_SHAPES = [(5, 64, 132, 132), (3, 7, 8, 12), (4, 1, 4, 4), (2, 256, 4, 8)]  # (rows, group, C, dy_ld)


@functools.lru_cache(maxsize=None)
def group_max_case(rows, group, C):
    """Planted ties: row 0 holds its exact maximum at members m1 < m2 in every channel (arg must be m1); row 1 is constant (arg 0); the first half of the channels of
    the other rows hold small integers, so most of their maxima are repeated.  arg = the first index of the maximum, computed as such."""
    g = _gen(rows, group, C, 6)
    x = torch.randn(rows, group, C, generator=g)
    x[2:, :, :C // 2] = torch.randint(0, 4, (max(rows - 2, 0), group, C // 2), generator=g).float()
    m1, m2 = (group // 3, group - 1) if group > 1 else (0, 0)
    x[0, m1] = x[0, m2] = x[0].amax(0) + 1.0
    x[1] = 0.5
    dy = torch.randn(rows, C, generator=g)
    y = x.amax(1)
    members = torch.arange(group).view(1, group, 1)
    arg = torch.where(x == y.unsqueeze(1), members, group).amin(1)  # first index of the maximum
    dx = torch.where(members == arg.unsqueeze(1), dy.unsqueeze(1), torch.zeros(()))
    return dict(x=x, dy=dy, y=y, arg=arg.to(torch.uint8), dx=dx, m1=m1, m2=m2)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 7. kpf_ball_group_stacked_f32 and kpf_ball_group_bwd_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
RADII = (0.1, 0.2, 0.4)
BALL_J = 21
BALL_MARGIN = 1e-5  # no pair's squared distance lies within this (relative) of a squared radius
BALL_NS = [40, 130]


@functools.lru_cache(maxsize=None)
def ball_group_case(N, B=2):
    """Joint 0 far from everything (its balls hold its own centre alone); with N = 130, seventy points within 0.3 of joint 1 (its r = 0.4 ball is truncated to the first
    64 members in index order); points at r * (1 +- 1e-3) from joint 2 for each radius; the rest a cloud of the joints' extent."""
    g = _gen(N, B, 7)
    joint = (torch.rand(B, BALL_J, 3, generator=g) - 0.5) * 0.8
    joint[:, 0] = torch.tensor([3.0, 3.0, 3.0])
    pcl = (torch.rand(B, N, 3, generator=g) - 0.5) * 0.9
    crowded = N + BALL_J > 64 + 6
    unit = lambda: torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
    pairs = []
    for b in range(B):
        n = N - 1
        for ri, r in enumerate(RADII):
            r32 = float(torch.tensor(r, dtype=torch.float32))
            for f in (1 - 1e-3, 1 + 1e-3):
                pcl[b, n] = (joint[b, 2].double() + unit() * (r32 * f)).float()
                pairs.append((b, ri, n, f < 1))
                n -= 1
        if crowded:
            for i in range(70):
                pcl[b, 2 * i % (N - 6)] = (joint[b, 1].double() + unit() * 0.3 * float(torch.rand(1, generator=g))).float()
    X = torch.randn(B, N, 128, generator=g)
    JF = torch.randn(B, BALL_J, 128, generator=g)
    xyz = torch.cat((pcl, joint), 1)
    feat = torch.cat((X, JF), 1)
    idx = torch.stack([O.ball_query(r, 64, xyz, joint) for r in RADII])          # [3][B][J][64], fp32 as pointnet2's kernel
    idx64 = torch.stack([O.ball_query(r, 64, xyz.double(), joint.double()) for r in RADII])
    d2 = ((joint.double().unsqueeze(2) - xyz.double().unsqueeze(1)) ** 2).sum(-1)  # [B][J][N + J]
    r2 = torch.tensor([float(torch.tensor(r, dtype=torch.float32)) ** 2 for r in RADII], dtype=torch.float64)
    margin = float((d2.unsqueeze(-1) / r2 - 1).abs().min())
    members = torch.stack([(d2 < r2[i]).sum(-1) for i in range(3)])                # [3][B][J]

    def run(t):
        f, p = t(feat), t(xyz)
        gather = lambda v, ix: torch.gather(v.unsqueeze(1).expand(B, BALL_J, -1, -1), 2, ix.unsqueeze(-1).expand(-1, -1, -1, v.shape[-1]))
        GF = torch.cat([gather(f, idx[i]) - t(JF).unsqueeze(2) for i in range(3)], -1)  # [B][J][64][384]
        GX = torch.cat([torch.cat(((gather(p, idx[i]) - t(joint).unsqueeze(2)) / t(torch.tensor(RADII[i], dtype=torch.float32)), torch.zeros(B, BALL_J, 64, 1, dtype=f.dtype)), -1)
                        for i in range(3)], -1)
        return {"GF": GF.reshape(B * BALL_J * 64, 384), "GX": GX.reshape(B * BALL_J * 64, 12)}

    ref, plain = _both(run)
    return dict(pcl=pcl, joint=joint, X=X, JF=JF, idx=idx.to(torch.int32), idx64=idx64.to(torch.int32), margin=margin, members=members, pairs=pairs, crowded=crowded,
                d2=d2, r2=r2, ref=ref, plain=plain, B=B)


BALL_BWD = dict(B=2, N=40, Jn=5)
BALL_BWD_COUNTS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65)  # list lengths a source row must own in some radius image; and one of 129 or more
BALL_BWD_LD3 = [384, 388]


@functools.lru_cache(maxsize=None)
def ball_bwd_indices():
    """idx [3][B][Jn * 64] by hand.  An image is one (radius, sample): R = 320 entries over P = N + Jn = 45 source rows, so the required list lengths (their sum
    is 468) are spread over three images; in each the rows and their lengths are listed as (row, length) and the entries are dealt out in a seeded shuffle."""
    B, N, Jn = BALL_BWD["B"], BALL_BWD["N"], BALL_BWD["Jn"]
    P, R = N + Jn, Jn * 64
    plans = {(0, 0): [(3, 129), (N + 1, 65), (7, 64), (0, 33), (N + 4, 17), (P - 1 - 2, 2), (11, 1), (12, 9)],   # a heavy point row; joint rows among the others
             (1, 0): [(N + 2, 163), (5, 63), (N, 32), (39, 31), (20, 16), (21, 15)],                              # a heavy joint row
             (2, 1): [(N - 1, 140), (N + 3, 140), (1, 17), (2, 16), (8, 7)]}
    g = _gen(B, N, Jn, 77)
    idx = torch.randint(0, P, (3, B, R), generator=g, dtype=torch.int32)
    for (i, b), plan in plans.items():
        assert sum(n for _, n in plan) == R, (i, b)
        flat = torch.cat([torch.full((n,), p, dtype=torch.int32) for p, n in plan])
        idx[i, b] = flat[torch.randperm(R, generator=g)]
    counts = torch.stack([torch.bincount(idx[i, b].long(), minlength=P) for i in range(3) for b in range(B)]).view(3, B, P)
    return idx.contiguous(), counts


@functools.lru_cache(maxsize=None)
def ball_bwd_case(ld3):
    B, N, Jn = BALL_BWD["B"], BALL_BWD["N"], BALL_BWD["Jn"]
    P, R = N + Jn, Jn * 64
    idx, counts = ball_bwd_indices()
    g = _gen(ld3, 78)
    d3 = torch.randn(B * R, 384, generator=g)

    def run(t):
        d = t(d3).view(B, R, 3, 128)
        full = torch.zeros(B, P, 128, dtype=d.dtype)
        for b in range(B):
            for i in range(3):  # radius ascending, entries ascending
                full[b].index_add_(0, idx[i, b].long(), d[b, :, i])
        centre = d.view(B, Jn, 64, 3, 128).sum((2, 3))
        return {"dX": full[:, :N].contiguous(), "dnode": full[:, N:] - centre}

    ref, plain = _both(run)
    return dict(idx=idx, counts=counts, d3=d3, ref=ref, plain=plain, P=P, R=R, **BALL_BWD)


def stable_inverse(idx, P):
    """idx [B][E] -> (start [B][P + 1], list [B][E]): the entries sorted by source row, entry order kept within a row."""
    B, E = idx.shape
    order = torch.sort(idx.long(), dim=1, stable=True).indices
    cnt = torch.stack([torch.bincount(idx[b].long(), minlength=P) for b in range(B)])
    start = torch.cat((torch.zeros(B, 1, dtype=torch.long), torch.cumsum(cnt, 1)), 1)
    return start.to(torch.int32), order.to(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 8. kpf_row_gather_fwd_f32, _cols_f32, _invert, _accum_f32, _bwd_f32
# ----------------------------------------------------------------------------------------------------------------------------------------
# (B, P, R, G, C, weights given)
GATHER_CASES = [(2, 37, 50, 3, 8, True), (2, 37, 50, 3, 8, False),
                (2, 2049, 375, 4, 4, True),     # the 8-wave inversion with E = 1500 entries: every wave owns some
                (1, 3, 8192, 1, 4, False),      # every entry in the last row: 128 chunks of 64
                (2, 64, 40, 2, 132, True),      # C / 4 = 33: no half-waves, 31 dead lanes
                (1, 20, 30, 1, 260, False)]     # C / 4 = 65: two trips, 63 dead lanes in the second
GATHER_COLS = (2, 37, 50, 3, 21)  # (B, P, R, G, C): the source is NCHW planes


def _gather_idx(g, B, P, E):
    """Entries over the source rows that are no multiple of 5 (those own nothing), the last row P - 1 used; P = 3: every entry in row 2."""
    if P == 3:
        return torch.full((B, E), 2, dtype=torch.int32)
    allowed = torch.tensor([p for p in range(P) if p % 5], dtype=torch.int32)
    idx = allowed[torch.randint(0, len(allowed), (B, E), generator=g)]
    idx[:, E // 2] = P - 1
    idx[:, 0] = P - 1
    return idx.contiguous()


def _gather_fwd(t, src, idx, w, B, R, G):
    C = src.shape[-1]
    rows = torch.gather(t(src), 1, idx.long().unsqueeze(-1).expand(-1, -1, C)).view(B, R, G, C)
    return (rows * t(w).view(B, R, G, 1)).sum(2) if w is not None else rows.sum(2)


@functools.lru_cache(maxsize=None)
def gather_case(B, P, R, G, C, with_w):
    g = _gen(B, P, R, G, C, int(with_w))
    E = R * G
    src = torch.randn(B, P, C, generator=g)
    idx = _gather_idx(g, B, P, E)
    w = torch.randn(B, E, generator=g) if with_w else None
    dout = torch.randn(B, R, C, generator=g)

    def run(t):
        out = _gather_fwd(t, src, idx, w, B, R, G)
        contrib = t(dout).unsqueeze(2).expand(B, R, G, C).reshape(B, E, C)
        if w is not None:
            contrib = contrib * t(w).unsqueeze(-1)
        dsrc = torch.zeros(B, P, C, dtype=contrib.dtype)
        for b in range(B):
            dsrc[b].index_add_(0, idx[b].long(), contrib[b])
        return {"out": out, "dsrc": dsrc}

    ref, plain = _both(run)
    start, lst = stable_inverse(idx, P)
    return dict(src=src, idx=idx, w=w, dout=dout, ref=ref, plain=plain, start=start, list=lst, counts=start[:, 1:] - start[:, :-1])


@functools.lru_cache(maxsize=None)
def gather_cols_case(with_w):
    B, P, R, G, C = GATHER_COLS
    g = _gen(B, P, R, G, C, int(with_w), 9)
    planes = torch.randn(B, C, P, generator=g)  # NCHW: element (b, p, c) at b * C * P + c * P + p
    idx = _gather_idx(g, B, P, R * G)
    w = torch.randn(B, R * G, generator=g) if with_w else None
    ref, plain = _both(lambda t: {"out": _gather_fwd(t, planes.permute(0, 2, 1), idx, w, B, R, G)})
    return dict(planes=planes, idx=idx, w=w, ref=ref, plain=plain)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 9. kpf_attn21_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
ATTN_T, ATTN_HD = 21, 32
ATTN_SHAPES = [(3, 4, 128, 128), (1, 1, 32, 32), (2, 4, 384, 128), (2, 4, 128, 160)]  # (B, H, ld, ldc); 384: q, k, v are column slices of one buffer
ATTN_SCALES = [32 ** -0.5, 1.0]
ATTN_SHARP_STD = 16.0  # "about 15": at 15.0 the share of rows with a probability above 0.99 is 0.5 +- the noise of 21 to 252 rows, at 16.0 it clears one half


@functools.lru_cache(maxsize=None)
def attn_inputs(B, H, scale, kind):
    """q, k, v, dctx [B * 21][H * 32].  sharp: q and k scaled so that the logits scale * q . k have a standard deviation of ATTN_SHARP_STD."""
    g = _gen(B, H, int(1000 * scale), int(kind == "sharp"), 14)
    q, k, v, dctx = (torch.randn(B * ATTN_T, H * ATTN_HD, generator=g) for _ in range(4))
    if kind == "sharp":
        a = math.sqrt(ATTN_SHARP_STD / (scale * math.sqrt(ATTN_HD)))
        q, k = q * a, k * a
    return q, k, v, dctx


def attn_restate(t, q, k, v, dctx, B, H, scale, keep=None, p_drop=0.0):
    """softmax(scale q k^T) per (sample, head), dropout by the given keep mask [B][H][21][21] (1 / (1 - p) on what is kept), times v; gradients by autograd."""
    heads = lambda x: x.view(B, ATTN_T, H, ATTN_HD).transpose(1, 2)
    ql, kl, vl = (_leaf(t, x) for x in (q, k, v))
    P = torch.softmax(scale * (heads(ql) @ heads(kl).transpose(-1, -2)), -1)
    Pd = P if keep is None else P * t(keep) / (1.0 - p_drop)
    ctx = (Pd @ heads(vl)).transpose(1, 2).reshape(B * ATTN_T, H * ATTN_HD)
    (ctx * t(dctx)).sum().backward()
    return {"P": P.detach(), "ctx": ctx.detach(), "dq": ql.grad, "dk": kl.grad, "dv": vl.grad}


@functools.lru_cache(maxsize=None)
def attn_case(B, H, scale, kind):
    q, k, v, dctx = attn_inputs(B, H, scale, kind)
    ref, plain = _both(lambda t: attn_restate(t, q, k, v, dctx, B, H, scale))
    return dict(q=q, k=k, v=v, dctx=dctx, ref=ref, plain=plain, P_in=ref["P"].float().contiguous(), sharp_share=float((ref["P"].amax(-1) > 0.99).double().mean()))


def attn_dropout_refs(B, H, scale, kind, keep, p_drop):
    """The same restatement replayed with a keep mask read back from the kernel (bytes [B][H][21][21])."""
    q, k, v, dctx = attn_inputs(B, H, scale, kind)
    keep = keep.to(torch.float32)
    return _both(lambda t: attn_restate(t, q, k, v, dctx, B, H, scale, keep, p_drop))
