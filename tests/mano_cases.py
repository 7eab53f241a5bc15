"""Inputs and float64 restatements for the MANO layer's backward kernel and the joint fit (kpf_mano_backward_f32, kpf_mano_fit_f32).  No GPU.

The reference of every comparison is torch autograd, in float64, of the oracle's restatement of the head's tail (oracle/aux_oracle.py: rot6d_to_mat, mat_to_quat,
quat_to_aa, mano_layer).  A kernel result passes by the project's rule for fp32 kernels (tests/wgrad_forms.py): e_kernel <= 4 e_plain + 8 * 2^-24, where e_plain is
how far fp32 torch-CPU autograd of the SAME restatement is from the float64 one — the bound comes from the reference's own fp32 error, not from the kernel.
The only inputs excluded from a float64 comparison are exact identity and exact 180-degree turns (autograd's NaN, and an arbitrary axis sign); neither is in
grad_case, and identity_case has its own finite reference."""
import functools
import math

import numpy as np
import torch

from oracle import aux_oracle as A
from test_heads_oracle import mano_case

FLOOR = 8 * 2.0 ** -24
OUTPUTS = ("verts3d", "joints3d", "mano_pose", "mano_pose_aa")


def within(e_kernel, e_plain, scale=1.0):
    return e_kernel <= 4 * e_plain + FLOOR * scale


@functools.lru_cache(maxsize=None)
def model_sd():
    """the synthetic hand's tensors, float32 (as the kernels get them)"""
    return {k: v for k, v in mano_case()[0].items() if k.startswith("mano_layer.")}


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def quat_to_aa_safe(q):
    """A.quat_to_aa with the double-`where` form: a safe divisor where s2 == 0, then k = 2 there — the same forward values, and a finite derivative at identity
    (the derivative of the k = 2 branch the forward takes), where the single-`where` form differentiates sqrt at 0."""
    q1, q2, q3 = q[:, 1], q[:, 2], q[:, 3]
    s2 = q1 * q1 + q2 * q2 + q3 * q3
    pos = s2 > 0.0
    s = torch.sqrt(torch.where(pos, s2, torch.ones_like(s2)))
    c = q[:, 0]
    two_theta = 2.0 * torch.where(c < 0.0, torch.atan2(-s, -c), torch.atan2(s, c))
    k = torch.where(pos, two_theta / s, torch.full_like(s, 2.0))
    aa = torch.stack([q1 * k, q2 * k, q3 * k], -1)
    return torch.where(torch.isnan(aa), torch.zeros_like(aa), aa)


def head_tail(sd, pose6d, betas, safe=False):
    """what kpf_mano_forward_f32 computes: (verts3d, joints3d in the head's order, mano_pose, mano_pose_aa)"""
    R = A.rot6d_to_mat(pose6d.reshape(-1, 6))
    aa = (quat_to_aa_safe if safe else A.quat_to_aa)(A.mat_to_quat(R)).reshape(-1, 48)
    verts, joints = A.mano_layer(sd, aa, betas)
    return verts, joints[:, list(A.OBMAN2MANO)], R.view(-1, 16, 3, 3), aa


def gradients(pose6d, betas, projs, dtype, which=(0, 1, 2, 3), safe=False):
    """autograd of sum_i <output_i, proj_i> over the outputs in `which` -> (d_pose6d, d_betas) in `dtype`"""
    p6, bt = pose6d.to(dtype).clone().requires_grad_(True), betas.to(dtype).clone().requires_grad_(True)
    outs = head_tail(_cast(model_sd(), dtype), p6, bt, safe)
    loss = sum((outs[i] * projs[i].to(dtype)).sum() for i in which)
    g = torch.autograd.grad(loss, (p6, bt), allow_unused=True)  # the rotations and the axis-angle do not depend on betas
    return tuple(torch.zeros_like(x) if d is None else d for d, x in zip(g, (p6, bt)))


def _axis_rot(deg, axis):
    a = torch.tensor(axis, dtype=torch.float64)
    return A.rodrigues((a / a.norm() * math.radians(deg))[None])[0]


def branch_counts(pose6d):
    """how many of the rotations take each of the four quaternion branches (model/mano_head.py:84-141, on the transpose)"""
    m = A.rot6d_to_mat(pose6d.reshape(-1, 6).float()).transpose(1, 2)
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    d2, d01, d0n1 = m22 < 1e-6, m00 > m11, m00 < -m11
    return [int(c.sum()) for c in (d2 & d01, d2 & ~d01, ~d2 & d0n1, ~d2 & ~d0n1)]


class Case:
    pass


def _projections(gen, B):
    return [torch.rand(B, *s, generator=gen, dtype=torch.float64).mul(2).sub(1).float() for s in ((778, 3), (21, 3), (16, 3, 3), (48,))]


def _finish(c, safe):
    c.ref = gradients(c.pose6d, c.betas, c.projs, torch.float64, safe=safe)
    c.plain = gradients(c.pose6d, c.betas, c.projs, torch.float32, safe=safe)
    c.safe = safe
    return c


@functools.lru_cache(maxsize=None)
def grad_case():
    """B = 5.  Every joint's 6D input is one of six rotations (170 degrees about z, x and y: the three branches off the main one, each near its 180-degree
    edge; 20, 95 and 3 degrees about oblique axes), its two column vectors given unequal lengths and a skew, plus 0.02 Gaussian noise; sample 0 is fully random."""
    gen = torch.Generator().manual_seed(11)
    B = 5
    rots = torch.stack([_axis_rot(170, (0, 0, 1)), _axis_rot(170, (1, 0, 0)), _axis_rot(170, (0, 1, 0)), _axis_rot(20, (1, 2, -1)),
                        _axis_rot(95, (-2, 1, 3)), _axis_rot(3, (3, -1, 2))])
    pick = torch.randint(0, 6, (B, 16), generator=gen)
    R = rots[pick]  # [B, 16, 3, 3]
    len1 = 0.5 + 1.5 * torch.rand(B, 16, 1, generator=gen, dtype=torch.float64)
    len2 = 0.5 + 1.5 * torch.rand(B, 16, 1, generator=gen, dtype=torch.float64)
    skew = torch.rand(B, 16, 1, generator=gen, dtype=torch.float64) - 0.5
    a1 = R[..., 0] * len1
    a2 = R[..., 1] * len2 + skew * a1
    six = torch.cat([a1, a2], -1) + 0.02 * torch.randn(B, 16, 6, generator=gen, dtype=torch.float64)
    six[0] = torch.randn(16, 6, generator=gen, dtype=torch.float64)
    c = Case()
    c.pose6d = six.reshape(B, 96).float()
    c.betas = (0.5 * torch.randn(B, 10, generator=gen, dtype=torch.float64)).float()
    c.projs = _projections(gen, B)
    c.single = {i: (gradients(c.pose6d, c.betas, c.projs, torch.float64, (i,)), gradients(c.pose6d, c.betas, c.projs, torch.float32, (i,))) for i in range(4)}
    return _finish(c, False)


@functools.lru_cache(maxsize=None)
def identity_case():
    """Sample 0 is exactly (1, 0, 0, 0, 1, 0) x 16; sample 1 is sample 1 of grad_case.  The reference is the double-`where` restatement (quat_to_aa_safe)."""
    g = grad_case()
    gen = torch.Generator().manual_seed(12)
    c = Case()
    c.pose6d = torch.stack([torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(16), g.pose6d[1]])
    c.betas = (0.5 * torch.randn(2, 10, generator=gen, dtype=torch.float64)).float()
    c.projs = _projections(gen, 2)
    return _finish(c, True)


def errors(c, d6, db, ref=None, plain=None):
    """-> {"d_pose6d": (e_kernel, e_plain), "d_betas": ...}, both relative to max|ref64| (absolute where the reference is identically zero)"""
    ref, plain = ref or c.ref, plain or c.plain
    out = {}
    for name, got, r, p in (("d_pose6d", d6, ref[0], plain[0]), ("d_betas", db, ref[1], plain[1])):
        den = float(r.abs().max()) or 1.0
        out[name] = (float((got.detach().cpu().double() - r).abs().max()) / den, float((p.double() - r).abs().max()) / den)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------
# the fit
# ----------------------------------------------------------------------------------------------------------------------------------------
FIT_LR, FIT_EPS, FIT_LAMBDA_SHAPE = (0.02, 0.05, 1.0), 1.0, 1.0


def _f32(v):
    return float(np.float32(v))  # the kernel's configuration holds float32 numbers: the restatement steps with the same values


@functools.lru_cache(maxsize=None)
def fit_inputs():
    """B = 3 synthetic hands at aa ~ 0.3 N, betas ~ 0.5 N, shifted by (30, -20, 600) mm; sample 1 has two zero weights.  Starts: zeros, or the truth + 0.1 noise."""
    gen = torch.Generator().manual_seed(21)
    B = 3
    c = Case()
    c.aa = (0.3 * torch.randn(B, 48, generator=gen, dtype=torch.float64)).float()
    c.betas = (0.5 * torch.randn(B, 10, generator=gen, dtype=torch.float64)).float()
    c.trans = torch.tensor([30.0, -20.0, 600.0]).repeat(B, 1)
    _, j = A.mano_layer(_cast(model_sd(), torch.float64), c.aa.double(), c.betas.double())
    c.target = (j[:, list(A.OBMAN2MANO)] + c.trans[:, None].double()).float().contiguous()
    c.weight = torch.ones(B, 21)
    c.weight[1, 4] = c.weight[1, 17] = 0.0
    noise = lambda n: (0.1 * torch.randn(B, n, generator=gen, dtype=torch.float64)).float()  # noqa: E731
    c.starts = {"zeros": (torch.zeros(B, 48), torch.zeros(B, 10), torch.zeros(B, 3)),
                "near": (c.aa + noise(48), c.betas + noise(10), c.trans + noise(3))}
    return c


def fit_reference(dtype, target, weight, start, iters, lr=FIT_LR, eps=FIT_EPS, lambda_shape=FIT_LAMBDA_SHAPE, lambda_pose=0.0, init_trans=True,
                  adam_betas=(0.9, 0.999)):
    """The fit restated with oracle.aux_oracle.mano_layer and torch.optim.Adam, in `dtype` -> dict(pose_aa, betas, trans, joints, verts, residual [B, 2])."""
    sd = _cast(model_sd(), dtype)
    w = weight.to(dtype)
    y = torch.where(w[..., None] > 0, target.to(dtype), torch.zeros((), dtype=dtype))
    th, be, tr = [s.detach().clone().to(dtype).requires_grad_(True) for s in start]
    sw = w.sum(1)

    def model():
        v, j = A.mano_layer(sd, th, be)
        return v, j[:, list(A.OBMAN2MANO)]

    def residual(j):
        return (w * (j + tr[:, None] - y).norm(dim=-1)).sum(1) / sw

    with torch.no_grad():
        j = model()[1]
        if init_trans and iters > 0:
            tr.copy_((w[..., None] * (y - j)).sum(1) / sw[:, None])
        res0 = residual(j)
    opt = torch.optim.Adam([{"params": [th], "lr": _f32(lr[0])}, {"params": [be], "lr": _f32(lr[1])}, {"params": [tr], "lr": _f32(lr[2])}],
                           betas=(_f32(adam_betas[0]), _f32(adam_betas[1])), eps=_f32(eps))
    for _ in range(iters):
        opt.zero_grad()
        r = model()[1] + tr[:, None] - y
        loss = (w * (r * r).sum(-1)).sum(1) / sw + _f32(lambda_shape) * (be * be).sum(1) + _f32(lambda_pose) * (th[:, 3:] * th[:, 3:]).sum(1)
        loss.sum().backward()  # the samples are independent and Adam is element-wise: the batch sum steps every sample as if alone
        opt.step()
    with torch.no_grad():
        v, j = model()
        return {"pose_aa": th.detach(), "betas": be.detach(), "trans": tr.detach(), "joints": j + tr[:, None], "verts": v + tr[:, None],
                "residual": torch.stack([res0, residual(j)], 1)}


@functools.lru_cache(maxsize=None)
def fit_pair(start, iters):
    """(float64 reference, fp32 restatement) of the default fit from the named start"""
    c = fit_inputs()
    return tuple(fit_reference(dt, c.target, c.weight, c.starts[start], iters) for dt in (torch.float64, torch.float32))


def fit_errors(got, ref, plain):
    """-> {name: (e_kernel, e_plain, max|ref|)}, absolute"""
    out = {}
    for k in ("pose_aa", "betas", "trans", "joints", "verts"):
        r = ref[k].double()
        out[k] = (float((got[k].detach().cpu().double() - r).abs().max()), float((plain[k].double() - r).abs().max()), float(r.abs().max()))
    return out
