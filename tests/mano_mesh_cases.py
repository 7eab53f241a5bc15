"""Inputs and host restatements for the mesh fit and the point-to-vertex association (kpf_mano_fit_mesh_f32, kpf_mano_assoc_f32).  No GPU.

associate_host is the association restated in numpy float32, operation by operation: the kernel is held to its bits.  fit_mesh_reference is
mano_cases.fit_reference restated with the vertex term, the [B][4] residual and the new init_trans and status rules; the kernel is held to its float64
run under the project's rule (mano_cases.within), the fp32 run of the same restatement giving e_plain."""
import functools

import numpy as np
import torch

import mano_cases as M
from oracle import aux_oracle as A

NV = 778


# ----------------------------------------------------------------------------------------------------------------------------------------
# the association
# ----------------------------------------------------------------------------------------------------------------------------------------
def associate_host(points, weight, verts, max_dist2):
    """points [B, N, 3], weight [B, N] or None (= ones), verts [B, 778, 3], max_dist2 a number -> idx [B, N] int32, vert_target [B, 778, 3],
    vert_weight [B, 778], stats [B, 2], float32 numpy.  Every product, sum, quotient and root is one float32 operation (numpy fuses nothing)."""
    P, V = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(verts, np.float32)
    B, N = P.shape[:2]
    W = np.ones((B, N), np.float32) if weight is None else np.ascontiguousarray(weight, np.float32)
    gate = np.float32(max_dist2)
    idx = np.empty((B, N), np.int32)
    vt, vw, stats = np.zeros((B, NV, 3), np.float32), np.zeros((B, NV), np.float32), np.zeros((B, 2), np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            best, bi = np.full(N, np.inf, np.float32), np.zeros(N, np.int32)
            for v in range(NV):  # ascending, strict <
                dx, dy, dz = P[b, :, 0] - V[b, v, 0], P[b, :, 1] - V[b, v, 1], P[b, :, 2] - V[b, v, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                upd = d2 < best
                best, bi = np.where(upd, d2, best), np.where(upd, np.int32(v), bi)
            matched = (W[b] > 0) & np.isfinite(P[b]).all(1) & (best <= gate)
            idx[b] = np.where(matched, bi, -1)
            dist = np.sqrt(best)
            S, total, count = np.zeros((NV, 3), np.float32), np.float32(0), 0
            for n in np.nonzero(matched)[0]:  # ascending point index
                v, w = bi[n], W[b, n]
                vw[b, v] = vw[b, v] + w
                S[v] = S[v] + w * P[b, n]
                total = np.float32(total + dist[n])
                count += 1
            some = vw[b] > 0
            vt[b][some] = S[some] / vw[b][some, None]
            vw[b][~some] = 0
            stats[b] = (count, total / np.float32(count) if count else 0.0)
    return idx, vt, vw, stats


def argmin64(points, verts):
    """float64: (nearest vertex, its squared distance, the second nearest's squared distance), each [B, N]"""
    d2 = ((np.asarray(points, np.float64)[:, :, None] - np.asarray(verts, np.float64)[:, None]) ** 2).sum(-1)
    order = np.argsort(d2, axis=-1, kind="stable")[..., :2]
    two = np.take_along_axis(d2, order, -1)
    return order[..., 0], two[..., 0], two[..., 1]


@functools.lru_cache(maxsize=None)
def true_mesh():
    """float32 [3, 778, 3]: the vertices of fit_inputs()'s three hands, in mm with their translation"""
    c = M.fit_inputs()
    v, _ = A.mano_layer(M._cast(M.model_sd(), torch.float64), c.aa.double(), c.betas.double())
    return (v + c.trans[:, None].double()).float().contiguous()


CLOUD_SIGMA = 0.5  # mm


@functools.lru_cache(maxsize=None)
def cloud():
    """float32 [3, 519, 3]: the true mesh's vertices with index % 3 < 2 plus a seeded 0.5 mm Gaussian -- two thirds of the skin, seen by a noisy sensor"""
    keep = torch.arange(NV) % 3 < 2
    v = true_mesh()[:, keep]
    noise = torch.randn(v.shape, generator=torch.Generator().manual_seed(31), dtype=torch.float64)
    return (v.double() + CLOUD_SIGMA * noise).float().contiguous()


def sized_cloud(N, seed=32):
    """float32 [3, N, 3] and weights [3, N] for the bit comparisons: N vertices of the true mesh drawn with replacement, 2 mm of noise (so that some points do
    tie or sit between vertices), weights in (0, 2] with every seventh 0"""
    gen = torch.Generator().manual_seed(seed + N)
    pick = torch.randint(0, NV, (3, N), generator=gen)
    v = torch.gather(true_mesh(), 1, pick[..., None].expand(3, N, 3))
    pts = (v.double() + 2.0 * torch.randn(3, N, 3, generator=gen, dtype=torch.float64)).float().contiguous()
    w = (2.0 * torch.rand(3, N, generator=gen, dtype=torch.float64)).float() + 2.0 ** -10
    w[:, 3::7] = 0.0
    return pts, w.contiguous()


def hand_made():
    """One hand (the first true mesh) and seven points, each there for one rule:
      0, 1  two points on vertex 5 with weights 1 and 3 (a centroid of two, in index order)
      2     500 mm away: gated at max_dist 20
      3     a NaN coordinate
      4     weight 0 (it sits exactly on vertex 9)
      5     an exact tie: verts 700 and 701 are made the same position, the point sits on it -> 700
      6     exactly on vertex 12: the only hit at max_dist2 = 0 besides 5 (points 0, 1 are off their vertex)
    -> points [1, 7, 3], weight [1, 7], verts [1, 778, 3]"""
    verts = true_mesh()[:1].clone()
    verts[0, 701] = verts[0, 700]
    p = torch.zeros(1, 7, 3)
    p[0, 0] = verts[0, 5] + torch.tensor([0.25, 0.0, -0.125])
    p[0, 1] = verts[0, 5] + torch.tensor([-0.125, 0.25, 0.0])
    p[0, 2] = verts[0, 5] + torch.tensor([0.0, 500.0, 0.0])
    p[0, 3] = verts[0, 20]
    p[0, 3, 1] = float("nan")
    p[0, 4] = verts[0, 9]
    p[0, 5] = verts[0, 700]
    p[0, 6] = verts[0, 12]
    w = torch.tensor([[1.0, 3.0, 1.0, 1.0, 0.0, 1.0, 1.0]])
    return p.contiguous(), w, verts.contiguous()


# ----------------------------------------------------------------------------------------------------------------------------------------
# the fit with a vertex term
# ----------------------------------------------------------------------------------------------------------------------------------------
def fit_mesh_reference(dtype, target, weight, vert_target, vert_weight, start, iters, lr=M.FIT_LR, eps=M.FIT_EPS, lambda_shape=M.FIT_LAMBDA_SHAPE,
                       lambda_pose=0.0, lambda_verts=1.0, init_trans=True, adam_betas=(0.9, 0.999)):
    """L = [sw > 0] (1/sw) sum_i w_i |J_i + t - y_i|^2 + lambda_verts [sv > 0] (1/sv) sum_v u_v |V_v + t - c_v|^2 + lambda_shape |beta|^2
    + lambda_pose |theta[3:]|^2 by torch.optim.Adam in `dtype` -> dict(pose_aa, betas, trans, joints, verts, residual [B, 4], status [B]).
    target=None: no joint carries weight.  vert_weight=None: no vertex term, and the result is fit_reference's, tensor for tensor.  A sample with a status
    bit keeps its state and is only evaluated."""
    sd = M._cast(M.model_sd(), dtype)
    B = start[0].shape[0]
    zero = torch.zeros((), dtype=dtype)
    w = torch.zeros(B, 21, dtype=dtype) if target is None else (torch.ones(B, 21, dtype=dtype) if weight is None else weight.to(dtype))
    y = torch.zeros(B, 21, 3, dtype=dtype) if target is None else torch.where(w[..., None] > 0, target.to(dtype), zero)
    has_v = vert_weight is not None
    u = vert_weight.to(dtype) if has_v else torch.zeros(B, NV, dtype=dtype)
    c = torch.where(u[..., None] > 0, vert_target.to(dtype), zero) if has_v else torch.zeros(B, NV, 3, dtype=dtype)
    sw, sv = w.sum(1), u.sum(1)
    status = (((sw <= 0) & (sv <= 0)).int() + 2 * (~(torch.isfinite(y).all(-1).all(-1) & torch.isfinite(c).all(-1).all(-1))).int()).int()
    ok = status == 0
    out = {"status": status}

    def run(rows, n_iters):
        """the fit of the samples `rows` (a bool mask) for n_iters"""
        w_, y_, u_, c_, sw_, sv_ = w[rows], y[rows], u[rows], c[rows], sw[rows], sv[rows]
        jw, vw = sw_ > 0, sv_ > 0
        swd, svd = torch.where(jw, sw_, torch.ones_like(sw_)), torch.where(vw, sv_, torch.ones_like(sv_))
        th, be, tr = [s[rows].detach().clone().to(dtype).requires_grad_(True) for s in start]

        def model():
            v, j = A.mano_layer(sd, th, be)
            return v, j[:, list(A.OBMAN2MANO)]

        def residual(v, j):
            rj = torch.where(jw, (w_ * (j + tr[:, None] - y_).norm(dim=-1)).sum(1) / swd, zero)
            rv = torch.where(vw, (u_ * (v + tr[:, None] - c_).norm(dim=-1)).sum(1) / svd, zero)
            return rj, rv

        with torch.no_grad():
            v, j = model()
            if init_trans and n_iters > 0:
                tj = (w_[..., None] * (y_ - j)).sum(1) / swd[:, None]
                tv = (u_[..., None] * (c_ - v)).sum(1) / svd[:, None]
                tr.copy_(torch.where(jw[:, None], tj, tv))
            res0 = residual(v, j)
        opt = torch.optim.Adam([{"params": [th], "lr": M._f32(lr[0])}, {"params": [be], "lr": M._f32(lr[1])}, {"params": [tr], "lr": M._f32(lr[2])}],
                               betas=(M._f32(adam_betas[0]), M._f32(adam_betas[1])), eps=M._f32(eps))
        for _ in range(n_iters):
            opt.zero_grad()
            v, j = model()
            r = j + tr[:, None] - y_
            loss = torch.where(jw, (w_ * (r * r).sum(-1)).sum(1) / swd, zero)
            if has_v:
                rv = v + tr[:, None] - c_
                loss = loss + M._f32(lambda_verts) * torch.where(vw, (u_ * (rv * rv).sum(-1)).sum(1) / svd, zero)
            loss = loss + M._f32(lambda_shape) * (be * be).sum(1) + M._f32(lambda_pose) * (th[:, 3:] * th[:, 3:]).sum(1)
            loss.sum().backward()  # the samples are independent and Adam is element-wise: the batch sum steps every sample as if alone
            opt.step()
        with torch.no_grad():
            v, j = model()
            res1 = residual(v, j)
            return {"pose_aa": th.detach(), "betas": be.detach(), "trans": tr.detach(), "joints": j + tr[:, None], "verts": v + tr[:, None],
                    "residual": torch.stack([res0[0], res1[0], res0[1], res1[1]], 1)}

    parts = [(ok, run(ok, iters))] if bool(ok.any()) else []
    if not bool(ok.all()):
        parts.append((~ok, run(~ok, 0)))
    for k in parts[0][1]:
        full = torch.zeros((B,) + tuple(parts[0][1][k].shape[1:]), dtype=dtype)
        for rows, res in parts:
            full[rows] = res[k]
        out[k] = full
    return out


def mesh_targets(kind):
    """The vertex inputs of the GPU cases -> (target or None, weight or None, vert_target, vert_weight)
      both    the joints of fit_inputs() and every vertex of the true mesh, u = 1
      verts   vertices only: the entry gets target = NULL
      zerow   vertices only, the joint weights given as all 0 (the other way to say it)
      third   joints, and the vertices with a third of the weights 0 and NaN targets under those"""
    c = M.fit_inputs()
    vt, u = true_mesh().clone(), torch.ones(3, NV)
    if kind == "both":
        return c.target, c.weight, vt, u
    if kind == "verts":
        return None, None, vt, u
    if kind == "zerow":
        return c.target, torch.zeros(3, 21), vt, u
    assert kind == "third"
    off = torch.arange(NV) % 3 == 2
    u[:, off] = 0.0
    vt[:, off] = float("nan")
    return c.target, c.weight, vt, u


@functools.lru_cache(maxsize=None)
def mesh_pair(kind, start, iters):
    """(float64 reference, fp32 restatement) of the default mesh fit of mesh_targets(kind) from the named start of fit_inputs()"""
    t, w, vt, u = mesh_targets(kind)
    return tuple(fit_mesh_reference(dt, t, w, vt, u, M.fit_inputs().starts[start], iters) for dt in (torch.float64, torch.float32))


MESH_CASES = [(k, s, i) for k in ("both", "verts", "third") for s, i in (("zeros", 1), ("near", 1), ("zeros", 10), ("near", 10), ("zeros", 50))]


def mean_vertex_error(verts):
    """mean distance of the fitted vertices from the true mesh, mm, per hand"""
    return (verts.double() - true_mesh().double()).norm(dim=-1).mean(1)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the chain joints -> cloud, restated: fit, then rounds x (associate_host, fit_mesh_reference), then associate_host
# ----------------------------------------------------------------------------------------------------------------------------------------
CLOUD_START = "near"  # see fit_cloud_reference


def fit_cloud_reference(dtype, points, start, rounds, iters, iters_cloud, max_dist=20.0, lambda_verts=1.0):
    """fit_inputs()'s joints from the named start, then the cloud -> (cloud_before, cloud_after) stats [B, 2] and the last fit.

    Which start the "the cloud pulls the mesh in" test uses.  In float64, 50 iterations per fit, 3 rounds, gate 20 mm, the mean point-to-vertex distance goes
      from zeros   6.7 / 6.9 / 6.6 mm -> 6.2 / 6.1 / 6.0 mm   (8 rounds: 6.0 / 5.9 / 5.5; 200 iterations, gate 40 mm, lambda_verts 4: no better)
      from "near"  5.7 / 5.5 / 5.4 mm -> 1.5 / 1.0 / 1.6 mm   (6 rounds: 0.83 / 0.82 / 0.81, the 0.5 mm noise's own 0.8 mm)
    The synthetic hand's skin is random, with vertices 1.4 - 6 mm apart: 50 joint-only iterations from zeros leave the vertices 15 - 19 mm off, the nearest
    vertex of most points is then the wrong one, and the alternation settles in that assignment.  From the truth + 0.1 noise in pose and shape the joint fit
    leaves them about 5 mm off, the assignments are mostly right and the cloud pulls the mesh in by more than a factor of three.  So the test starts "near":
    a factor of less than two from zeros would let fp32 noise decide the comparison."""
    c = M.fit_inputs()
    out = fit_mesh_reference(dtype, c.target, c.weight, None, None, c.starts[start], iters)
    first = None
    for _ in range(rounds):
        a = associate_host(points.numpy(), None, out["verts"].float().numpy(), max_dist * max_dist)
        first = a if first is None else first
        state = (out["pose_aa"], out["betas"], out["trans"])
        out = fit_mesh_reference(dtype, c.target, c.weight, torch.from_numpy(a[1]), torch.from_numpy(a[2]), state, iters_cloud, lambda_verts=lambda_verts,
                                 init_trans=False)
    last = associate_host(points.numpy(), None, out["verts"].float().numpy(), max_dist * max_dist)
    return (last if first is None else first)[3], last[3], out
