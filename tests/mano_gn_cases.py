"""The damped Gauss-Newton joint fit (kpf_mano_fit_gn_f32) restated on the CPU: oracle.aux_oracle.mano_layer, torch.autograd.functional.jacobian
and torch.linalg.cholesky, in float64 (the reference) or float32 (the "plain" run whose distance from the reference sets the bound, mano_cases.within).  No GPU.

Per sample, p = (pose 0..47, betas 48..57, trans 58..60):
    r_i = sqrt(w_i / sw) (J_map[i](theta, beta) + t - y_i)        63 rows, mm; a row under weight 0 is selected out, never multiplied
    J = d r / d p,  Lambda = diag(0 x3, lambda_pose x45, lambda_shape x10, 0 x3)
    A = J^T J + Lambda + mu diag(J^T J) + nu I,  g = J^T r + Lambda p,  A delta = g by Cholesky,  p <- p - delta
The inputs are mano_cases.fit_inputs() (B = 3, two joints off on sample 1)."""
import functools

import torch

import mano_cases as M
from oracle import aux_oracle as A

GN_ITERS, GN_MU, GN_NU = 8, 0.1, 1e-2
ORDER = list(A.OBMAN2MANO)


def _joints(sd, p):
    """p [61] -> (verts [778, 3], joints [21, 3] in the head's order), mm, with the translation"""
    v, j = A.mano_layer(sd, p[None, :48], p[None, 48:58])
    return v[0] + p[58:61], j[0, ORDER] + p[58:61]


def entry_jacobian(dtype, start):
    """the unweighted d (J_i + t) / d p of every sample of `start` -> [B, 63, 61] in `dtype`"""
    sd = M._cast(M.model_sd(), dtype)
    P = torch.cat([s.to(dtype) for s in start], 1)
    return torch.stack([torch.autograd.functional.jacobian(lambda q: _joints(sd, q)[1].reshape(63), p) for p in P])


def gn_reference(dtype, target, weight, start, iters, mu=GN_MU, nu=GN_NU, lambda_shape=M.FIT_LAMBDA_SHAPE, lambda_pose=0.0, init_trans=True, jacobian=True):
    """-> dict(pose_aa, betas, trans, joints, verts, residual [B, 2], history [B, iters + 1], status [B], jacobian [B, 63, 61] or None), all in `dtype`.
    status: 1 the weights sum to 0, 2 a target under a positive weight is not finite (either: the state is left alone), 4 the Cholesky factorisation
    failed (the state holds the last completed iteration and the rest of history repeats its distance)."""
    sd = M._cast(M.model_sd(), dtype)
    B = target.shape[0]
    w = weight.to(dtype)
    y = torch.where(w[..., None] > 0, target.to(dtype), torch.zeros((), dtype=dtype))
    P = torch.cat([s.detach().clone().to(dtype) for s in start], 1)
    mu, nu, ls, lp = (torch.tensor(M._f32(v), dtype=dtype) for v in (mu, nu, lambda_shape, lambda_pose))  # the kernel's configuration holds float32 numbers
    lam = torch.cat([torch.zeros(3, dtype=dtype), lp.expand(45), ls.expand(10), torch.zeros(3, dtype=dtype)])
    out = {k: [] for k in ("pose_aa", "betas", "trans", "joints", "verts", "residual", "history", "status")}
    for b in range(B):
        p, wb, yb = P[b].clone(), w[b], y[b]
        on = wb > 0
        sw = wb.sum()
        st = (0 if bool(sw > 0) else 1) | (0 if bool(torch.isfinite(yb[on]).all()) else 2)
        n = iters if st == 0 else 0

        def distance(q):
            if not bool(sw > 0):
                return torch.zeros((), dtype=dtype)
            d = (_joints(sd, q)[1] - yb).norm(dim=-1)
            return (wb[on] * d[on]).sum() / sw

        def rows(q):
            sq = torch.sqrt(torch.where(on, wb, torch.ones_like(wb)) / sw)
            return torch.where(on[:, None], sq[:, None] * (_joints(sd, q)[1] - yb), torch.zeros((), dtype=dtype)).reshape(63)

        with torch.no_grad():
            if n > 0 and init_trans:
                j0 = _joints(sd, p)[1] - p[58:61]
                p[58:61] = (wb[on, None] * (yb[on] - j0[on])).sum(0) / sw
            hist = [distance(p)]
        for _ in range(n):
            J = torch.autograd.functional.jacobian(rows, p)
            with torch.no_grad():
                r = rows(p)
                N = J.t() @ J
                Amat = N + torch.diag(lam) + mu * torch.diag(torch.diagonal(N)) + nu * torch.eye(61, dtype=dtype)
                g = J.t() @ r + lam * p
                Lc, info = torch.linalg.cholesky_ex(Amat)
                if int(info) != 0 or not bool(torch.isfinite(Lc).all()):
                    st |= 4
                    break
                p = p - torch.cholesky_solve(g[:, None], Lc)[:, 0]
                hist.append(distance(p))
        with torch.no_grad():
            hist = hist + [hist[-1]] * (iters + 1 - len(hist))
            v, j = _joints(sd, p)
        for k, val in (("pose_aa", p[:48]), ("betas", p[48:58]), ("trans", p[58:61]), ("joints", j), ("verts", v), ("residual", torch.stack([hist[0], hist[-1]])),
                       ("history", torch.stack(hist)), ("status", torch.tensor(st))):
            out[k].append(val)
    out = {k: torch.stack(v) for k, v in out.items()}
    out["jacobian"] = entry_jacobian(dtype, start) if jacobian else None
    return out


@functools.lru_cache(maxsize=None)
def gn_pair(start, iters, mu=GN_MU, nu=GN_NU):
    """(float64 reference, fp32 restatement) of the default Gauss-Newton fit of fit_inputs() from the named start"""
    c = M.fit_inputs()
    return tuple(gn_reference(dt, c.target, c.weight, c.starts[start], iters, mu, nu, jacobian=False) for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def grad_states():
    """The B = 5 rotations of mano_cases.grad_case() as an axis-angle state (the head's own conversion, in float64, rounded to float32): every joint near 170
    degrees about an axis, or at 20, 95 or 3 degrees about an oblique one; its betas; no translation."""
    g = M.grad_case()
    aa = A.quat_to_aa(A.mat_to_quat(A.rot6d_to_mat(g.pose6d.double().reshape(-1, 6)))).reshape(-1, 48)
    return aa.float().contiguous(), g.betas.clone(), torch.zeros(g.betas.shape[0], 3)


@functools.lru_cache(maxsize=None)
def jacobian_pair(which):
    """(float64, fp32) entry Jacobians of the named set of states: "grad" (grad_states) or "zeros" (fit_inputs' cold start: an exact zero root rotation)"""
    start = grad_states() if which == "grad" else M.fit_inputs().starts["zeros"]
    return start, entry_jacobian(torch.float64, start), entry_jacobian(torch.float32, start)


def wrist_only():
    """fit_inputs' targets with weight on the wrist alone: the wrist does not move with any rotation, so all 48 pose columns of J are exactly zero"""
    c = M.fit_inputs()
    w = torch.zeros(3, 21)
    w[:, 0] = 1.0
    return c.target, w, c.starts["near"]


def gn_errors(got, ref, plain, keys=("pose_aa", "betas", "trans", "joints", "verts", "history")):
    """-> {name: (e_kernel, e_plain, max|ref|)}, absolute"""
    out = {}
    for k in keys:
        r = ref[k].double()
        out[k] = (float((got[k].detach().cpu().double() - r).abs().max()), float((plain[k].double() - r).abs().max()), float(r.abs().max()))
    return out
