"""The damped Gauss-Newton mesh fit (kpf_mano_fit_mesh_gn_f32) restated on the CPU in the manner of mano_gn_cases.gn_reference, with the
vertex rows: oracle.aux_oracle.mano_layer, forward-mode torch.autograd.functional.jacobian and torch.linalg.cholesky_ex, in float64 (the reference) or
float32 (the "plain" run whose distance from the reference sets the bound, mano_cases.within).  No GPU.

Per sample, p = (pose 0..47, betas 48..57, trans 58..60):
    63 joint rows    sqrt(w_i / sw) (J_map[i] + t - y_i)                   mm; a row under weight 0 is selected out, never multiplied
    2334 vertex rows sqrt(lambda_verts u_v / sv) (V_v + t - c_v)           a term whose weights sum to 0 contributes nothing
    N = J^T J,  A = N + Lambda + mu diag(N) + nu I,  g = J^T r + Lambda p,  A delta = g by Cholesky,  p <- p - delta
The inputs are mano_cases.fit_inputs() (B = 3) with mano_mesh_cases.mesh_targets(kind).  A run of n iterations passes through the states of every
shorter run, so one 8-iteration trajectory per (kind, start, dtype) serves the cases of 1, 3 and 8 iterations."""
import functools

import torch

import mano_cases as M
import mano_gn_cases as G
import mano_mesh_cases as MM

NV = MM.NV
MESH_GN_ITERS = 8
MESH_GN_CASES = [(k, s, i) for k in ("both", "verts", "third") for s in ("zeros", "near") for i in (1, 3, 8)]


def _trajectory(dtype, target, weight, vert_target, vert_weight, start, iters, mu, nu, lambda_shape, lambda_pose, lambda_verts, init_trans):
    """-> (sd, w, y, u, c, status [B], states: per sample the list of p before iteration 1 and after each completed iteration, failed [B])"""
    sd = M._cast(M.model_sd(), dtype)
    B = start[0].shape[0]
    zero = torch.zeros((), dtype=dtype)
    w = torch.zeros(B, 21, dtype=dtype) if target is None else (torch.ones(B, 21, dtype=dtype) if weight is None else weight.to(dtype))
    y = torch.zeros(B, 21, 3, dtype=dtype) if target is None else torch.where(w[..., None] > 0, target.to(dtype), zero)
    has_v = vert_weight is not None
    u = vert_weight.to(dtype) if has_v else torch.zeros(B, NV, dtype=dtype)
    c = torch.where(u[..., None] > 0, vert_target.to(dtype), zero) if has_v else torch.zeros(B, NV, 3, dtype=dtype)
    P = torch.cat([s.detach().clone().to(dtype) for s in start], 1)
    mu, nu, ls, lp, lv = (torch.tensor(M._f32(v), dtype=dtype) for v in (mu, nu, lambda_shape, lambda_pose, lambda_verts))  # the configuration holds float32
    lam = torch.cat([torch.zeros(3, dtype=dtype), lp.expand(45), ls.expand(10), torch.zeros(3, dtype=dtype)])
    status, states, failed = [], [], []
    for b in range(B):
        p, wb, yb, ub, cb = P[b].clone(), w[b], y[b], u[b], c[b]
        on, von = wb > 0, ub > 0
        sw, sv = wb.sum(), ub.sum()
        jw, vw = bool(sw > 0), bool(sv > 0)
        st = (0 if (jw or vw) else 1) | (0 if bool(torch.isfinite(yb[on]).all()) and bool(torch.isfinite(cb[von]).all()) else 2)
        n = iters if st == 0 else 0

        def rows(q):
            v, j = G._joints(sd, q)
            out = []
            if jw:  # gn_reference's expression
                sq = torch.sqrt(torch.where(on, wb, torch.ones_like(wb)) / sw)
                out.append(torch.where(on[:, None], sq[:, None] * (j - yb), zero).reshape(63))
            else:
                out.append(torch.zeros(63, dtype=dtype) + 0 * q[0])
            if has_v:
                if vw:
                    sq = torch.sqrt(lv * torch.where(von, ub, torch.ones_like(ub)) / sv)
                    out.append(torch.where(von[:, None], sq[:, None] * (v - cb), zero).reshape(NV * 3))
                else:
                    out.append(torch.zeros(NV * 3, dtype=dtype) + 0 * q[0])
            return torch.cat(out)

        with torch.no_grad():
            if n > 0 and init_trans:
                v0, j0 = G._joints(sd, p)
                if jw:
                    p[58:61] = (wb[on, None] * (yb[on] - (j0 - p[58:61])[on])).sum(0) / sw
                else:
                    p[58:61] = (ub[von, None] * (cb[von] - (v0 - p[58:61])[von])).sum(0) / sv
        traj, fail = [p.clone()], False
        for _ in range(n):
            if has_v:
                J = torch.autograd.functional.jacobian(rows, p, vectorize=True, strategy="forward-mode")
            else:
                J = torch.autograd.functional.jacobian(rows, p)  # 63 rows: gn_reference's call, and its bits
            with torch.no_grad():
                r = rows(p)
                N = J.t() @ J
                Amat = N + torch.diag(lam) + mu * torch.diag(torch.diagonal(N)) + nu * torch.eye(61, dtype=dtype)
                g = J.t() @ r + lam * p
                Lc, info = torch.linalg.cholesky_ex(Amat)
                if int(info) != 0 or not bool(torch.isfinite(Lc).all()):
                    fail = True
                    break
                p = p - torch.cholesky_solve(g[:, None], Lc)[:, 0]
                traj.append(p.clone())
        status.append(st)
        states.append(traj)
        failed.append(fail)
    return sd, w, y, u, c, status, states, failed


def _at(run, iters, dtype):
    """the outputs of the run stopped after `iters` iterations"""
    sd, w, y, u, c, status, states, failed = run
    zero = torch.zeros((), dtype=dtype)
    out = {k: [] for k in ("pose_aa", "betas", "trans", "joints", "verts", "residual", "history", "status")}
    for b, traj in enumerate(states):
        on, von = w[b] > 0, u[b] > 0
        sw, sv = w[b].sum(), u[b].sum()
        n = iters if status[b] == 0 else 0
        seen = traj[:n + 1]
        st = status[b] | (4 if failed[b] and len(traj) < n + 1 else 0)
        with torch.no_grad():
            hist = []
            for q in seen:
                v, j = G._joints(sd, q)
                dj = (w[b][on] * (j - y[b]).norm(dim=-1)[on]).sum() / sw if bool(sw > 0) else zero
                dv = (u[b][von] * (v - c[b]).norm(dim=-1)[von]).sum() / sv if bool(sv > 0) else zero
                hist.append(torch.stack([dj, dv]))
            hist = hist + [hist[-1]] * (iters + 1 - len(hist))
            p = seen[-1]
            v, j = G._joints(sd, p)
        for k, val in (("pose_aa", p[:48]), ("betas", p[48:58]), ("trans", p[58:61]), ("joints", j), ("verts", v),
                       ("residual", torch.stack([hist[0][0], hist[-1][0], hist[0][1], hist[-1][1]])), ("history", torch.stack(hist)),
                       ("status", torch.tensor(st))):
            out[k].append(val)
    return {k: torch.stack(v) for k, v in out.items()}


def mesh_gn_reference(dtype, target, weight, vert_target, vert_weight, start, iters, mu=G.GN_MU, nu=G.GN_NU, lambda_shape=M.FIT_LAMBDA_SHAPE,
                      lambda_pose=0.0, lambda_verts=1.0, init_trans=True):
    """-> dict(pose_aa, betas, trans, joints, verts, residual [B, 4], history [B, iters + 1, 2], status [B]) in `dtype`.  target=None: no joint carries
    weight.  vert_weight=None: no vertex term, and pose_aa, betas, trans, joints, verts, status, residual[:, :2] and history[..., 0] are gn_reference's,
    tensor for tensor.  status: 1 both weight sums are 0, 2 a joint or vertex target under a positive weight is not finite (either: the state is left
    alone), 4 the factorisation failed (the state holds the last completed iteration, the history repeats)."""
    run = _trajectory(dtype, target, weight, vert_target, vert_weight, start, iters, mu, nu, lambda_shape, lambda_pose, lambda_verts, init_trans)
    return _at(run, iters, dtype)


@functools.lru_cache(maxsize=None)
def _case_run(kind, start, dtype):
    t, w, vt, u = MM.mesh_targets(kind)
    return _trajectory(dtype, t, w, vt, u, M.fit_inputs().starts[start], MESH_GN_ITERS, G.GN_MU, G.GN_NU, M.FIT_LAMBDA_SHAPE, 0.0, 1.0, True)


@functools.lru_cache(maxsize=None)
def mesh_gn_pair(kind, start, iters):
    """(float64 reference, fp32 restatement) of the default Gauss-Newton mesh fit of mesh_targets(kind) from the named start of fit_inputs(), iters <= 8"""
    assert 0 <= iters <= MESH_GN_ITERS
    if iters == 0:  # only evaluates: no init_trans, so not the head of a longer run
        t, w, vt, u = MM.mesh_targets(kind)
        return tuple(mesh_gn_reference(dt, t, w, vt, u, M.fit_inputs().starts[start], 0) for dt in (torch.float64, torch.float32))
    return tuple(_at(_case_run(kind, start, dt), iters, dt) for dt in (torch.float64, torch.float32))


def entry_vertex_jacobian(dtype, start):
    """the unweighted d (V_v + t) / d p of every sample of `start` -> [B, 2334, 61] in `dtype`, row v * 3 + d"""
    sd = M._cast(M.model_sd(), dtype)
    P = torch.cat([s.to(dtype) for s in start], 1)
    return torch.stack([torch.autograd.functional.jacobian(lambda q: G._joints(sd, q)[0].reshape(NV * 3), p, vectorize=True, strategy="forward-mode")
                        for p in P])


@functools.lru_cache(maxsize=None)
def vertex_jacobian_pair(which):
    """(start, float64, fp32) entry vertex Jacobians of mano_gn_cases.grad_states() ("grad") or of the cold start ("zeros")"""
    start = G.grad_states() if which == "grad" else M.fit_inputs().starts["zeros"]
    return start, entry_vertex_jacobian(torch.float64, start), entry_vertex_jacobian(torch.float32, start)


def mesh_gn_errors(got, ref, plain, keys=("pose_aa", "betas", "trans", "joints", "verts", "history", "residual")):
    """-> {name: (e_kernel, e_plain, max|ref|)}, absolute"""
    return G.gn_errors(got, ref, plain, keys)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the chain joints -> cloud with Gauss-Newton rounds: the Adam joint fit, then rounds x (associate_host, mesh_gn_reference), then associate_host
# ----------------------------------------------------------------------------------------------------------------------------------------
def fit_cloud_gn_reference(dtype, points, start, rounds, iters, iters_cloud, max_dist=20.0, lambda_verts=1.0):
    """mano_mesh_cases.fit_cloud_reference with mesh_gn_reference for the rounds -> (cloud_before, cloud_after) stats [B, 2] and the last fit"""
    c = M.fit_inputs()
    out = MM.fit_mesh_reference(dtype, c.target, c.weight, None, None, c.starts[start], iters)
    first = None
    for _ in range(rounds):
        a = MM.associate_host(points.numpy(), None, out["verts"].float().numpy(), max_dist * max_dist)
        first = a if first is None else first
        state = (out["pose_aa"], out["betas"], out["trans"])
        out = mesh_gn_reference(dtype, c.target, c.weight, torch.from_numpy(a[1]), torch.from_numpy(a[2]), state, iters_cloud, lambda_verts=lambda_verts,
                                init_trans=False)
    last = MM.associate_host(points.numpy(), None, out["verts"].float().numpy(), max_dist * max_dist)
    return (last if first is None else first)[3], last[3], out
