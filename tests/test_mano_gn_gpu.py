"""kpf_mano_fit_gn_f32 / ManoFitter.fit_gn: the damped Gauss-Newton joint fit in one launch, against its float64 restatement (tests/mano_gn_cases.py:
oracle.aux_oracle.mano_layer, autograd's Jacobian, torch.linalg.cholesky).  Bound of every comparison with the reference: e_kernel <= 4 e_plain +
8 * 2^-24 max|ref| (mano_cases.within), e_plain being the distance of the fp32 restatement from the float64 one.  Measured on the MI355X: DESIGN.md 4.13."""
import pytest
import torch

import mano_cases as M
import mano_gn_cases as G
import mano_mesh_cases as MM
from test_heads_gpu import _dev

pytestmark = pytest.mark.gpu
STATE = ("mano_pose_aa", "mano_shape", "trans")
BITS = STATE + ("verts3d", "joints3d", "mano_pose", "residual", "status", "history")


def _fitter(dev, **kw):
    from keypointfusion_amd.mano_fit import ManoFitter
    return ManoFitter(M.model_sd(), dev, **kw)


def _state(dev, start):
    return tuple(s.clone().to(dev).contiguous() for s in start)


def _fit(dev, iters=None, start="zeros", target=None, weight="case", fitter_kw=None, **kw):
    """one fit_gn of fit_inputs() (or the given target / weight / start tensors) -> ({name: cpu tensor}, the state tensors)"""
    c = M.fit_inputs()
    y = (c.target if target is None else target).to(dev).contiguous()
    w = c.weight if isinstance(weight, str) else weight
    st = _state(dev, c.starts[start] if isinstance(start, str) else start)
    out = _fitter(dev, **(fitter_kw or {})).fit_gn(y, None if w is None else w.to(dev).contiguous(), state=st, iters=iters, **kw)
    return {k: v.detach().cpu().clone() for k, v in out.items()}, st


def _named(out):
    return {"pose_aa": out["mano_pose_aa"], "betas": out["mano_shape"], "trans": out["trans"], "joints": out["joints3d"], "verts": out["verts3d"],
            "history": out["history"]}


def _same(a, b, rows=None, keys=None):
    for k in keys or a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        assert torch.equal(x, y), k


@pytest.mark.parametrize("which", ["grad", "zeros"])
def test_entry_jacobian_matches_float64_autograd(which):
    """iters = 0 with jacobian=True: rotations near 170 degrees about each axis, at 20, 95 and 3 degrees (B = 5), and the cold start's exact zero rotations.
    The weights carry zeros: the output is unweighted, so those rows are reported like the others."""
    dev = _dev()
    start, ref, plain = G.jacobian_pair(which)
    B = start[0].shape[0]
    w = torch.ones(B, 21)
    w[0, 4] = w[B - 1, 17] = w[B - 1, 0] = 0.0
    out, st = _fit(dev, 0, start, target=torch.zeros(B, 21, 3), weight=w, jacobian=True)
    for s, s0 in zip(st, start):
        assert torch.equal(s.cpu(), s0)
    got = out["jacobian"].double()
    assert tuple(got.shape) == (B, 63, 61) and bool(torch.isfinite(got).all())
    mx = float(ref.abs().max())
    for name, cols in (("pose", slice(0, 48)), ("betas", slice(48, 58)), ("trans", slice(58, 61))):
        ek, ep = float((got[..., cols] - ref[..., cols]).abs().max()), float((plain[..., cols].double() - ref[..., cols]).abs().max())
        print("MANO-GN jacobian %-5s %-5s e_kernel %.3e e_plain %.3e max|ref| %.3e%s" % (which, name, ek, ep, mx, "" if M.within(ek, ep, mx) else " MISSES"))
    ek, ep = float((got - ref).abs().max()), float((plain.double() - ref).abs().max())
    assert M.within(ek, ep, mx), (ek, ep, mx)
    assert bool(got[0, 12:15].abs().max() > 0) and bool(got[B - 1, 0:3, 58:].abs().max() > 0)  # rows under weight 0


@pytest.mark.parametrize("start", ["zeros", "near"])
@pytest.mark.parametrize("iters", [1, 3, 8])
def test_fit_matches_the_float64_iteration(start, iters):
    dev = _dev()
    ref, plain = G.gn_pair(start, iters)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values() if v is not None) and ref["status"].tolist() == [0, 0, 0]
    out, _ = _fit(dev, iters, start)
    assert out["status"].tolist() == [0, 0, 0] and tuple(out["history"].shape) == (3, iters + 1)
    errs = G.gn_errors(_named(out), ref, plain)
    for k, (ek, ep, mx) in errs.items():
        print("MANO-GN %-5s iters %d %-8s e_kernel %.3e e_plain %.3e max|ref| %.3e%s" % (start, iters, k, ek, ep, mx, "" if M.within(ek, ep, mx) else " MISSES"))
    for k, (ek, ep, mx) in errs.items():
        assert M.within(ek, ep, mx), (k, ek, ep, mx)
    # the history's ends are the residual, and it is the mean weighted joint distance of the returned joints
    assert torch.equal(out["history"][:, 0], out["residual"][:, 0]) and torch.equal(out["history"][:, -1], out["residual"][:, 1])
    c = M.fit_inputs()
    host = (c.weight.double() * (out["joints3d"].double() - c.target.double()).norm(dim=-1)).sum(1) / c.weight.double().sum(1)
    assert bool(((out["residual"][:, 1].double() - host).abs() <= 1e-3 + 1e-5 * host).all())


def test_iters_zero_only_evaluates_with_the_adam_entrys_bits():
    dev = _dev()
    c = M.fit_inputs()
    out, st = _fit(dev, 0, "near")
    for s, s0 in zip(st, c.starts["near"]):
        assert torch.equal(s.cpu(), s0)
    adam = _fitter(dev, iters=0).fit(c.target.to(dev), c.weight.to(dev), state=_state(dev, c.starts["near"]))
    for k in ("verts3d", "joints3d", "mano_pose", "residual", "status"):
        assert torch.equal(out[k], adam[k].cpu()), k
    assert tuple(out["history"].shape) == (3, 1) and torch.equal(out["history"][:, 0], out["residual"][:, 0])
    assert torch.equal(out["residual"][:, 0], out["residual"][:, 1])


def test_unobservable_columns_take_an_exact_zero_step():
    """weight on the wrist only, lambda_pose = 0: all 48 pose columns of J are zero; with nu > 0 the matrix stays positive definite and the pose does not move"""
    dev = _dev()
    t, w, start = G.wrist_only()
    ref, plain = [G.gn_reference(dt, t, w, start, G.GN_ITERS, jacobian=False) for dt in (torch.float64, torch.float32)]
    out, _ = _fit(dev, None, start, target=t, weight=w)
    assert out["status"].tolist() == [0, 0, 0]
    assert torch.equal(out["mano_pose_aa"], start[0])
    assert not torch.equal(out["mano_shape"], start[1])
    for k, (ek, ep, mx) in G.gn_errors(_named(out), ref, plain, keys=("betas", "trans")).items():
        print("MANO-GN wrist only %-8s e_kernel %.3e e_plain %.3e max|ref| %.3e" % (k, ek, ep, mx))
        assert M.within(ek, ep, mx), (k, ek, ep, mx)


def test_singular_matrix_sets_bit_4_and_leaves_the_state():
    dev = _dev()
    c = M.fit_inputs()
    t, w, start = G.wrist_only()
    w = w.clone()
    w[1] = c.weight[1]  # sample 1 keeps the weights of fit_inputs: the neighbour
    out, st = _fit(dev, None, start, target=t, weight=w, fitter_kw=dict(lambda_shape=0.0), mu=0.0, nu=0.0)
    # with mu = nu = lambda_shape = 0 the neighbour's 57 rows leave J^T J singular as well (the float64 restatement stops there too:
    # test_mano_gn_host.py::test_reference_status_and_jacobian_conventions), so all three stop
    assert out["status"].tolist() == [4, 4, 4]
    assert torch.equal(out["mano_pose_aa"], start[0]) and torch.equal(out["mano_shape"], start[1])
    assert not torch.equal(out["trans"], start[2])  # init_trans ran before iteration 1
    for k in ("verts3d", "joints3d", "mano_pose", "residual", "history"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert torch.equal(out["history"], out["residual"][:, :1].expand(3, G.GN_ITERS + 1))
    # a good sample beside singular ones, bit-equal to a launch without them.  The configuration is one per launch, so the neighbour needs one under which
    # it can be solved: Marquardt's mu alone (nu = lambda_shape = 0) -- the wrist-only samples' zero pose columns keep a zero pivot under any mu
    mixed, _ = _fit(dev, None, start, target=t, weight=w, fitter_kw=dict(lambda_shape=0.0), mu=0.1, nu=0.0)
    alone, _ = _fit(dev, None, tuple(s[1:2] for s in start), target=t[1:2], weight=w[1:2], fitter_kw=dict(lambda_shape=0.0), mu=0.1, nu=0.0)
    assert mixed["status"].tolist() == [4, 0, 4] and alone["status"].tolist() == [0]
    _same(alone, mixed, rows=(0, 1), keys=BITS)


def test_status_bits_1_and_2_leave_the_state_alone_and_the_neighbours_untouched():
    dev = _dev()
    c = M.fit_inputs()
    good, _ = _fit(dev)
    w = c.weight.clone()
    w[1] = 0.0
    y = c.target.clone()
    y[2, 5, 1] = float("nan")
    out, st = _fit(dev, target=y, weight=w)
    assert out["status"].tolist() == [0, 1, 2]
    for s, s0 in zip(st, c.starts["zeros"]):
        assert torch.equal(s.cpu()[1:], s0[1:])
    _same(good, out, rows=(0, 0), keys=BITS)
    assert float(out["residual"][1].abs().max()) == 0.0 and float(out["history"][1].abs().max()) == 0.0 and bool(torch.isfinite(out["verts3d"][1:]).all())
    # a NaN target under weight 0 is selected out: the bits of the run without it
    y = c.target.clone()
    y[1, 4] = float("nan")  # fit_inputs gives this row weight 0
    y[1, 17, 2] = float("inf")
    out, _ = _fit(dev, target=y)
    assert out["status"].tolist() == [0, 0, 0]
    _same(good, out, keys=BITS)


def test_joint_map_default_weights_batch_and_repeat_keep_the_bits():
    dev = _dev()
    c = M.fit_inputs()
    good, _ = _fit(dev)
    again, _ = _fit(dev)
    _same(good, again, keys=BITS)
    perm = torch.randperm(21, generator=torch.Generator().manual_seed(5))
    assert perm.tolist() != list(range(21))
    out, _ = _fit(dev, target=c.target[:, perm], weight=c.weight[:, perm], fitter_kw=dict(joint_map=perm.tolist()))
    _same(good, out, keys=STATE + ("verts3d", "mano_pose", "residual", "status", "history"))
    assert torch.equal(out["joints3d"], good["joints3d"][:, perm])
    ones, _ = _fit(dev, weight=torch.ones(3, 21))
    none, _ = _fit(dev, weight=None)
    _same(ones, none, keys=BITS)
    for i in (0, 2):
        one, _ = _fit(dev, None, tuple(s[i:i + 1] for s in c.starts["zeros"]), target=c.target[i:i + 1], weight=c.weight[i:i + 1])
        _same(one, good, rows=(0, i), keys=BITS)


def test_fit_gn_replays_from_a_captured_graph():
    dev = _dev()
    c = M.fit_inputs()
    eager, _ = _fit(dev)
    fitter = _fitter(dev)
    y, w = c.target.to(dev), c.weight.to(dev)
    st = _state(dev, c.starts["zeros"])
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fitter.fit_gn(y, w, state=st)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = fitter.fit_gn(y, w, state=st)
    torch.cuda.current_stream(dev).wait_stream(side)
    for _ in range(2):
        for s, s0 in zip(st, c.starts["zeros"]):
            s.copy_(s0)
        graph.replay()
        torch.cuda.synchronize(dev)
        _same(eager, {k: v.cpu() for k, v in out.items()}, keys=BITS)


def _cloud_inputs(dev):
    c = M.fit_inputs()
    return c.target.to(dev).contiguous(), c.weight.to(dev).contiguous(), MM.cloud().to(dev).contiguous()


def test_fit_cloud_default_solver_keeps_its_bits():
    dev = _dev()
    c = M.fit_inputs()
    y, w, pts = _cloud_inputs(dev)
    outs = []
    for kw in ({}, {"joint_solver": "adam"}):
        out = _fitter(dev, iters=5).fit_cloud(y, pts, w, state=_state(dev, c.starts["near"]), rounds=1, **kw)
        outs.append({k: v.detach().cpu().clone() for k, v in out.items()})
    assert set(outs[0]) == set(outs[1])
    _same(outs[0], outs[1])
    with pytest.raises(ValueError):
        _fitter(dev, iters=5).fit_cloud(y, pts, w, joint_solver="newton")


def test_fit_cloud_with_gn_is_the_composition_by_hand():
    dev = _dev()
    c = M.fit_inputs()
    y, w, pts = _cloud_inputs(dev)
    out = _fitter(dev, iters=5).fit_cloud(y, pts, w, state=_state(dev, c.starts["near"]), rounds=1, joint_solver="gn")
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    f = _fitter(dev, iters=5)
    st = _state(dev, c.starts["near"])
    first = f.fit_gn(y, w, state=st)
    a0 = {k: v.clone() for k, v in f.associate(pts, first["verts3d"]).items()}
    mesh = f.fit_mesh(y, w, a0["vert_target"], a0["vert_weight"], state=st, init_trans=False)
    a1 = f.associate(pts, mesh["verts3d"])
    for k in STATE + ("verts3d", "joints3d", "mano_pose", "residual", "status"):
        assert torch.equal(out[k], mesh[k].cpu()), k
    assert torch.equal(out["cloud_before"], a0["stats"].cpu()) and torch.equal(out["cloud_after"], a1["stats"].cpu())
    for k in ("idx", "vert_target", "vert_weight"):
        assert torch.equal(out[k], a1[k].cpu()), k
    # and the first stage did its work: the joints start the cloud rounds closer than the Adam stage's 5 iterations leave them
    adam = _fitter(dev, iters=5).fit(y, w, state=_state(dev, c.starts["near"]))
    assert bool((first["residual"][:, 1] < adam["residual"][:, 1]).all())
