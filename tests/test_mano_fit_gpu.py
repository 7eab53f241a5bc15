"""kpf_mano_fit_f32 / mano_fit.ManoFitter: the whole Adam fit of 21 joints in one launch, against the fit restated with oracle.aux_oracle.mano_layer and
torch.optim.Adam in float64 (tests/mano_cases.py::fit_reference).  Bound of every trajectory comparison: e_kernel <= 4 e_plain + 8 * 2^-24 max|ref|, e_plain
being the distance of the fp32 restatement from the float64 one.  CPU figures of e_plain at 50 steps from zeros, as orientation: joints 9e-5 mm, vertices
1.7e-4 mm, axis-angle 1.4e-6.  Measured on the MI355X: see DESIGN.md 4.11."""
import pytest
import torch

import mano_cases as M
from test_heads_gpu import _dev, rel_err

pytestmark = pytest.mark.gpu
STATE = ("mano_pose_aa", "mano_shape", "trans")


def _fitter(dev, iters, **kw):
    from keypointfusion_amd.mano_fit import ManoFitter
    return ManoFitter(M.model_sd(), dev, iters=iters, **kw)


def _state(dev, start):
    return tuple(s.clone().to(dev) for s in start)


def _fit(dev, iters, start="zeros", target=None, weight="case", init_trans=True, **kw):
    """one fit of fit_inputs() (or the given target / weight) -> ({name: cpu tensor}, the state tensors)"""
    c = M.fit_inputs()
    y = (c.target if target is None else target).to(dev).contiguous()
    w = c.weight if isinstance(weight, str) else weight
    st = _state(dev, c.starts[start])
    out = _fitter(dev, iters, **kw).fit(y, None if w is None else w.to(dev).contiguous(), state=st, init_trans=init_trans)
    return {k: v.detach().cpu().clone() for k, v in out.items()}, st


def _named(out):
    return {"pose_aa": out["mano_pose_aa"], "betas": out["mano_shape"], "trans": out["trans"], "joints": out["joints3d"], "verts": out["verts3d"]}


def _same(a, b, rows=None):
    for k in a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        assert torch.equal(x, y), k


@pytest.mark.parametrize("start", ["zeros", "near"])
@pytest.mark.parametrize("iters", [1, 10, 50])
def test_trajectory_matches_the_float64_fit(start, iters):
    dev = _dev()
    ref, plain = M.fit_pair(start, iters)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    out, _ = _fit(dev, iters, start)
    errs = M.fit_errors(_named(out), ref, plain)
    for k, (ek, ep, mx) in errs.items():
        print("MANO-FIT %-5s iters %2d %-8s e_kernel %.3e e_plain %.3e max|ref| %.3e%s" % (start, iters, k, ek, ep, mx, "" if M.within(ek, ep, mx) else " MISSES"))
    for k, (ek, ep, mx) in errs.items():
        assert M.within(ek, ep, mx), (k, ek, ep, mx)
    assert int(out["status"].abs().sum()) == 0
    # the residual: it falls, and it is the mean weighted joint distance of the returned joints
    c = M.fit_inputs()
    res = out["residual"].double()
    assert bool((res[:, 1] < res[:, 0]).all())
    host = (c.weight.double() * (out["joints3d"].double() - c.target.double()).norm(dim=-1)).sum(1) / c.weight.double().sum(1)
    assert bool(((res[:, 1] - host).abs() <= 1e-3 + 1e-5 * host).all()), (res[:, 1], host)
    assert bool(((res[:, 0] - ref["residual"][:, 0]).abs() <= 1e-3 + 1e-5 * ref["residual"][:, 0]).all())


def _forward_of_rotmat(dev, rotmat, betas):
    """kpf_mano_forward_f32 fed the 6D form (first two columns) of the rotations"""
    from keypointfusion_amd import lib as L
    from keypointfusion_amd.heads import mano_model_arrays
    B = rotmat.shape[0]
    six = torch.cat([rotmat[..., 0], rotmat[..., 1]], -1).reshape(B, 96).to(dev).contiguous()
    bt = betas.to(dev).contiguous()
    o = [torch.empty(B, 778, 3, device=dev), torch.empty(B, 21, 3, device=dev), torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 48, device=dev)]
    L.check(L.load().kpf_mano_forward_f32(six.data_ptr(), 96, bt.data_ptr(), 10, *[m.data_ptr() for m in mano_model_arrays(M.model_sd(), dev)],
                                          *[t.data_ptr() for t in o], B, torch.cuda.current_stream().cuda_stream), "kpf_mano_forward_f32")
    return o[0].cpu(), o[1].cpu()


@pytest.mark.parametrize("iters", [0, 10])
def test_outputs_are_the_forward_kernel_of_the_returned_state(iters):
    dev = _dev()
    c = M.fit_inputs()
    out, st = _fit(dev, iters, "near", init_trans=iters > 0)
    if iters == 0:  # only evaluates: the state keeps its bits
        for s, s0 in zip(st, c.starts["near"]):
            assert torch.equal(s.cpu(), s0)
        assert torch.equal(out["residual"][:, 0], out["residual"][:, 1])
    verts, joints = _forward_of_rotmat(dev, out["mano_pose"], out["mano_shape"])
    t = out["trans"][:, None]
    assert rel_err(out["verts3d"] - t, verts) < 1e-5 and rel_err(out["joints3d"] - t, joints) < 1e-5


def test_status_bits_leave_the_state_alone_and_the_neighbours_untouched():
    dev = _dev()
    c = M.fit_inputs()
    good, _ = _fit(dev, 10)
    # sample 1: all weights zero -> status 1; sample 2: a NaN target under a positive weight -> status 2; sample 0 is their neighbour
    w = c.weight.clone()
    w[1] = 0.0
    y = c.target.clone()
    y[2, 5, 1] = float("nan")
    out, st = _fit(dev, 10, target=y, weight=w)
    assert out["status"].tolist() == [0, 1, 2]
    for s, s0 in zip(st, c.starts["zeros"]):
        assert torch.equal(s.cpu()[1:], s0[1:])
    _same({k: good[k] for k in STATE + ("verts3d", "joints3d", "residual")}, out, rows=(0, 0))
    assert float(out["residual"][1].abs().max()) == 0.0 and bool(torch.isfinite(out["verts3d"][1:]).all())
    # a NaN target under weight 0 is selected out: the bits of the run without it
    y = c.target.clone()
    y[1, 4] = float("nan")  # fit_inputs gives this row weight 0
    y[1, 17, 2] = float("inf")
    out, _ = _fit(dev, 10, target=y)
    assert out["status"].tolist() == [0, 0, 0]
    _same(good, out)


def test_joint_map_and_default_weights():
    dev = _dev()
    c = M.fit_inputs()
    good, _ = _fit(dev, 10)
    perm = torch.randperm(21, generator=torch.Generator().manual_seed(5))
    assert perm.tolist() != list(range(21))
    out, _ = _fit(dev, 10, target=c.target[:, perm], weight=c.weight[:, perm], joint_map=perm.tolist())
    _same({k: good[k] for k in STATE + ("verts3d", "residual", "status")}, out)
    assert torch.equal(out["joints3d"], good["joints3d"][:, perm])
    ones, _ = _fit(dev, 10, weight=torch.ones(3, 21))
    none, _ = _fit(dev, 10, weight=None)
    _same(ones, none)


def test_fit_is_deterministic_and_independent_of_the_batch():
    dev = _dev()
    c = M.fit_inputs()
    a, _ = _fit(dev, 10)
    b, _ = _fit(dev, 10)
    _same(a, b)
    from keypointfusion_amd.mano_fit import ManoFitter
    for i in (0, 2):
        st = tuple(s[i:i + 1].clone().to(dev) for s in c.starts["zeros"])
        one = ManoFitter(M.model_sd(), dev, iters=10).fit(c.target[i:i + 1].to(dev).contiguous(), c.weight[i:i + 1].to(dev).contiguous(), state=st)
        _same({k: v.cpu() for k, v in one.items()}, a, rows=(0, i))


def test_warm_start_restarts_the_moments():
    dev = _dev()
    c = M.fit_inputs()
    fitter = _fitter(dev, 10)
    y, w = c.target.to(dev), c.weight.to(dev)
    st = _state(dev, c.starts["zeros"])
    fitter.fit(y, w, state=st)
    first = tuple(s.cpu().clone() for s in st)
    second = {k: v.cpu().clone() for k, v in fitter.fit(y, w, state=st, init_trans=False).items()}
    once, _ = _fit(dev, 20)
    assert not torch.equal(second["mano_pose_aa"], once["mano_pose_aa"])  # Adam's moments are zero at the start of every call
    ref, plain = [M.fit_reference(dt, c.target, c.weight, first, 10, init_trans=False) for dt in (torch.float64, torch.float32)]
    for k, (ek, ep, mx) in M.fit_errors(_named(second), ref, plain).items():
        print("MANO-FIT warm start %-8s e_kernel %.3e e_plain %.3e" % (k, ek, ep))
        assert M.within(ek, ep, mx), (k, ek, ep, mx)


def test_fit_replays_from_a_captured_graph():
    dev = _dev()
    c = M.fit_inputs()
    eager, _ = _fit(dev, 10)
    fitter = _fitter(dev, 10)
    y, w = c.target.to(dev), c.weight.to(dev)
    st = _state(dev, c.starts["zeros"])
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fitter.fit(y, w, state=st)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = fitter.fit(y, w, state=st)
    torch.cuda.current_stream(dev).wait_stream(side)
    for _ in range(2):
        for s, s0 in zip(st, c.starts["zeros"]):
            s.copy_(s0)
        graph.replay()
        torch.cuda.synchronize(dev)
        _same(eager, {k: v.cpu() for k, v in out.items()})
