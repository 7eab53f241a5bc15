"""kpf_mano_fit_mesh_gn_plane_f32 / ManoFitter.fit_mesh_gn(vert_normal=...) / fit_cloud(metric="plane"): the Gauss-Newton mesh fit with one point-to-plane
row per vertex, against its float64 restatement (tests/mano_surface_cases.py::fit_mesh_gn_plane_reference).  Bound of every comparison with the reference:
e_kernel <= 4 e_plain + 8 * 2^-24 max|ref| (mano_cases.within), e_plain being the distance of the fp32 restatement from the float64 one.  B = 3, the inputs of
mano_cases.fit_inputs() with mano_mesh_cases.mesh_targets and the normals of mano_surface_cases.plane_normals.  Measured on the MI355X: DESIGN.md 4.15."""
import pytest
import torch

import mano_cases as M
import mano_gn_cases as G
import mano_mesh_cases as MM
import mano_mesh_gn_cases as MG
import mano_surface_cases as S
from test_heads_gpu import _dev

pytestmark = pytest.mark.gpu
STATE = ("mano_pose_aa", "mano_shape", "trans")
BITS = STATE + ("verts3d", "joints3d", "mano_pose", "residual", "status", "history")


def _fitter(dev, sd=None, **kw):
    from keypointfusion_amd.mano_fit import ManoFitter
    return ManoFitter(M.model_sd() if sd is None else sd, dev, **kw)


def _d(dev, t):
    return None if t is None else t.to(dev).contiguous()


def _cpu(out):
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _state(dev, start):
    return tuple(s.clone().to(dev).contiguous() for s in start)


def _fit(dev, iters, start="near", kind="both", normals="start", rows=slice(None), targets=None, **kw):
    """one fit_mesh_gn of mesh_targets(kind) from the named start with the given normals ("start": plane_normals(start); None: none)"""
    t, w, vt, u = MM.mesh_targets(kind) if targets is None else targets
    nm = S.plane_normals(start) if isinstance(normals, str) else normals
    st = _state(dev, [s[rows] for s in M.fit_inputs().starts[start]])
    cut = lambda x: None if x is None else _d(dev, x[rows])  # noqa: E731
    out = _fitter(dev).fit_mesh_gn(cut(t), cut(w), cut(vt), cut(u), state=st, iters=iters, vert_normal=cut(nm), **kw)
    return _cpu(out), st


def _named(out):
    return {"pose_aa": out["mano_pose_aa"], "betas": out["mano_shape"], "trans": out["trans"], "joints": out["joints3d"], "verts": out["verts3d"],
            "history": out["history"], "residual": out["residual"]}


def _same(a, b, rows=None, keys=None):
    for k in keys or a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        assert torch.equal(x, y), k


def _held(tag, errs):
    for k, (ek, ep, mx) in errs.items():
        print("MANO-PLANE-GN %s %-8s e_kernel %.3e e_plain %.3e ratio %6.2f max|ref| %.3e%s" % (
            tag, k, ek, ep, ek / ep if ep else float("inf") if ek else 0.0, mx, "" if M.within(ek, ep, mx) else " MISSES"))
    for k, (ek, ep, mx) in errs.items():
        assert M.within(ek, ep, mx), (tag, k, ek, ep, mx)


@pytest.mark.parametrize("kind,start,iters", S.PLANE_CASES)
def test_plane_fit_matches_the_float64_iteration(kind, start, iters):
    """joints and vertices together; vertices only (the entry gets target = NULL).  The normals are the start mesh's by the synthetic hand's random faces, a
    fifth of them zero: directions with no meaning, which is all the arithmetic needs."""
    dev = _dev()
    ref, plain = S.plane_pair(kind, start, iters)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values()) and ref["status"].tolist() == [0, 0, 0]
    out, _ = _fit(dev, iters, start, kind)
    assert out["status"].tolist() == [0, 0, 0] and tuple(out["history"].shape) == (3, iters + 1, 2) and tuple(out["residual"].shape) == (3, 4)
    _held("%-5s %-5s iters %d" % (kind, start, iters), MG.mesh_gn_errors(_named(out), ref, plain))
    h, res = out["history"], out["residual"]
    assert torch.equal(h[:, 0, 0], res[:, 0]) and torch.equal(h[:, -1, 0], res[:, 1]) and torch.equal(h[:, 0, 1], res[:, 2]) and torch.equal(h[:, -1, 1], res[:, 3])


def test_without_normals_the_bits_are_fit_mesh_gns():
    """vert_normal=None through the wrapper is today's call; the plane entry itself with a null vert_normal launches the same kernel"""
    dev = _dev()
    from keypointfusion_amd import lib as L
    c = M.fit_inputs()
    t, w, vt, u = (_d(dev, x) for x in MM.mesh_targets("both"))
    f = _fitter(dev)
    old = _cpu(f.fit_mesh_gn(t, w, vt, u, state=_state(dev, c.starts["near"]), iters=3))
    none, _ = _fit(dev, 3, "near", normals=None)
    _same(old, none, keys=BITS)
    st = _state(dev, c.starts["near"])
    o = f._mesh_gn_bufs[3]
    hist = o["history"][3]
    cfg = f.mesh_gn_cfg
    cfg.iters, cfg.init_trans = 3, 1
    for buf in (o["verts3d"], o["joints3d"], o["residual"], hist):
        buf.zero_()
    L.check(L.load().kpf_mano_fit_mesh_gn_plane_f32(t.data_ptr(), w.data_ptr(), vt.data_ptr(), u.data_ptr(), None, *[m.data_ptr() for m in f.model],
                                                    L.C.byref(cfg), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), o["verts3d"].data_ptr(),
                                                    o["joints3d"].data_ptr(), o["mano_pose"].data_ptr(), o["residual"].data_ptr(), o["status"].data_ptr(),
                                                    hist.data_ptr(), None, None, 3, torch.cuda.current_stream().cuda_stream), "plane entry, no normals")
    torch.cuda.synchronize(dev)
    raw = {"mano_pose_aa": st[0], "mano_shape": st[1], "trans": st[2], "verts3d": o["verts3d"], "joints3d": o["joints3d"], "mano_pose": o["mano_pose"],
           "residual": o["residual"], "status": o["status"], "history": hist}
    _same(old, _cpu(raw), keys=BITS)


def test_iters_zero_keeps_the_state_and_reports_the_plane_distance():
    dev = _dev()
    c = M.fit_inputs()
    ref, plain = S.plane_pair("both", "near", 0)
    out, st = _fit(dev, 0, "near")
    for s, s0 in zip(st, c.starts["near"]):
        assert torch.equal(s.cpu(), s0)
    assert out["status"].tolist() == [0, 0, 0] and tuple(out["history"].shape) == (3, 1, 2)
    _held("iters 0", MG.mesh_gn_errors(_named(out), ref, plain, keys=("joints", "verts", "history", "residual")))
    point, _ = _fit(dev, 0, "near", normals=None)
    assert bool((out["residual"][:, 2] < point["residual"][:, 2]).all()) and torch.equal(out["residual"][:, :2], point["residual"][:, :2])
    _same(out, point, keys=("verts3d", "joints3d", "mano_pose"))


def test_a_nan_normal_under_weight_sets_status_2_and_leaves_the_neighbours():
    dev = _dev()
    c = M.fit_inputs()
    good, _ = _fit(dev, 3, "near")
    n = S.plane_normals("near").clone()
    n[1, 301, 2] = float("nan")
    out, st = _fit(dev, 3, "near", normals=n)
    assert out["status"].tolist() == [0, 2, 0]
    for s, s0 in zip(st, c.starts["near"]):
        assert torch.equal(s.cpu()[1], s0[1])
    _same(good, out, rows=(0, 0), keys=BITS)
    _same(good, out, rows=(2, 2), keys=BITS)
    assert bool(torch.isfinite(out["verts3d"]).all()) and bool(torch.isfinite(out["joints3d"]).all())
    # under weight 0 a NaN or inf normal changes no bit
    t, w, vt, u = MM.mesh_targets("both")
    u = u.clone()
    u[:, 301] = 0.0
    n2 = S.plane_normals("near").clone()
    a, _ = _fit(dev, 3, "near", normals=n2, targets=(t, w, vt, u))
    n2[:, 301] = float("inf")
    n2[1, 301, 0] = float("nan")
    b, _ = _fit(dev, 3, "near", normals=n2, targets=(t, w, vt, u))
    assert b["status"].tolist() == [0, 0, 0]
    _same(a, b, keys=BITS)


def test_zero_normals_everywhere_leave_the_joint_fit():
    """every vertex row is zero (and still counts in sv): the state follows the joint-only Gauss-Newton fit of the float64 reference within the bound"""
    dev = _dev()
    ref, plain = G.gn_pair("near", 3)
    out, _ = _fit(dev, 3, "near", normals=torch.zeros(3, MM.NV, 3))
    assert out["status"].tolist() == [0, 0, 0] and not bool(out["history"][..., 1].any())
    _held("zero normals", G.gn_errors(_named(out), ref, plain, keys=("pose_aa", "betas", "trans", "joints", "verts")))


def test_rows_do_not_depend_on_the_batch_and_a_repeat_keeps_the_bits():
    dev = _dev()
    good, _ = _fit(dev, 3, "zeros", "verts")
    again, _ = _fit(dev, 3, "zeros", "verts")
    _same(good, again, keys=BITS)
    for i in (0, 2):
        one, _ = _fit(dev, 3, "zeros", "verts", rows=slice(i, i + 1))
        _same(one, good, rows=(0, i), keys=BITS)


def _cloud_inputs(dev):
    c = S.surface_inputs()
    return c.target.to(dev).contiguous(), c.weight.to(dev).contiguous(), S.surface_cloud().to(dev).contiguous()


def _by_hand(f, y, w, pts, st, rounds, facing_min=0.0):
    """fit_cloud(metric="plane", cloud_solver="gn") composed from the three entries"""
    fit = f.fit(y, w, state=st)
    first = None
    for _ in range(rounds):
        nrm = f.normals(fit["verts3d"]).clone()
        a = {k: v.clone() for k, v in f.associate(pts, fit["verts3d"], normals=nrm, facing_min=facing_min).items()}
        first = a if first is None else first
        fit = f.fit_mesh_gn(y, w, a["vert_target"], a["vert_weight"], state=st, init_trans=False, iters=2, vert_normal=nrm)
    nrm = f.normals(fit["verts3d"]).clone()
    last = {k: v.clone() for k, v in f.associate(pts, fit["verts3d"], normals=nrm, facing_min=facing_min).items()}
    return fit, (last if first is None else first), last, nrm


@pytest.mark.parametrize("rounds", [2, 0])
def test_fit_cloud_plane_is_the_composition_by_hand(rounds):
    dev = _dev()
    c = S.surface_inputs()
    y, w, pts = _cloud_inputs(dev)
    out = _cpu(_fitter(dev, S.surface_sd(), iters=5).fit_cloud(y, pts, w, state=_state(dev, c.near), rounds=rounds, cloud_solver="gn", metric="plane",
                                                              facing_min=0.25))
    fit, first, last, nrm = _by_hand(_fitter(dev, S.surface_sd(), iters=5), y, w, pts, _state(dev, c.near), rounds, 0.25)
    keys = STATE + ("verts3d", "joints3d", "mano_pose", "residual", "status") + (("history",) if rounds else ())
    for k in keys:
        assert torch.equal(out[k], fit[k].cpu()), k
    assert tuple(out["cloud_before"].shape) == (3, 4) and tuple(out["cloud_after"].shape) == (3, 4)
    assert torch.equal(out["cloud_before"], first["stats"].cpu()) and torch.equal(out["cloud_after"], last["stats"].cpu())
    for k in ("idx", "vert_target", "vert_weight", "visible"):
        assert torch.equal(out[k], last[k].cpu()), k
    assert torch.equal(out["normals"], nrm.cpu())
    assert out["status"].tolist() == [0, 0, 0] and bool((out["cloud_after"][:, 0] > 700).all())


def test_fit_cloud_plane_replays_from_a_captured_graph():
    dev = _dev()
    c = S.surface_inputs()
    y, w, pts = _cloud_inputs(dev)
    kw = dict(rounds=2, cloud_solver="gn", metric="plane")
    eager = _cpu(_fitter(dev, S.surface_sd(), iters=5).fit_cloud(y, pts, w, state=_state(dev, c.near), **kw))
    fitter = _fitter(dev, S.surface_sd(), iters=5)
    st = _state(dev, c.near)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fitter.fit_cloud(y, pts, w, state=st, **kw)  # warm-up outside the capture
        for s, s0 in zip(st, c.near):
            s.copy_(s0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = fitter.fit_cloud(y, pts, w, state=st, **kw)
    torch.cuda.current_stream(dev).wait_stream(side)
    for _ in range(2):
        for s, s0 in zip(st, c.near):
            s.copy_(s0)
        graph.replay()
        torch.cuda.synchronize(dev)
        _same(eager, {k: v.cpu() for k, v in out.items()})


def test_fit_cloud_without_the_new_arguments_keeps_its_bits():
    """metric="point" is the composition of associate and fit_mesh_gn the parent revision ran, on the synthetic hand and its cloud"""
    dev = _dev()
    c = M.fit_inputs()
    y, w, pts = _d(dev, c.target), _d(dev, c.weight), _d(dev, MM.cloud())
    outs = [_cpu(_fitter(dev, iters=5).fit_cloud(y, pts, w, state=_state(dev, c.starts["near"]), rounds=2, cloud_solver="gn", **kw))
            for kw in ({}, {"metric": "point", "facing_min": 0.5, "normal_sign": -1.0})]
    assert set(outs[0]) == set(outs[1]) and "normals" not in outs[0] and "visible" not in outs[0] and tuple(outs[0]["cloud_after"].shape) == (3, 2)
    _same(outs[0], outs[1])
    f = _fitter(dev, iters=5)
    st = _state(dev, c.starts["near"])
    fit = f.fit(y, w, state=st)
    first = None
    for _ in range(2):
        a = {k: v.clone() for k, v in f.associate(pts, fit["verts3d"]).items()}
        first = a if first is None else first
        fit = f.fit_mesh_gn(y, w, a["vert_target"], a["vert_weight"], state=st, init_trans=False, iters=2)
    last = f.associate(pts, fit["verts3d"])
    for k in BITS:
        assert torch.equal(outs[0][k], fit[k].cpu()), k
    assert torch.equal(outs[0]["cloud_before"], first["stats"].cpu()) and torch.equal(outs[0]["cloud_after"], last["stats"].cpu())
    for k in ("idx", "vert_target", "vert_weight"):
        assert torch.equal(outs[0][k], last[k].cpu()), k
    with pytest.raises(ValueError):
        f.fit_cloud(y, pts, w, metric="plane", cloud_solver="adam")
