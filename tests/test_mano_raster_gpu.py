"""kpf_mano_raster_f32 / ManoFitter.render_depth, kpf_mano_assoc_vis_mask_f32 / associate(vert_mask=...) and fit_cloud(occlusion="zbuffer") (DESIGN.md
4.16).  The kernels are held to the BITS of the numpy-float32 restatements (tests/mano_raster_cases.py::raster_host and associate_vis_mask_host, checked
against float64 in test_mano_raster_host.py): depth, face, occluded, stats, idx, targets and weights are compared with array_equal, never with a
tolerance.  B <= 3 per launch."""
import functools

import numpy as np
import pytest
import torch

import mano_cases as M
import mano_mesh_cases as MM
import mano_raster_cases as R
import mano_surface_cases as S
from test_heads_gpu import _dev

pytestmark = pytest.mark.gpu
NAMES = ("depth", "face", "occluded", "stats")
VIS = ("idx", "vert_target", "vert_weight", "visible", "stats")
STATE = ("mano_pose_aa", "mano_shape", "trans")


def _raster(dev, verts, faces, cam, Mx, H, W, margin=10.0, obs=None, fill=None, F=None):
    """the raw entry -> (return code, cpu numpy outputs in the order of NAMES)"""
    from keypointfusion_amd import lib as L
    d = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(np.array(a)).to(dt).to(dev).contiguous()  # noqa: E731
    v, f, c, m, o = d(verts), d(faces, torch.int32), d(cam), d(Mx), d(obs)
    B = v.shape[0]
    n = max(H * W, 1) if 0 < H * W <= 16384 else 16
    out = [torch.empty(B, n, device=dev), torch.empty(B, n, device=dev, dtype=torch.int32), torch.empty(B, R.NV, device=dev, dtype=torch.int32),
           torch.empty(B, 4, device=dev)]
    if fill is not None:
        for t in out:
            t.fill_(fill)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.load().kpf_mano_raster_f32(v.data_ptr(), f.data_ptr(), int(f.shape[0]) if F is None else F, c.data_ptr(), ptr(m), H, W, margin, ptr(o), *[t.data_ptr() for t in out], B,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    got = [t.cpu().numpy() for t in out]
    if fill is None:
        got[0], got[1] = got[0].reshape(B, H, W), got[1].reshape(B, H, W)
    return rc, got


def _same(got, want, what):
    for name, g, h in zip(NAMES, got, want):
        assert g.dtype == h.dtype and np.array_equal(g, h, equal_nan=True), (what, name, int((g != h).sum()))


@functools.lru_cache(maxsize=None)
def _case(size, with_M):
    """hands() in the window of `size`: (cam, M or None, depth_obs, raster_host's outputs with depth_obs).  Without M the crop map is folded into the
    camera (M is a scale and a shift: u' = s (x fx / z + u0) + t = x (s fx) / z + (s u0 + t)), which puts the same hand into the same window."""
    v = R.hands()
    cam, Mx = R.crop_for(v, size)
    if not with_M:
        cam = np.stack([Mx[:, 0, 0] * cam[:, 0], Mx[:, 1, 1] * cam[:, 1], Mx[:, 0, 0] * cam[:, 2] + Mx[:, 0, 2], Mx[:, 1, 1] * cam[:, 3] + Mx[:, 1, 2]], 1)
        cam, Mx = cam.astype(np.float32), None
    depth, face, occ, _ = R.raster_host(v, R.surface_faces(), cam, Mx, size[0], size[1], 10.0)
    obs = R.observed_from(depth)
    return cam, Mx, obs, (depth, face, occ, R.stats_host(depth, face, obs))


@pytest.mark.parametrize("with_obs", [False, True])
@pytest.mark.parametrize("with_M", [True, False])
@pytest.mark.parametrize("size", R.SIZES)
def test_raster_is_the_host_restatement_bit_for_bit(size, with_M, with_obs):
    dev = _dev()
    v, f = R.hands(), R.surface_faces()
    cam, Mx, obs, want = _case(size, with_M)
    if not with_obs:
        want = want[:3] + (want[3] * np.asarray([1, 0, 0, 0], np.float32),)
    for rows in (slice(0, 3), slice(3, 5)):  # surface_poses(), curl_poses()
        rc, got = _raster(dev, v[rows], f, cam[rows], None if Mx is None else Mx[rows], size[0], size[1], 10.0, obs[rows] if with_obs else None)
        assert rc == 0
        _same(got, [w[rows] for w in want], (size, with_M, with_obs, rows))
    print("MANO-RASTER %s M %s obs %s stats %s" % (size, with_M, with_obs, want[3].tolist()))
    if size == (128, 128):  # the case is not empty
        assert bool((want[3][:, 0] > 2000).all()) and bool((want[2].sum(1) > 100).all())
        if with_obs:
            assert bool((want[3][:, 2] > 500).all()) and bool((want[3][:, 2] < want[3][:, 0]).all()) and bool((want[3][:, 3] > 0).all())


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_constructed_scenes(name):
    dev = _dev()
    v, f, H, W, want = R.scene_render(name)
    rc, got = _raster(dev, v, f, R.UNIT, None, H, W)
    assert rc == 0
    _same(got, want, name)
    # the faces in the reverse order arrive at the pixels in another order: the same depths, and a tie goes to the lower index of THAT numbering
    rc, rev = _raster(dev, v, f[::-1], R.UNIT, None, H, W)
    assert rc == 0 and np.array_equal(rev[0], got[0]) and np.array_equal(rev[2], got[2])
    _same(rev, R.raster_host(v, f[::-1], R.UNIT, None, H, W, 10.0), name + " reversed")


def test_the_synthetic_hands_random_faces():
    """faces drawn at random span the whole hand: every pixel is contested by tens of faces, which is where the order of arrival would show"""
    dev = _dev()
    v, f = MM.true_mesh().numpy(), S.faces_of(M.model_sd())
    cam, Mx = R.crop_for(v, (48, 40))
    obs = R.observed_from(R.raster_host(v, f, cam, Mx, 48, 40, 5.0)[0])
    want = R.raster_host(v, f, cam, Mx, 48, 40, 5.0, obs)
    rc, got = _raster(dev, v, f, cam, Mx, 48, 40, 5.0, obs)
    assert rc == 0
    _same(got, want, "random faces")
    assert bool((want[3][:, 0] > 200).all())


@pytest.mark.parametrize("bad", [dict(H=129, W=128), dict(H=0, W=8), dict(margin=-1.0), dict(F=0), dict(F=2049)])
def test_raster_refuses_and_writes_nothing(bad):
    dev = _dev()
    v, f = R.hands()[:1], R.surface_faces()
    cam, Mx = R.crop_for(v, (16, 16))
    kw = dict(H=16, W=16, margin=10.0, F=len(f))
    kw.update(bad)
    rc, got = _raster(dev, v, f, cam, Mx, kw["H"], kw["W"], kw["margin"], fill=7, F=kw["F"])
    assert rc != 0
    for g in got:
        assert bool((g == 7).all())


def test_rows_do_not_depend_on_the_batch_a_repeat_or_a_graph_replay():
    dev = _dev()
    from keypointfusion_amd.mano_fit import ManoFitter
    v, f = R.hands(), R.surface_faces()
    cam, Mx, obs, want = _case((128, 128), True)
    _, all3 = _raster(dev, v[:3], f, cam[:3], Mx[:3], 128, 128, 10.0, obs[:3])
    _, again = _raster(dev, v[:3], f, cam[:3], Mx[:3], 128, 128, 10.0, obs[:3])
    _same(again, all3, "repeat")
    for b in range(3):
        _, one = _raster(dev, v[b:b + 1], f, cam[b:b + 1], Mx[b:b + 1], 128, 128, 10.0, obs[b:b + 1])
        _same(one, [a[b:b + 1] for a in all3], b)
    # the wrapper, eager and replayed from a captured graph
    fitter = ManoFitter(S.surface_sd(), dev)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a[:3])).to(dev)  # noqa: E731
    vd, cd, md, od = d(v), d(cam), d(Mx), d(obs)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eager = {k: t.cpu().numpy() for k, t in fitter.render_depth(vd, cd, md, (128, 128), 10.0, od).items()}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = fitter.render_depth(vd, cd, md, (128, 128), 10.0, od)
    torch.cuda.current_stream(dev).wait_stream(side)
    _same([eager[k] for k in NAMES], [w[:3] for w in want], "wrapper")
    st = eager["stats"]
    assert np.array_equal(eager["iou"], st[:, 2] / (st[:, 0] + st[:, 1] - st[:, 2])) and set(eager) == set(NAMES) | {"iou"}
    for _ in range(2):
        for k in NAMES:
            out[k].zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        _same([out[k].cpu().numpy() for k in NAMES], [eager[k] for k in NAMES], "replay")
        assert np.array_equal(out["iou"].cpu().numpy(), eager["iou"])
    assert "iou" not in fitter.render_depth(vd, cd, md, (32, 32))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the mask entry
# ----------------------------------------------------------------------------------------------------------------------------------------
def _assoc(dev, pts, w, verts, normals, mask, gate2, facing=0.0, masked_entry=True):
    """kpf_mano_assoc_vis_mask_f32 (or, masked_entry=False, kpf_mano_assoc_vis_f32) -> (return code, cpu numpy outputs in the order of VIS)"""
    from keypointfusion_amd import lib as L
    d = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(np.array(a)).to(dt).to(dev).contiguous()  # noqa: E731
    p, pw, v, nm, mk = d(pts), d(w), d(verts), d(normals), d(mask, torch.int32)
    B, N = p.shape[:2]
    out = [torch.empty(B, N, device=dev, dtype=torch.int32), torch.empty(B, S.NV, 3, device=dev), torch.empty(B, S.NV, device=dev),
           torch.empty(B, S.NV, device=dev, dtype=torch.int32), torch.empty(B, 4, device=dev)]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    tail = (gate2, facing, *[o.data_ptr() for o in out], B, N, torch.cuda.current_stream().cuda_stream)
    if masked_entry:
        rc = L.load().kpf_mano_assoc_vis_mask_f32(p.data_ptr(), ptr(pw), v.data_ptr(), nm.data_ptr(), ptr(mk), *tail)
    else:
        rc = L.load().kpf_mano_assoc_vis_f32(p.data_ptr(), ptr(pw), v.data_ptr(), nm.data_ptr(), *tail)
    torch.cuda.synchronize(dev)
    return rc, [o.cpu().numpy() for o in out]


def _same_vis(got, want, what):
    for name, g, h in zip(VIS, got, want):
        assert np.array_equal(g, h, equal_nan=True), (what, name, int((g != h).sum()))


@functools.lru_cache(maxsize=None)
def _vis_inputs():
    """surface_poses(), their fp32 normals, a 257-point cloud on their camera side with weights (every seventh 0)"""
    verts = S.surface_poses().numpy()
    pts = S.one_sided_cloud(verts, R.surface_faces(), N=257, sigma=2.0, seed=81).numpy()
    w = (2.0 * np.random.Generator(np.random.PCG64(82)).random((3, 257)) + 2.0 ** -10).astype(np.float32)
    w[:, 3::7] = 0.0
    return verts, S.normals_host(verts, R.surface_faces()), pts, w


def test_without_a_mask_and_with_ones_the_bits_are_the_visibility_entrys():
    dev = _dev()
    verts, nrm, pts, w = _vis_inputs()
    for gate2, facing in ((400.0, 0.0), (float("inf"), 0.5)):
        rc, old = _assoc(dev, pts, w, verts, nrm, None, gate2, facing, masked_entry=False)
        assert rc == 0
        for mask in (None, np.ones((3, 778), np.int32), np.full((3, 778), -3, np.int32)):  # any non-zero entry keeps the vertex
            rc, new = _assoc(dev, pts, w, verts, nrm, mask, gate2, facing)
            assert rc == 0
            _same_vis(new, old, (gate2, facing))
        _same_vis(old, R.associate_vis_mask_host(pts, w, verts, nrm, None, gate2, facing), "host")


def test_masks_of_zeros_of_one_vertex_and_of_the_renders_occlusion():
    dev = _dev()
    verts, nrm, pts, w = _vis_inputs()
    rc, none = _assoc(dev, pts, w, verts, nrm, np.zeros((3, 778), np.int32), 400.0)
    assert rc == 0 and bool((none[0] == -1).all()) and not none[3].any() and not none[4].any() and not none[1].any() and not none[2].any()
    _same_vis(none, R.associate_vis_mask_host(pts, w, verts, nrm, np.zeros((3, 778), np.int32), 400.0), "zeros")
    # hide the vertex of each hand's first matched point: the point goes to the next facing vertex
    _, plain = _assoc(dev, pts, w, verts, nrm, None, float("inf"))
    mask = np.ones((3, 778), np.int32)
    firsts = [int(np.nonzero(plain[0][b] >= 0)[0][0]) for b in range(3)]
    for b, n in enumerate(firsts):
        mask[b, plain[0][b, n]] = 0
    rc, got = _assoc(dev, pts, w, verts, nrm, mask, float("inf"))
    assert rc == 0
    _same_vis(got, R.associate_vis_mask_host(pts, w, verts, nrm, mask, np.inf), "one vertex")
    for b, n in enumerate(firsts):
        assert got[0][b, n] not in (-1, plain[0][b, n]) and got[3][b, plain[0][b, n]] == 0 and plain[3][b, plain[0][b, n]] == 1
        d = np.linalg.norm(verts[b].astype(np.float64) - pts[b, n], axis=-1)
        d[(plain[3][b] == 0) | (mask[b] == 0)] = np.inf
        assert got[0][b, n] == int(np.argmin(d))
    assert np.array_equal(got[4][:, 3], plain[4][:, 3] - 1)
    # the mask the fit uses, on the curled hands: 1 - occluded of the render hides facing vertices
    cv = R.curl_poses().numpy()
    cn = S.normals_host(cv, R.surface_faces())
    cp = R.curl_inputs().cloud.numpy()[:, :257]
    occ = R.rendered((128, 128))[2][3:]
    want = R.associate_vis_mask_host(cp, None, cv, cn, 1 - occ, 400.0)
    rc, got = _assoc(dev, cp, None, cv, cn, 1 - occ, 400.0)
    assert rc == 0
    _same_vis(got, want, "curl")
    facing = S.visible_host(cv, cn, 0.0)
    assert np.array_equal(got[3], facing & (1 - occ)) and bool(((facing.sum(1) - got[3].sum(1)) >= 30).all())


def test_the_wrapper_takes_the_mask():
    dev = _dev()
    from keypointfusion_amd.mano_fit import ManoFitter
    verts, nrm, pts, w = _vis_inputs()
    f = ManoFitter(S.surface_sd(), dev)
    p, pw, v, nm = (torch.from_numpy(t).to(dev).contiguous() for t in (pts, w, verts, nrm))
    mask = np.ones((3, 778), np.int32)
    mask[:, ::3] = 0
    out = {k: t.cpu().numpy() for k, t in f.associate(p, v, pw, max_dist=20.0, normals=nm, vert_mask=torch.from_numpy(mask).to(dev)).items()}
    _same_vis([out[k] for k in VIS], R.associate_vis_mask_host(pts, w, verts, nrm, mask, 400.0), "wrapper")
    with pytest.raises(ValueError):
        f.associate(p, v, pw, vert_mask=torch.from_numpy(mask).to(dev))
    with pytest.raises(ValueError):
        f.associate(p, v, pw, normals=nm, vert_mask=torch.from_numpy(mask).to(dev).float())


# ----------------------------------------------------------------------------------------------------------------------------------------
# fit_cloud(occlusion="zbuffer")
# ----------------------------------------------------------------------------------------------------------------------------------------
def _fitter(dev):
    from keypointfusion_amd.mano_fit import ManoFitter
    return ManoFitter(S.surface_sd(), dev, iters=5)


def _cpu(out):
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _curl(dev):
    c = R.curl_inputs()
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    obs = torch.from_numpy(R.observed_from(R.rendered((128, 128))[0][3:]))
    return c, d(c.target), d(c.weight), d(c.cloud), (d(c.cam), d(c.M)), d(obs)


def _state(dev, start):
    return tuple(s.clone().to(dev).contiguous() for s in start)


def _by_hand(f, y, w, pts, camera, obs, st, rounds):
    """fit_cloud(metric="plane", cloud_solver="gn", occlusion="zbuffer") composed from the public methods"""
    fit = f.fit(y, w, state=st)
    first = None
    for _ in range(rounds):
        nrm = f.normals(fit["verts3d"]).clone()
        ren = f.render_depth(fit["verts3d"], camera[0], camera[1], (128, 128), 10.0)
        a = {k: v.clone() for k, v in f.associate(pts, fit["verts3d"], normals=nrm, vert_mask=1 - ren["occluded"]).items()}
        first = a if first is None else first
        fit = f.fit_mesh_gn(y, w, a["vert_target"], a["vert_weight"], state=st, init_trans=False, iters=2, vert_normal=nrm)
    nrm = f.normals(fit["verts3d"]).clone()
    ren = {k: v.clone() for k, v in f.render_depth(fit["verts3d"], camera[0], camera[1], (128, 128), 10.0, depth_obs=obs).items()}
    last = {k: v.clone() for k, v in f.associate(pts, fit["verts3d"], normals=nrm, vert_mask=1 - ren["occluded"]).items()}
    return fit, (last if first is None else first), last, nrm, ren


@pytest.mark.parametrize("rounds", [2, 0])
def test_fit_cloud_zbuffer_is_the_composition_by_hand(rounds):
    dev = _dev()
    c, y, w, pts, camera, obs = _curl(dev)
    out = _cpu(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), rounds=rounds, cloud_solver="gn", metric="plane", occlusion="zbuffer",
                                      camera=camera, depth_obs=obs))
    fit, first, last, nrm, ren = _by_hand(_fitter(dev), y, w, pts, camera, obs, _state(dev, c.near), rounds)
    for k in STATE + ("verts3d", "joints3d", "mano_pose", "residual", "status") + (("history",) if rounds else ()):
        assert torch.equal(out[k], fit[k].cpu()), k
    assert torch.equal(out["cloud_before"], first["stats"].cpu()) and torch.equal(out["cloud_after"], last["stats"].cpu())
    for k in ("idx", "vert_target", "vert_weight", "visible"):
        assert torch.equal(out[k], last[k].cpu()), k
    assert torch.equal(out["normals"], nrm.cpu())
    for k, name in (("depth", "depth"), ("face", "face"), ("occluded", "occluded"), ("stats", "depth_stats"), ("iou", "iou")):
        assert torch.equal(out[name], ren[k].cpu()), name
    assert out["status"].tolist() == [0, 0] and bool((out["depth_stats"][:, 0] > 2000).all()) and bool((out["iou"] > 0).all()) and bool((out["iou"] < 1).all())
    # the mask is at work: fewer vertices are candidates than face the camera
    facing = S.visible_host(out["verts3d"].numpy(), out["normals"].numpy(), 0.0)
    assert np.array_equal(out["visible"].numpy(), facing & (1 - out["occluded"].numpy())) and bool(((facing.sum(1) - out["visible"].numpy().sum(1)) >= 30).all())
    # and without depth_obs there is no iou and the stats hold the coverage alone
    bare = _cpu(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), rounds=rounds, cloud_solver="gn", metric="plane", occlusion="zbuffer", camera=camera))
    assert "iou" not in bare and torch.equal(bare["depth"], out["depth"]) and not bare["depth_stats"][:, 1:].any()


def test_fit_cloud_zbuffer_replays_from_a_captured_graph():
    dev = _dev()
    c, y, w, pts, camera, obs = _curl(dev)
    kw = dict(rounds=2, cloud_solver="gn", metric="plane", occlusion="zbuffer", camera=camera, depth_obs=obs)
    eager = _cpu(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), **kw))
    fitter = _fitter(dev)
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
        for k in eager:
            assert torch.equal(eager[k], out[k].cpu()), k


def test_fit_cloud_without_occlusion_keeps_the_plane_calls_bits():
    dev = _dev()
    c, y, w, pts, camera, obs = _curl(dev)
    kw = dict(rounds=2, cloud_solver="gn", metric="plane", facing_min=0.25)
    a = _cpu(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), **kw))
    b = _cpu(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), occlusion=None, camera=camera, raster_size=(32, 32), occlusion_margin=2.0,
                                    depth_obs=obs, **kw))
    assert set(a) == set(b) and "depth" not in a and "occluded" not in a
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the composition the parent revision ran
    f = _fitter(dev)
    st = _state(dev, c.near)
    fit = f.fit(y, w, state=st)
    for _ in range(2):
        nrm = f.normals(fit["verts3d"]).clone()
        asc = {k: v.clone() for k, v in f.associate(pts, fit["verts3d"], normals=nrm, facing_min=0.25).items()}
        fit = f.fit_mesh_gn(y, w, asc["vert_target"], asc["vert_weight"], state=st, init_trans=False, iters=2, vert_normal=nrm)
    nrm = f.normals(fit["verts3d"])
    last = f.associate(pts, fit["verts3d"], normals=nrm, facing_min=0.25)
    for k in STATE + ("verts3d", "joints3d", "residual", "status", "history"):
        assert torch.equal(a[k], fit[k].cpu()), k
    for k in ("idx", "vert_target", "vert_weight", "visible"):
        assert torch.equal(a[k], last[k].cpu()), k
