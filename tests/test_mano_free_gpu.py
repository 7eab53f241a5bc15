"""kpf_depth_silhouette_f32 / ManoFitter.silhouette, kpf_mano_free_space_f32 / ManoFitter.free_space and fit_cloud(free_space="silhouette") (DESIGN.md
4.18).  The kernels are held to the BITS of the numpy restatements (tests/mano_free_cases.py::silhouette_host and free_space_host, checked against the
definition and against float64 in test_mano_free_host.py): every output is compared with array_equal, never with a tolerance.  B <= 3 per launch."""
import numpy as np
import pytest
import torch

import mano_free_cases as F
import mano_raster_cases as R
import mano_surface_cases as S
from test_heads_gpu import _dev
from test_mano_raster_gpu import _cpu, _curl, _fitter, _state

pytestmark = pytest.mark.gpu
SIL = ("nearest", "dist2", "front", "count")
FREE = ("vert_target", "vert_weight", "vert_normal", "kind", "stats")
STATE = ("mano_pose_aa", "mano_shape", "trans")
INF = float("inf")


def _d(dev, a, dt=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev).contiguous()


def _silhouette(dev, depth):
    """the raw entry -> (return code, cpu numpy outputs in the order of SIL)"""
    from keypointfusion_amd import lib as L
    d = _d(dev, depth)
    B, H, W = d.shape
    out = [torch.full((B, H, W), 7, device=dev, dtype=torch.int32), torch.full((B, H, W), 7, device=dev, dtype=torch.int32),
           torch.full((B, H, W), 7.0, device=dev), torch.full((B,), 7, device=dev, dtype=torch.int32)]
    rc = L.load().kpf_depth_silhouette_f32(d.data_ptr(), H, W, *[t.data_ptr() for t in out], B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, [t.cpu().numpy() for t in out]


def _free(dev, verts, cam, Mx, sil, slack2=1, margin=5.0, step=20.0, lam=1.0, vt=None, vw=None, vn=None):
    """the raw entry -> (return code, cpu numpy outputs in the order of FREE)"""
    from keypointfusion_amd import lib as L
    v, c, m, tin, win, nin = (_d(dev, a) for a in (verts, cam, Mx, vt, vw, vn))
    near, dist, front = _d(dev, sil[0], torch.int32), _d(dev, sil[1], torch.int32), _d(dev, sil[2])
    B, H, W = front.shape
    out = [torch.full((B, F.NV, 3), 7.0, device=dev), torch.full((B, F.NV), 7.0, device=dev), torch.full((B, F.NV, 3), 7.0, device=dev),
           torch.full((B, F.NV), 7, device=dev, dtype=torch.int32), torch.full((B, 4), 7.0, device=dev)]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.load().kpf_mano_free_space_f32(v.data_ptr(), c.data_ptr(), ptr(m), H, W, near.data_ptr(), dist.data_ptr(), front.data_ptr(), slack2, margin, step,
                                          lam, ptr(tin), ptr(win), ptr(nin), *[t.data_ptr() for t in out], B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, [t.cpu().numpy() for t in out]


def _same(names, got, want, what):
    for name, g, h in zip(names, got, want):
        assert g.dtype == h.dtype and g.shape == h.shape, (what, name, g.dtype, h.dtype)
        bits = (lambda a: a.view(np.uint32)) if g.dtype == np.float32 else (lambda a: a)
        assert np.array_equal(bits(g), bits(h)), (what, name, int((bits(g) != bits(h)).sum()))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the silhouette
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", F.SIL_SIZES)
def test_silhouette_of_the_masks_is_the_host_restatement(size):
    dev = _dev()
    for name, depth in F.mask_cases(*size).items():
        rc, got = _silhouette(dev, depth)
        assert rc == 0
        _same(SIL, got, F.silhouette_host(depth), (size, name))


@pytest.mark.parametrize("size", [(128, 128), (32, 32), (16, 64)])
def test_silhouette_of_the_rendered_hands(size):
    dev = _dev()
    obs = F.render_obs(size)
    want = F.silhouette_host(obs)
    for rows in (slice(0, 3), slice(3, 5)):
        rc, got = _silhouette(dev, obs[rows])
        assert rc == 0
        _same(SIL, got, [w[rows] for w in want], (size, rows))
    assert bool((want[3] > 0.1 * size[0] * size[1]).all())
    if size == (128, 128):  # rows do not depend on the batch or on a repeat; NaN, 0 and negative depths are not observed
        pat = R.observed_from(obs)[:3]
        _, all3 = _silhouette(dev, pat)
        _, again = _silhouette(dev, pat)
        _same(SIL, again, all3, "repeat")
        _same(SIL, all3, F.silhouette_host(pat), "pattern")
        for b in range(3):
            _, one = _silhouette(dev, pat[b:b + 1])
            _same(SIL, one, [a[b:b + 1] for a in all3], b)


def test_silhouette_refuses_and_writes_nothing():
    dev = _dev()
    from keypointfusion_amd import lib as L
    out = torch.full((4, 64), 7, device=dev, dtype=torch.int32)
    d = torch.zeros(1, 8, 8, device=dev)
    for H, W in ((0, 8), (129, 128), (8, -1)):
        assert L.load().kpf_depth_silhouette_f32(d.data_ptr(), H, W, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), 1,
                                                 torch.cuda.current_stream().cuda_stream) != 0
    torch.cuda.synchronize(dev)
    assert bool((out == 7).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# the free-space term
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_inputs", [True, False])
@pytest.mark.parametrize("with_M", [True, False])
@pytest.mark.parametrize("case", ["crossed", "self"])
def test_free_space_is_the_host_restatement_bit_for_bit(case, with_M, with_inputs):
    dev = _dev()
    v, cam, Mx, sil = (F.crossed if case == "crossed" else F.selfcase)((128, 128), with_M)
    vt, vw, vn = F.assoc_inputs() if with_inputs else (None, None, None)
    want = F.free_space_host(v, cam, Mx, sil, vert_target=vt, vert_weight=vw, vert_normal=vn)
    cut = lambda a, rows: None if a is None else a[rows]  # noqa: E731
    for rows in (slice(0, 3), slice(3, 5)):
        rc, got = _free(dev, v[rows], cam[rows], cut(Mx, rows), [s[rows] for s in sil[:3]], vt=cut(vt, rows), vw=cut(vw, rows), vn=cut(vn, rows))
        assert rc == 0
        _same(FREE, got, [w[rows] for w in want], (case, with_M, with_inputs, rows))
    kind = want[3]
    print("MANO-FREE %s M %s inputs %s: outside %s, in front %s" % (case, with_M, with_inputs, (kind == 1).sum(1).tolist(), (kind == 2).sum(1).tolist()))
    if case == "crossed":  # the case is not empty
        assert int((kind == 1).sum()) > 500 and int((kind == 2).sum()) > 200
    else:
        assert not kind.any()


def test_kind_0_vertices_pass_their_inputs_through_bit_for_bit():
    dev = _dev()
    v, cam, Mx, sil = F.crossed()
    vt, vw, vn = F.assoc_inputs()
    rc, got = _free(dev, v[:3], cam[:3], Mx[:3], [s[:3] for s in sil[:3]], lam=0.25, vt=vt[:3], vw=vw[:3], vn=vn[:3])
    assert rc == 0
    off, on = got[3] == 0, got[3] != 0
    assert int(off.sum()) > 500 and int(on.sum()) > 500
    for g, h in zip(got[:3], (vt[:3], vw[:3], vn[:3])):
        assert np.array_equal(g[off].view(np.uint32), h[off].view(np.uint32))
    assert bool(np.isnan(got[0][:, 5, 0][off[:, 5]]).all()) and bool((got[1][on] == 0.25).all())
    assert np.abs(np.linalg.norm(got[2][on].astype(np.float64), axis=-1) - 1).max() < 1e-6
    assert np.linalg.norm(got[0][on].astype(np.float64) - v[:3][on], axis=-1).max() <= 20.0 + 1e-3  # coordinates near 600 mm: half an ulp is 3e-5 mm
    rc, bare = _free(dev, v[:3], cam[:3], Mx[:3], [s[:3] for s in sil[:3]], lam=0.25)
    assert rc == 0 and np.array_equal(bare[3], got[3]) and np.array_equal(bare[4], got[4])
    for g, h in zip(bare[:3], got[:3]):
        assert np.array_equal(g[on].view(np.uint32), h[on].view(np.uint32)) and not g[off].any()


@pytest.mark.parametrize("variant", ["defaults", "margin_inf", "step_inf", "slack2_4", "singular_M", "nan_M", "background", "lambda_0"])
def test_constructed_scene(variant):
    dev = _dev()
    v, sil = F.scene_verts(), F.silhouette_host(F.scene_obs())
    kw, Mx = {}, None
    expect = list(F.SCENE_KINDS)
    if variant == "margin_inf":
        kw, expect = dict(margin=INF), [k if k == 1 else 0 for k in expect]
    elif variant == "step_inf":
        kw = dict(step=INF)
    elif variant == "slack2_4":
        kw, expect = dict(slack2=4), [0, 0, 0, 0, 0, 2, 2, 1, 1, 0, 0, 0]
    elif variant == "singular_M":
        Mx, expect = np.asarray([[[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]]], np.float32), [0] * 12
    elif variant == "nan_M":
        Mx, expect = np.asarray([[[1.0, 0.0, 0.0], [0.0, np.nan, 0.0]]], np.float32), [0] * 12
    elif variant == "background":
        sil, expect = F.silhouette_host(np.zeros((1, 16, 16), np.float32)), [0] * 12
    elif variant == "lambda_0":
        kw = dict(lambda_free=0.0)
    want = F.free_space_host(v, R.UNIT, Mx, sil, **kw)
    assert want[3][0, :12].tolist() == expect and not want[3][0, 12:].any()
    raw = dict(kw)
    if "lambda_free" in raw:
        raw["lam"] = raw.pop("lambda_free")
    rc, got = _free(dev, v, R.UNIT, Mx, sil, **raw)
    assert rc == 0
    _same(FREE, got, want, variant)
    if variant == "step_inf":  # unclamped: the centre of the nearest observed pixel at the vertex's depth, and depth front - margin along the ray
        assert np.array_equal(got[0][0, 2], np.asarray(R._at(4, 6, 512.0), np.float32)) and got[0][0, 6, 2] == 507.0
    if variant == "defaults":
        assert np.allclose(np.linalg.norm(got[0][0, [2, 6, 7]].astype(np.float64) - v[0, [2, 6, 7]], axis=-1), 20.0, rtol=1e-4)


def test_free_space_refuses_and_writes_nothing():
    dev = _dev()
    v, sil = F.scene_verts(), F.silhouette_host(F.scene_obs())
    for bad in (dict(slack2=-1), dict(margin=0.0), dict(margin=float("nan")), dict(step=0.0), dict(lam=-1.0), dict(vt=np.zeros((1, 778, 3), np.float32))):
        rc, got = _free(dev, v, R.UNIT, None, sil, **bad)
        assert rc != 0
        for g in got:
            assert bool((g == 7).all())


def test_the_wrappers_give_the_entries_bits_for_any_batch_and_on_a_repeat():
    dev = _dev()
    from keypointfusion_amd.mano_fit import ManoFitter
    v, cam, Mx, _ = F.crossed()
    obs = np.roll(F.render_obs((128, 128)), -1, 0)
    vt, vw, vn = F.assoc_inputs()
    f = ManoFitter(S.surface_sd(), dev)
    d = lambda a: _d(dev, a[:3])  # noqa: E731
    sil = f.silhouette(d(obs))
    want_sil = F.silhouette_host(obs[:3])
    _same(SIL, [sil[k].cpu().numpy() for k in SIL], want_sil, "silhouette")
    out = f.free_space(d(v), d(cam), d(Mx), sil, vert_target=d(vt), vert_weight=d(vw), vert_normal=d(vn))
    want = F.free_space_host(v[:3], cam[:3], Mx[:3], want_sil, vert_target=vt[:3], vert_weight=vw[:3], vert_normal=vn[:3])
    first = [out[k].cpu().numpy() for k in FREE]
    _same(FREE, first, want, "free_space")
    assert set(out) == set(FREE) and set(sil) == set(SIL)
    again = f.free_space(d(v), d(cam), d(Mx), sil, vert_target=d(vt), vert_weight=d(vw), vert_normal=d(vn))
    _same(FREE, [again[k].cpu().numpy() for k in FREE], first, "repeat")
    for b in range(3):
        one = lambda a: _d(dev, a[b:b + 1])  # noqa: E731
        s1 = f.silhouette(one(obs))
        o1 = f.free_space(one(v), one(cam), one(Mx), s1, vert_target=one(vt), vert_weight=one(vw), vert_normal=one(vn))
        _same(FREE, [o1[k].cpu().numpy() for k in FREE], [a[b:b + 1] for a in first], b)
    other = f.free_space(d(v), d(cam), d(Mx), sil, slack2=9, margin=INF, step=INF, lambda_free=2.0, _slot=1)
    _same(FREE, [other[k].cpu().numpy() for k in FREE], F.free_space_host(v[:3], cam[:3], Mx[:3], want_sil, 9, INF, INF, 2.0), "other rule")
    assert other["kind"].data_ptr() != out["kind"].data_ptr()
    with pytest.raises(ValueError):
        f.free_space(d(v), d(cam), d(Mx), f.silhouette(_d(dev, obs[:2])))  # another batch's maps
    with pytest.raises(ValueError):
        f.free_space(d(v), d(cam), d(Mx), sil, vert_target=d(vt), vert_weight=d(vw)[:, :700].contiguous())


# ----------------------------------------------------------------------------------------------------------------------------------------
# fit_cloud(free_space="silhouette")
# ----------------------------------------------------------------------------------------------------------------------------------------
RULE = dict(free_slack2=2, free_margin=4.0, free_step=15.0, lambda_free=0.5)
CHAINS = {"point": dict(cloud_solver="gn"), "plane": dict(cloud_solver="gn", metric="plane"),
          "zbuffer": dict(cloud_solver="gn", metric="plane", occlusion="zbuffer")}


def _clone(out):
    return {k: v.clone() for k, v in out.items()}


def _host(out):
    """_cpu for fit_cloud's output with the term: its `silhouette` is a dict of tensors"""
    return {k: _cpu(v) if isinstance(v, dict) else v.detach().cpu().clone() for k, v in out.items()}


def _by_hand(f, chain, y, w, pts, camera, obs, st, rounds):
    """fit_cloud(free_space="silhouette", **RULE) composed from the public methods -> (fit, first and last association, first and last free_space, sil)"""
    plane, zbuf = chain != "point", chain == "zbuffer"
    fit = f.fit(y, w, state=st)
    sil = f.silhouette(obs)
    first = free_first = None

    def assoc(verts, last):
        if not plane:
            return None, _clone(f.associate(pts, verts))
        nrm = f.normals(verts).clone()
        mask = 1 - f.render_depth(verts, camera[0], camera[1], (128, 128), 10.0, depth_obs=obs if last else None)["occluded"] if zbuf else None
        return nrm, _clone(f.associate(pts, verts, normals=nrm, vert_mask=mask))

    for _ in range(rounds):
        nrm, a = assoc(fit["verts3d"], False)
        fs = _clone(f.free_space(fit["verts3d"], camera[0], camera[1], sil, RULE["free_slack2"], RULE["free_margin"], RULE["free_step"], RULE["lambda_free"],
                                 a["vert_target"], a["vert_weight"], nrm))
        first, free_first = (a, fs) if first is None else (first, free_first)
        fit = f.fit_mesh_gn(y, w, fs["vert_target"], fs["vert_weight"], state=st, init_trans=False, iters=2, vert_normal=fs["vert_normal"] if plane else None)
    nrm, last = assoc(fit["verts3d"], True)
    rep = _clone(f.free_space(fit["verts3d"], camera[0], camera[1], sil, RULE["free_slack2"], RULE["free_margin"], RULE["free_step"], RULE["lambda_free"]))
    return fit, (last if first is None else first), last, (rep if free_first is None else free_first), rep, sil


@pytest.mark.parametrize("rounds", [2, 0])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_fit_cloud_free_space_is_the_composition_by_hand(chain, rounds):
    dev = _dev()
    c, y, w, pts, camera, obs = _curl(dev)
    kw = dict(CHAINS[chain], rounds=rounds, camera=camera, depth_obs=obs, free_space="silhouette", **RULE)
    out = _host(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), **kw))
    fit, first, last, free_first, rep, sil = _by_hand(_fitter(dev), chain, y, w, pts, camera, obs, _state(dev, c.near), rounds)
    for k in STATE + ("verts3d", "joints3d", "mano_pose", "residual", "status") + (("history",) if rounds else ()):
        assert torch.equal(out[k], fit[k].cpu()), k
    assert torch.equal(out["cloud_before"], first["stats"].cpu()) and torch.equal(out["cloud_after"], last["stats"].cpu())
    for k in ("idx", "vert_target", "vert_weight") + (("visible",) if chain != "point" else ()):
        assert torch.equal(out[k], last[k].cpu()), k
    assert torch.equal(out["free_before"], free_first["stats"].cpu()) and torch.equal(out["free_after"], rep["stats"].cpu())
    assert torch.equal(out["free_kind"], rep["kind"].cpu())
    for k in SIL:
        assert torch.equal(out["silhouette"][k].cpu(), sil[k].cpu()), k
    assert out["status"].tolist() == [0, 0]
    # the term is at work: the observation is the OTHER curled hand's render, so vertices of both kinds exist before the first round
    assert bool((out["free_before"][:, 0] > 0).all()) and bool((out["free_before"][:, 2] > 0).all())
    assert int((out["free_kind"] == 1).sum()) == int(out["free_after"][:, 0].sum())
    if rounds:  # and it changes the fit
        plain = _cpu(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), **dict(CHAINS[chain], rounds=rounds, camera=camera, depth_obs=obs)))
        assert not torch.equal(plain["verts3d"], out["verts3d"]) and "free_kind" not in plain and "silhouette" not in plain


def _only_tensors(out):
    flat = {k: v for k, v in out.items() if k != "silhouette"}
    flat.update({"silhouette." + k: v for k, v in out["silhouette"].items()})
    return flat


@pytest.mark.parametrize("chain", ["point", "zbuffer"])
def test_fit_cloud_free_space_replays_from_a_captured_graph(chain):
    dev = _dev()
    c, y, w, pts, camera, obs = _curl(dev)
    kw = dict(CHAINS[chain], rounds=2, camera=camera, depth_obs=obs, free_space="silhouette")
    eager = _cpu(_only_tensors(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), **kw)))
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
            out = _only_tensors(fitter.fit_cloud(y, pts, w, state=st, **kw))
    torch.cuda.current_stream(dev).wait_stream(side)
    for _ in range(2):
        for s, s0 in zip(st, c.near):
            s.copy_(s0)
        graph.replay()
        torch.cuda.synchronize(dev)
        for k in eager:
            assert torch.equal(eager[k], out[k].cpu()), k


def test_fit_cloud_without_free_space_keeps_the_previous_calls_bits_and_launches():
    dev = _dev()
    from keypointfusion_amd import lib as L
    c, y, w, pts, camera, obs = _curl(dev)
    for chain, per_round in (("point", 2), ("plane", 3), ("zbuffer", 4)):
        kw = dict(CHAINS[chain], rounds=2, camera=camera, depth_obs=obs)
        f = _fitter(dev)
        n0 = L.CALLS[0]
        a = _cpu(f.fit_cloud(y, pts, w, state=_state(dev, c.near), **kw))
        n1 = L.CALLS[0]
        b = _cpu(f.fit_cloud(y, pts, w, state=_state(dev, c.near), free_space=None, free_slack2=0, free_margin=1.0, free_step=1.0, lambda_free=9.0, **kw))
        n2 = L.CALLS[0]
        free = f.fit_cloud(y, pts, w, state=_state(dev, c.near), free_space="silhouette", **kw)
        n3 = L.CALLS[0]
        assert n1 - n0 == n2 - n1 == per_round * (2 + 1) and n3 - n2 == (n1 - n0) + (2 + 2)  # per_round * (rounds + 1) calls; the term adds rounds + 2
        assert set(a) == set(b) and set(free) == set(a) | {"free_before", "free_after", "free_kind", "silhouette"}
        for k in a:
            assert torch.equal(a[k], b[k]), (chain, k)
    # the composition the parent revision ran for the point metric
    f = _fitter(dev)
    st = _state(dev, c.near)
    fit = f.fit(y, w, state=st)
    for _ in range(2):
        asc = _clone(f.associate(pts, fit["verts3d"]))
        fit = f.fit_mesh_gn(y, w, asc["vert_target"], asc["vert_weight"], state=st, init_trans=False, iters=2)
    last = f.associate(pts, fit["verts3d"])
    a = _cpu(_fitter(dev).fit_cloud(y, pts, w, state=_state(dev, c.near), rounds=2, cloud_solver="gn"))
    for k in STATE + ("verts3d", "joints3d", "residual", "status", "history"):
        assert torch.equal(a[k], fit[k].cpu()), k
    for k in ("idx", "vert_target", "vert_weight"):
        assert torch.equal(a[k], last[k].cpu()), k
