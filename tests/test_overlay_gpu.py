"""kpf_overlay_project_f32, kpf_overlay_draw_u8 and overlay.FrameOverlay.  The kernels are held to the BITS of overlay.draw_host, the
numpy-float32 statement of the rule (checked against hand-computed pixels in test_overlay_host.py): integers with array_equal, floats through their bits,
no pixel left out, never a tolerance.  The grid is 70 x 100 (two by two tiles, partial at both edges), F = 2 frames, B = 3 hands."""
import functools

import numpy as np
import pytest
import torch

import mano_raster_cases as R
import overlay_cases as C
from keypointfusion_amd import overlay as O
from test_heads_gpu import _dev

pytestmark = pytest.mark.gpu


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _overlay(dev, frames=C.F, frame_index=C.FRAME_INDEX, size=(C.H, C.W), faces=None, **kw):
    return O.FrameOverlay(C.faces() if faces is None else faces, dev, size, frames, frame_index, **kw)


def _run(ov, dev, c, with_mesh=True, with_skel=True, **kw):
    """one draw of the case's arrays -> numpy copies of the outputs and of launch 1's buffers"""
    B = len(c["cam"])
    out = ov.draw(_t(dev, c["rgb"]), _t(dev, c["verts3d"]) if with_mesh else None, _t(dev, c["cam"]) if with_mesh else None,
                  _t(dev, c["normals"]) if with_mesh else None, _t(dev, c["joints_px"]) if with_skel else None, **{k: _t(dev, v) for k, v in kw.items()})
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy().copy() for k, v in out.items()}
    got["project"] = {k: ov._bufs[B][k].cpu().numpy().copy() for k in C.PROJECT}
    return got


def test_the_full_case_is_the_host_restatement_bit_for_bit():
    dev = _dev()
    c, want = C.full_case(), C.full_host()
    got = _run(_overlay(dev), dev, c)
    C.same(got, want, "full")
    C.same(got["project"], want["project"], "launch 1", C.PROJECT)
    print("OVERLAY full: labels %s rect %s" % (np.bincount(got["label"].ravel(), minlength=5).tolist(), got["project"]["rect"].tolist()))
    # the mesh alone and the skeleton alone
    C.same(_run(_overlay(dev), dev, c, with_skel=False), C.host(c, joints_px=None), "mesh only")
    C.same(_run(_overlay(dev), dev, c, with_mesh=False), C.host(c, verts3d=None), "skeleton only")
    # other parameters: per-hand colours, no normals, a wide skeleton
    col = np.asarray([[255.0, 40.0, 10.0], [20.0, 250.0, 60.0], [30.0, 90.0, 255.0]], np.float32)
    kw = dict(mesh_color=col, alpha=0.85, ambient=0.1, joint_radius=3.5, bone_half_width=1.6)
    C.same(_run(_overlay(dev, **kw), dev, c), C.host(c, **kw), "parameters")
    bare = dict(c, normals=None)
    got = _run(_overlay(dev), dev, bare)
    C.same(got, C.host(bare), "no normals")
    assert bool((got["project"]["shade"] == 1).all())


def test_the_nearer_hand_owns_the_overlap_whatever_the_order():
    dev = _dev()
    c = C.subset(C.full_case(), (0, 1))
    one = dict(frames=1, frame_index=(0, 0))
    rgb1 = dict(rgb=c["rgb"][:1])
    both = _run(_overlay(dev, **one), dev, dict(c, **rgb1), with_skel=False)
    C.same(both, C.host(dict(c, **rgb1), joints_px=None, frame_index=(0, 0)), "both")
    alone = [_run(_overlay(dev, frames=1, frame_index=(0,)), dev, dict(C.subset(c, (b,)), **rgb1), with_skel=False) for b in (0, 1)]
    d0, d1 = alone[0]["depth"], alone[1]["depth"]
    lap = (d0 > 0) & (d1 > 0)
    assert lap.sum() > 300 and (d1[lap] < d0[lap]).mean() > 0.9  # hand 1 is 60 mm nearer
    assert np.array_equal(both["depth"][lap], np.minimum(d0, d1)[lap]) and np.array_equal(both["owner"][lap], np.where(d1 < d0, 1, 0)[lap].astype(np.int32))
    assert np.array_equal(both["owner"][(d0 > 0) & ~(d1 > 0)], np.zeros(int(((d0 > 0) & ~(d1 > 0)).sum()), np.int32))
    swapped = _run(_overlay(dev, **one), dev, dict(C.subset(c, (1, 0)), **rgb1), with_skel=False)
    assert np.array_equal(swapped["owner"], np.where(both["owner"] >= 0, 1 - both["owner"], -1))
    C.same(swapped, both, "swapped", ("image", "label", "prim", "depth"))


def test_frames_and_batch_positions_are_independent():
    dev = _dev()
    c, full = C.full_case(), C.full_host()
    got = _run(_overlay(dev), dev, c)
    # frame 0 without hand 2 on frame 1
    two = _run(_overlay(dev, frame_index=(0, 0)), dev, C.subset(c, (0, 1)))
    for k in C.OUTPUTS:
        assert np.array_equal(two[k][0], got[k][0]), k
    assert np.array_equal(two["image"][1], c["rgb"][1]) and not two["label"][1].any()
    # hand 2 alone at batch position 0, and at position 2 behind two hands that are switched off
    solo = _run(_overlay(dev, frame_index=(1,)), dev, C.subset(c, (2,)))
    last = _run(_overlay(dev), dev, c, status=np.asarray([1, 1, 0], np.int32))
    for k in ("image", "label", "prim", "depth"):
        assert np.array_equal(solo[k][1], got[k][1]) and np.array_equal(last[k][1], got[k][1]), k
    assert np.array_equal(solo["owner"][1], np.where(got["owner"][1] >= 0, 0, -1)) and np.array_equal(last["owner"][1], got["owner"][1])
    assert np.array_equal(last["image"][0], c["rgb"][0]) and np.array_equal(got["image"], full["image"])


def test_the_scene_hides_the_mesh_behind_it():
    dev = _dev()
    c, plain = C.full_case(), C.full_host()
    seen = np.zeros((C.F, C.H, C.W), np.uint16)
    box = (slice(20, 68), slice(48, 90))
    near = plain["depth"][0][box]
    seen[0][box] = int(near[near > 0].min()) - 50  # a plate 50 mm in front of the nearest point of the hands under it
    want = C.host(c, depth_frame=seen)
    got = _run(_overlay(dev), dev, c, depth_frame=seen)
    C.same(got, want, "plate")
    inbox = np.zeros((C.F, C.H, C.W), bool)
    inbox[0][box] = True
    hidden = inbox & (plain["label"] == O.LABEL_MESH)
    assert hidden.sum() > 500 and np.array_equal(got["label"] == O.LABEL_HIDDEN, hidden)
    assert np.array_equal(got["image"][hidden], c["rgb"][hidden]) and np.array_equal(got["depth"], plain["depth"]) and bool((got["depth"][hidden] > 0).all())
    C.same(_run(_overlay(dev), dev, c, depth_frame=c["depth_zero"]), plain, "zero depth frame")
    C.same(_run(_overlay(dev, occl_margin=60.0), dev, c, depth_frame=seen), C.host(c, depth_frame=seen, occl_margin=60.0), "margin 60")


def test_gating_and_degenerate_input():
    dev = _dev()
    c, full = C.full_case(), C.full_host()
    status = np.asarray([0, 1, 0], np.int32)
    got = _run(_overlay(dev), dev, c, status=status)
    C.same(got, C.host(c, status=status), "status")
    assert not (got["owner"] == 1).any() and (got["owner"] == 0).sum() > (full["owner"] == 0).sum()
    # NaN vertices in hand 0, a NaN joint in hand 1, hand 2 behind the camera
    bad = {k: v.copy() for k, v in c.items()}
    bad["verts3d"][0, 100:140] = np.nan
    bad["verts3d"][0, 200, 2] = np.inf
    bad["joints_px"][1, 14, 0] = np.nan
    bad["verts3d"][2, :, 2] *= -1.0
    bad["verts3d"][2, 5, 2] = 0.0
    bad["normals"] = C.S.normals_host(bad["verts3d"], C.faces())
    want = C.host(bad)
    got = _run(_overlay(dev), dev, bad)
    C.same(got, want, "degenerate")
    C.same(got["project"], want["project"], "degenerate launch 1", C.PROJECT)
    r = got["project"]["rect"][2]
    assert (r[2] < r[0] or r[3] < r[1]) and not got["project"]["ok"][2].any() and not (got["depth"][1] > 0).any()
    assert got["project"]["ok"][0].sum() == 778 - 41 and (got["owner"] == 0).sum() > 0
    # hand 1's mesh is untouched by its neighbours' trouble, and its skeleton loses joint 14 and the two bones that end there
    assert all(np.array_equal(got["project"][k][1], full["project"][k][1]) for k in C.PROJECT)
    skel1 = (got["owner"] == 1) & (got["label"] >= 2) & (got["label"] <= 3)
    assert skel1.any() and not ((got["label"] == O.LABEL_JOINT) & (got["owner"] == 1) & (got["prim"] == 14)).any()
    gone = [i for i, (a, b) in enumerate(O.MANO21_BONES) if 14 in (a, b)]
    assert len(gone) == 2 and not ((got["label"] == O.LABEL_BONE) & (got["owner"] == 1) & np.isin(got["prim"], gone)).any()


def test_the_crop_form_is_the_crop_renders_depth_and_face():
    dev = _dev()
    from keypointfusion_amd import lib as L
    v, f = R.hands()[:3], R.surface_faces()
    cam, Mx = R.crop_for(v, (128, 128))
    rgb = np.random.Generator(np.random.PCG64(191)).integers(0, 256, (3, 128, 128, 3), dtype=np.uint8)
    ov = _overlay(dev, frames=3, frame_index=None, size=(128, 128), faces=f)
    vd, fd, cd, md = _t(dev, v), _t(dev, f), _t(dev, cam), _t(dev, Mx)
    out = ov.draw(_t(dev, rgb), vd, cd, None, None, M=md)
    # kpf_mano_raster_f32 itself, on the same arrays
    ras = [torch.empty(3, 128, 128, device=dev), torch.empty(3, 128, 128, device=dev, dtype=torch.int32), torch.empty(3, 778, device=dev, dtype=torch.int32),
           torch.empty(3, 4, device=dev)]
    L.check(L.load().kpf_mano_raster_f32(vd.data_ptr(), fd.data_ptr(), len(f), cd.data_ptr(), md.data_ptr(), 128, 128, 10.0, None,
                                         *[t.data_ptr() for t in ras], 3, torch.cuda.current_stream().cuda_stream), "kpf_mano_raster_f32")
    torch.cuda.synchronize(dev)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    rd, rf = ras[0].cpu().numpy(), ras[1].cpu().numpy()
    mesh = got["label"] == O.LABEL_MESH
    assert mesh.sum() > 6000 and np.array_equal(mesh, rf >= 0)
    assert np.array_equal(got["depth"].view(np.uint32), rd.view(np.uint32)) and np.array_equal(got["prim"], rf)
    assert np.array_equal(got["owner"], np.where(mesh, np.arange(3, dtype=np.int32)[:, None, None], -1))
    C.same(got, O.draw_host(rgb, f, v, cam, M=Mx), "crop form")


def test_eager_and_replayed_draws_agree_and_nothing_is_allocated_after_the_first_call():
    dev = _dev()
    c = C.full_case()
    steps = []
    for i in range(3):
        s = {k: v.copy() for k, v in c.items()}
        s["verts3d"] = s["verts3d"] + np.float32(4.0 * i) * np.asarray([1.0, -0.5, 2.0], np.float32)
        s["joints_px"][..., :2] += np.float32(1.25 * i)
        steps.append(s)
    rgb, seen = _t(dev, c["rgb"]), _t(dev, c["depth_zero"])
    status = _t(dev, np.zeros(3, np.int32))
    ov = _overlay(dev)
    eager, ptrs = [], None
    for s in steps:
        out = ov.draw(rgb, _t(dev, s["verts3d"]), _t(dev, s["cam"]), _t(dev, s["normals"]), _t(dev, s["joints_px"]), status, seen)
        torch.cuda.synchronize(dev)
        here = {k: t.data_ptr() for k, t in out.items()}
        here.update({"buf_" + k: t.data_ptr() for k, t in ov._bufs[3].items()})
        assert ptrs is None or here == ptrs
        ptrs = here
        eager.append({k: t.cpu().numpy().copy() for k, t in out.items()})
    C.same(eager[0], C.host(steps[0], status=np.zeros(3, np.int32), depth_frame=c["depth_zero"]), "eager 0")
    assert not np.array_equal(eager[0]["image"], eager[2]["image"])
    vd, cd, nd, jd = (_t(dev, steps[0][k]).clone() for k in ("verts3d", "cam", "normals", "joints_px"))
    gv = _overlay(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        gv.draw(rgb, vd, cd, nd, jd, status, seen)  # warm-up outside the capture: the buffers exist
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = gv.draw(rgb, vd, cd, nd, jd, status, seen)
    torch.cuda.current_stream(dev).wait_stream(side)
    for s, want in zip(steps, eager):
        vd.copy_(_t(dev, s["verts3d"]))
        jd.copy_(_t(dev, s["joints_px"]))
        for t in out.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        C.same({k: t.cpu().numpy() for k, t in out.items()}, want, "replay")


# ----------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw_inputs():
    """a small valid call: B = 2 hands on F = 1 frame of 20 x 24, 4 faces, J = 3 joints, 2 bones"""
    rng = np.random.Generator(np.random.PCG64(192))
    return dict(rgb=rng.integers(0, 256, (1, 20, 24, 3), dtype=np.uint8), faces=np.asarray([[0, 1, 2], [2, 1, 3], [3, 4, 5], [5, 6, 0]], np.int32),
                sx=(24 * rng.random((2, 778))).astype(np.float32), sy=(20 * rng.random((2, 778))).astype(np.float32),
                iz=np.full((2, 778), 1 / 500.0, np.float32), shade=np.ones((2, 778), np.float32), ok=np.ones((2, 778), np.int32),
                rect=np.asarray([[0, 0, 23, 19]] * 2, np.int32), mesh_color=np.full((2, 3), 128.0, np.float32), frame_index=np.zeros(2, np.int32),
                joints_px=(18 * rng.random((2, 3, 3))).astype(np.float32))


def _raw_draw(dev, change):
    """kpf_overlay_draw_u8 on _raw_inputs() with `change` applied to the descriptor -> (return code, out, error text); out starts as 7s"""
    from keypointfusion_amd import lib as L
    a = {k: _t(dev, v) for k, v in _raw_inputs().items()}
    out = torch.full((1, 20, 24, 3), 7, dtype=torch.uint8, device=dev)
    side = {"label": torch.full((1, 20, 24), 7, dtype=torch.uint8, device=dev), "owner": torch.full((1, 20, 24), 7, dtype=torch.int32, device=dev),
            "prim": torch.full((1, 20, 24), 7, dtype=torch.int32, device=dev), "depth": torch.full((1, 20, 24), 7.0, device=dev)}
    host = {"bones": np.asarray([[0, 1], [1, 2]], np.int32), "bone_color": np.full((2, 3), 9, np.uint8), "joint_color": np.full((3, 3), 5, np.uint8)}
    d = L.OverlayDrawDesc()
    for k, t in list(a.items()) + list(side.items()):
        setattr(d, k, t.data_ptr())
    for k, h in host.items():
        setattr(d, k, h.ctypes.data)
    d.out = out.data_ptr()
    d.B, d.F, d.H, d.W, d.Fc, d.J, d.NB = 2, 1, 20, 24, 4, 3, 2
    d.occl_margin, d.alpha, d.joint_radius, d.bone_half_width = 10.0, 0.6, 2.0, 0.75
    for k, v in change.items():
        if k == "bones" and v is not None:
            host["bones"] = np.asarray(v, np.int32)
            d.bones = host["bones"].ctypes.data
        elif k == "out_is_rgb":
            d.out = a["rgb"].data_ptr()
        else:
            setattr(d, k, v)
    rc = L.load().kpf_overlay_draw_u8(L.C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    err = L.load().kpf_last_error().decode()
    untouched = bool((out == 7).all()) and all(bool((t == 7).all()) for t in side.values())
    return rc, untouched, err, (out.cpu().numpy(), {k: t.cpu().numpy() for k, t in side.items()})


BAD_DRAWS = [dict(rgb=None), dict(out=None), dict(sy=None), dict(rect=None), dict(faces=None), dict(mesh_color=None), dict(joint_color=None), dict(bones=None),
             dict(B=0), dict(B=1 << 20), dict(F=0), dict(H=0), dict(W=-3), dict(frame_index=None), dict(Fc=0), dict(Fc=2049), dict(J=0), dict(J=65), dict(NB=65),
             dict(alpha=-0.01), dict(alpha=1.5), dict(alpha=float("nan")), dict(joint_radius=-1.0), dict(joint_radius=float("inf")),
             dict(bone_half_width=float("nan")), dict(bone_half_width=-0.5), dict(bones=[[0, 1], [1, 3]]), dict(bones=[[-1, 1], [1, 2]]), dict(out_is_rgb=True)]


@pytest.mark.parametrize("bad", BAD_DRAWS, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()).replace(" ", ""))
def test_draw_refuses_and_writes_nothing(bad):
    dev = _dev()
    rc, untouched, err, _ = _raw_draw(dev, bad)
    assert rc != 0 and untouched and err.startswith("kpf_overlay_draw_u8"), (rc, err)


def test_the_raw_call_the_refusals_start_from_draws():
    dev = _dev()
    rc, untouched, _, (out, side) = _raw_draw(dev, {})
    assert rc == 0 and not untouched and (side["label"] == O.LABEL_MESH).any() and (side["label"] >= 2).any() and not (side["label"] == 7).any()


@pytest.mark.parametrize("bad", [dict(ambient=-0.1), dict(ambient=1.01), dict(ambient=float("nan")), dict(B=1 << 20), dict(W=0), dict(cam=None), dict(rect=None)])
def test_project_refuses_and_writes_nothing(bad):
    dev = _dev()
    from keypointfusion_amd import lib as L
    c = C.full_case()
    v, cam = _t(dev, c["verts3d"]), _t(dev, c["cam"])
    outs = [torch.full((3, 778), 7.0, device=dev) for _ in range(4)] + [torch.full((3, 778), 7, dtype=torch.int32, device=dev), torch.full((3, 4), 7, dtype=torch.int32, device=dev)]
    kw = dict(ambient=0.3, B=3, W=C.W, cam=cam.data_ptr(), rect=outs[5].data_ptr())
    kw.update(bad)
    rc = L.load().kpf_overlay_project_f32(v.data_ptr(), None, kw["cam"], None, 0.0, kw["ambient"], C.H, kw["W"], *[t.data_ptr() for t in outs[:5]], kw["rect"],
                                          kw["B"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    assert rc != 0 and L.load().kpf_last_error().decode().startswith("kpf_overlay_project_f32") and all(bool((t == 7).all()) for t in outs)


def test_the_wrapper_refuses_what_it_can_see():
    dev = _dev()
    c = C.full_case()
    ov = _overlay(dev)
    with pytest.raises(ValueError):
        ov.draw(_t(dev, c["rgb"]))
    with pytest.raises(ValueError):
        ov.draw(_t(dev, c["rgb"][:1]), _t(dev, c["verts3d"]), _t(dev, c["cam"]))
    with pytest.raises(ValueError):
        ov.draw(_t(dev, c["rgb"]), _t(dev, c["verts3d"]).double(), _t(dev, c["cam"]))
    with pytest.raises(ValueError):
        O.FrameOverlay(None, dev, (C.H, C.W), C.F, C.FRAME_INDEX).draw(_t(dev, c["rgb"]), _t(dev, c["verts3d"]), _t(dev, c["cam"]))
    from keypointfusion_amd import lib as L
    with pytest.raises(L.KpfError, match="alpha"):
        _overlay(dev, alpha=2.0).draw(_t(dev, c["rgb"]), _t(dev, c["verts3d"]), _t(dev, c["cam"]))
