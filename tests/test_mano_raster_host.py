"""Host side of the z-buffer render (ABI 31: kpf_mano_raster_f32, kpf_mano_assoc_vis_mask_f32): the export, the header and the binding, the refusals
without a launch, the fp32 restatement against float64, the pixel convention against the preprocessing's back-projection, scenes whose render is known by
construction, and what the curled hands show (tests/mano_raster_cases.py).  No GPU."""
import os
import re

import numpy as np
import pytest

import mano_raster_cases as R
import mano_surface_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kpf_mano_raster_f32", "kpf_mano_assoc_vis_mask_f32")
_X = 4096  # any non-null address: a refused call reads nothing


def _lib():
    from keypointfusion_amd import lib as L
    return L, L.load()


def test_header_library_and_binding_agree_on_the_raster_entries():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 31 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    for name in NAMES:
        assert name in L.EXPORTS and re.search(r"\bint %s\(" % name, hdr) and getattr(lib, name), name
    # the mask entry: the visibility entry's arguments with vert_mask after normals
    vis, mask = L._SIGS["kpf_mano_assoc_vis_f32"], L._SIGS[NAMES[1]]
    assert len(mask) == len(vis) + 1 and mask[:4] == vis[:4] and mask[5:] == vis[4:]


def _refused(lib, name, rc):
    assert rc != 0
    assert lib.kpf_last_error().decode().startswith(name + ": "), lib.kpf_last_error()


def test_raster_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()

    def call(verts=_X, faces=_X, F=8, cam=_X, M=None, H=16, W=16, margin=10.0, obs=None, depth=_X, face=_X, occ=_X, stats=_X, B=1):
        return lib.kpf_mano_raster_f32(verts, faces, F, cam, M, H, W, margin, obs, depth, face, occ, stats, B, None)

    for bad in (dict(F=0), dict(F=2049), dict(H=0), dict(W=0), dict(H=-1, W=-1), dict(H=129, W=128), dict(H=1, W=16385), dict(H=65536, W=65536),
                dict(margin=-1.0), dict(margin=float("nan")), dict(margin=float("inf")), dict(verts=None), dict(faces=None), dict(cam=None),
                dict(depth=None), dict(face=None), dict(occ=None), dict(stats=None), dict(B=0)):
        _refused(lib, NAMES[0], call(**bad))


def test_mask_entry_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()

    def call(points=_X, verts=_X, normals=_X, mask=_X, gate=400.0, facing=0.0, idx=_X, vt=_X, vw=_X, vis=_X, stats=_X, B=1, N=16):
        return lib.kpf_mano_assoc_vis_mask_f32(points, None, verts, normals, mask, gate, facing, idx, vt, vw, vis, stats, B, N, None)

    for bad in (dict(N=0), dict(N=4097), dict(facing=1.0), dict(facing=-0.1), dict(facing=float("nan")), dict(normals=None), dict(vis=None),
                dict(stats=None), dict(gate=-1.0), dict(gate=float("nan")), dict(B=0), dict(mask=None, N=0)):
        _refused(lib, NAMES[1], call(**bad))


def test_the_wrappers_refuse_before_anything_touches_the_device():
    from keypointfusion_amd.mano_fit import ManoFitter
    f = ManoFitter.__new__(ManoFitter)
    for kw in (dict(size=(129, 128)), dict(size=(0, 4)), dict(size=(4, 0)), dict(margin=-1.0), dict(margin=float("nan")), dict(margin=float("inf"))):
        with pytest.raises(ValueError):
            f.render_depth(None, None, **kw)
    with pytest.raises(ValueError):
        f.associate(None, None, vert_mask=object())  # a mask without normals
    for kw in (dict(occlusion="zbuffer"), dict(occlusion="zbuffer", metric="point", camera=(None, None)),
               dict(occlusion="zbuffer", metric="plane", cloud_solver="gn"), dict(occlusion="zbuffer", metric="plane", cloud_solver="gn", camera=(None,)),
               dict(occlusion="painter", metric="plane", cloud_solver="gn", camera=(None, None))):
        with pytest.raises(ValueError):
            f.fit_cloud(None, None, **kw)


def test_crop_helpers_follow_the_preprocessing():
    """crop_depth_mm is depth_to_pcl's dpt (img * cube_z / 2 + center_z, 0 where img is close to 1), crop_camera the top two rows of M"""
    import torch
    from keypointfusion_amd.mano_fit import crop_camera, crop_depth_mm
    rng = np.random.Generator(np.random.PCG64(5))
    img = (2 * rng.random((2, 1, 8, 8)) - 1).astype(np.float32)
    img[0, 0, 2, 3], img[1, 0, 0, 0], img[1, 0, 7, 7] = 1.0, 1.0 - 5e-6, 1.0 - 2e-5  # the first two are close to 1 by numpy.isclose, the third is not
    prep = {"img": torch.from_numpy(img), "cube": torch.tensor([[250.0, 250.0, 250.0], [200.0, 200.0, 300.0]]),
            "center": torch.tensor([[10.0, 20.0, 600.0], [-5.0, 0.0, 450.0]]), "cam_para": torch.tensor([[475.0, 475.0, 320.0, 240.0]] * 2),
            "M": torch.tensor([[[0.5, 0.0, 3.0], [0.0, 0.5, -2.0], [0.0, 0.0, 1.0]]] * 2)}
    d = crop_depth_mm(prep).numpy()
    for b in range(2):
        want = img[b, 0] * prep["cube"][b, 2].item() / 2.0 + prep["center"][b, 2].item()
        want[np.isclose(img[b, 0], 1)] = 0
        assert np.allclose(d[b], want, rtol=1e-6, atol=0)
    assert d[0, 2, 3] == 0 and d[1, 0, 0] == 0 and d[1, 7, 7] > 0 and d.shape == (2, 8, 8) and d.dtype == np.float32
    cam, M = crop_camera(prep)
    assert cam.dtype == torch.float32 and M.dtype == torch.float32 and tuple(M.shape) == (2, 2, 3) and M.is_contiguous()
    assert torch.equal(cam, prep["cam_para"]) and torch.equal(M, prep["M"][:, :2])


@pytest.mark.parametrize("size", [(128, 128), (32, 32)])
def test_fp32_render_follows_float64_on_the_surface_poses(size):
    """coverage and face identical, |d32 - d64| <= 1e-2 mm on every covered pixel -- a pixel may be left out only if its float64 decision margin (the
    smallest |w_i| / |area| of a face near it, or the relative depth gap between its two nearest faces) is under 1e-6, and at most 0.5 % of the covered
    pixels may be."""
    d32, f32 = R.rendered(size)[:2]
    d64, f64, _, _, edge, gap = R.rendered(size, "float64")
    d32, f32, d64, f64, edge, gap = (a[:3] for a in (d32, f32, d64, f64, edge, gap))  # surface_poses()
    cov = f64 >= 0
    out = np.minimum(edge, gap) < 1e-6
    worst = np.abs(d32.astype(np.float64) - d64)[cov & ~out].max()
    print("MANO-RASTER %s: covered %s, left out %d, face differs at %d, worst |d32 - d64| %.3e mm" % (
        size, cov.sum((1, 2)).tolist(), int((out & cov).sum()), int((f32 != f64).sum()), worst))
    assert int((out & (cov | (f32 >= 0))).sum()) <= 0.005 * int(cov.sum())
    assert np.array_equal((f32 >= 0)[~out], cov[~out])
    assert np.array_equal(f32[~out], f64[~out])
    assert worst <= 1e-2
    n = np.prod(size)
    assert bool((cov.sum((1, 2)) > 0.1 * n).all()) and bool((cov.sum((1, 2)) < 0.25 * n).all())  # the hand fills an eighth to a fifth of its crop


@pytest.mark.parametrize("margin", [2.0, 5.0, 10.0])
def test_fp32_occlusion_equals_float64(margin):
    v = R.hands()
    cam, M = R.crop_for(v, (128, 128))
    r32, r64 = R.rendered((128, 128)), R.rendered((128, 128), "float64")
    o32 = R.occluded_host(v, cam, M, r32[0], r32[1], margin, np.float32)
    o64 = R.occluded_host(v, cam, M, r64[0], r64[1], margin, np.float64)
    print("MANO-RASTER occluded at margin %g mm: %s" % (margin, o64.sum(1).tolist()))
    assert np.array_equal(o32, o64)
    if margin == 10.0:
        assert np.array_equal(o32, r32[2]) and np.array_equal(o64, r64[2])
    assert bool((o64.sum(1) > 100).all())  # the far side of the hand


@pytest.mark.parametrize("size", [(128, 128), (32, 32), (16, 64)])
def test_the_rendered_depth_back_projects_onto_its_face(size):
    """every covered pixel of the float64 render, back-projected from (c + 0.5, r + 0.5, depth) through inv(M) and the camera exactly as
    preprocess.depth_to_pcl does, lies in the plane of face[r, c]'s triangle within 1e-6 mm and inside it (barycentric coordinates >= -1e-9: the float64
    rounding of a point on an edge)"""
    v = R.hands().astype(np.float64)
    cam, M = R.crop_for(v, size)
    depth, face = R.rendered(size, "float64")[:2]
    f = R.surface_faces()
    worst, lowest = 0.0, 0.0
    for b in range(len(v)):
        cov = face[b] >= 0
        p = R.backproject_host(depth[b], cam[b], M[b])[cov]
        t = v[b][f[face[b][cov]]]  # [n, 3 corners, 3]
        e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        n = np.cross(e1, e2)
        n2 = (n * n).sum(-1)
        q = p - t[:, 0]
        worst = max(worst, float(np.abs((q * n).sum(-1) / np.sqrt(n2)).max()))
        b1, b2 = (np.cross(q, e2) * n).sum(-1) / n2, (np.cross(e1, q) * n).sum(-1) / n2
        lowest = min(lowest, float(np.minimum(np.minimum(b1, b2), 1 - b1 - b2).min()))
    print("MANO-RASTER back-projection %s: worst distance to the face's plane %.3e mm, lowest barycentric coordinate %.3e" % (size, worst, lowest))
    assert worst <= 1e-6 and lowest >= -1e-9


def test_two_plates():
    v, f, H, W, (depth, face, occ, stats) = R.scene_render("two_plates")
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    near, far = (c >= 10) & (c <= 20) & (r >= 10) & (r <= 20), (c >= 2) & (c <= 29) & (r >= 2) & (r <= 29)
    assert np.array_equal(face[0] >= 0, far) and np.array_equal(face[0] >= 2, near)
    assert np.allclose(depth[0][near], 400.0, rtol=1e-6) and np.allclose(depth[0][far & ~near], 500.0, rtol=1e-6) and not depth[0][~far].any()
    assert occ[0, [8, 9]].tolist() == [1, 1] and occ[0, [10, 11, 12]].tolist() == [0, 0, 0] and int(occ.sum()) == 2
    assert stats[0].tolist() == [784.0, 0.0, 0.0, 0.0]


def test_coincident_faces_give_the_lower_index():
    v, f, H, W, (depth, face, occ, stats) = R.scene_render("coincident")
    assert 1 in face and 3 in face and 0 in face and 2 not in face
    flipped = R.raster_host(v, f[[0, 2, 1, 3]], R.UNIT, None, H, W, 10.0)  # the two in the other order: the same pixels, the same depths
    assert np.array_equal(flipped[0], depth) and np.array_equal(flipped[1] == 1, face == 1)


def test_grid_aligned_mesh_loses_no_pixel_on_a_shared_edge():
    v, f, H, W, (depth, face, occ, stats) = R.scene_render("grid")
    assert bool((face[0, :13, :13] >= 0).all()) and int((face >= 0).sum()) == 169
    assert np.allclose(depth[0, :13, :13], 256.0, rtol=1e-6)
    sx, sy, _, _ = R.project_host(v[0], R.UNIT[0], None)
    assert np.array_equal(sx[:25].reshape(5, 5)[0], [0, 3, 6, 9, 12]) and np.array_equal(sy[:25].reshape(5, 5)[:, 0], [0, 3, 6, 9, 12])


def test_skipped_faces():
    v, f, H, W, (depth, face, occ, stats) = R.scene_render("skipped")
    alone = R.raster_host(v, f[:1], R.UNIT, None, H, W, 10.0)
    assert set(np.unique(face)) == {-1, 0} and np.array_equal(depth, alone[0]) and int((face == 0).sum()) == 78


def test_window():
    v, f, H, W, (depth, face, occ, stats) = R.scene_render("window")
    assert 0 in face[0, 0] and 0 in face[0, :, 0]           # face 0 reaches the top row and the left column
    assert 1 not in face                                    # face 1 is outside
    assert 2 in face and bool((face[0, :, 15] == 2).any())  # the vertex at z = 1e-3 drags face 2 to the right edge
    assert 3 not in face
    big = R.raster_host(v, f[:1], R.UNIT, None, 40, 40, 10.0)  # the same face in a larger window: the shared pixels agree
    one = R.raster_host(v, f[:1], R.UNIT, None, H, W, 10.0)
    assert np.array_equal(one[0][0], big[0][0, :16, :16]) and int((big[1] >= 0).sum()) == int((one[1] >= 0).sum())  # nothing of it lies beyond (16, 16)


def test_threshold_scene_has_boxes_on_both_sides_of_64_pixels():
    v, f, H, W, (depth, face, occ, stats) = R.scene_render("threshold")
    sx, sy, _, _ = R.project_host(v[0], R.UNIT[0], None)
    boxes = [int((sx[t].max() - sx[t].min() + 1) * (sy[t].max() - sy[t].min() + 1)) for t in f]
    assert boxes == [64, 65, 81]
    assert {0, 1, 2} <= set(np.unique(face)) and face[0, 1, 1] == 2 and face[0, 4, 4] == 0  # both pixels lie in faces 0 and 2: each wins where it is nearer


@pytest.mark.parametrize("name,F", [("one_face", 1), ("most_faces", 2048)])
def test_limits(name, F):
    v, f, H, W, (depth, face, occ, stats) = R.scene_render(name)
    assert len(f) == F and int((face >= 0).sum()) > 100 and face.max() < F
    d64, f64 = R.scene_render(name, "float64")[4][:2]
    assert np.mean(f64 == face) > 0.99 and np.abs(d64 - depth)[(f64 == face) & (face >= 0)].max() < 1e-2


def test_curled_hands_occlude_themselves():
    """the vertices that visible_host calls camera-facing and the render calls occluded (128 x 128, margin 10 mm): at least 30 on each curled hand
    (measured 87 and 52), at most 5 on each of surface_poses() (measured 0, 0, 1)"""
    v = R.hands()
    vis = S.visible_host(v, S.normals_host(v, R.surface_faces()), 0.0)
    occ = R.rendered((128, 128), "float64")[2]
    hidden = (vis & occ).sum(1)
    print("MANO-RASTER facing %s, facing and occluded %s" % (vis.sum(1).tolist(), hidden.tolist()))
    assert bool((hidden[3:] >= 30).all()) and bool((hidden[:3] <= 5).all())


def test_mask_restatement_is_the_visibility_restatement_under_a_mask():
    v = R.hands()[:1]
    n = S.normals_host(v, R.surface_faces())
    pts = S.one_sided_cloud(v, R.surface_faces(), N=64, sigma=2.0, seed=61).numpy()
    plain = S.associate_vis_host(pts, None, v, n, 400.0)
    for got in (R.associate_vis_mask_host(pts, None, v, n, None, 400.0), R.associate_vis_mask_host(pts, None, v, n, np.ones((1, 778), np.int32), 400.0)):
        for a, b in zip(got, plain):
            assert np.array_equal(a, b)
    mask = np.ones((1, 778), np.int32)
    mask[0, plain[0][0, 0]] = 0  # hide point 0's vertex: it gets another, and every idx stays unmasked
    got = R.associate_vis_mask_host(pts, None, v, n, mask, np.inf)
    assert got[0][0, 0] not in (-1, plain[0][0, 0]) and got[3][0, plain[0][0, 0]] == 0 and got[4][0, 3] == plain[4][0, 3] - 1
    none = R.associate_vis_mask_host(pts, None, v, n, np.zeros((1, 778), np.int32), np.inf)
    assert bool((none[0] == -1).all()) and none[4][0].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_reference_chain_with_and_without_the_mask_on_the_sensors_view():
    """What float64 says (reported, not a bar): the curled hands, a cloud that IS the sensor's view (1024 covered pixels of the true mesh's
    float64 render, back-projected, + 0.5 mm), joints = truth + 0.1 mm, a start 0.1 off the truth, the Adam joint stage, rounds=6, iters_cloud=2,
    metric="plane".  Mean error of all 778 vertices, measured: without the mask 1.512 / 1.712 mm, with it 1.512 / 1.724 mm -- from this start the mask
    changes nothing that matters."""
    plain, masked = R.fit_cloud_curl_reference(False), R.fit_cloud_curl_reference(True)
    print("MANO-RASTER chain, mean error of all vertices (mm): unmasked", [round(float(x), 3) for x in plain], "masked", [round(float(x), 3) for x in masked])
    assert bool(np.isfinite(plain.numpy()).all()) and bool(np.isfinite(masked.numpy()).all())
