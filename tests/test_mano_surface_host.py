"""Host side of the surface entries (ABI 30: kpf_mano_normals_f32, kpf_mano_assoc_vis_f32, kpf_mano_fit_mesh_gn_plane_f32): the export, the header and the
binding, the refusals without a launch, the surface model's properties, the fp32 restatements against float64, and what the CPU restatement of
fit_cloud says about point-to-plane rounds (tests/mano_surface_cases.py).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mano_cases as M
import mano_mesh_cases as MM
import mano_mesh_gn_cases as MG
import mano_surface_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kpf_mano_normals_f32", "kpf_mano_assoc_vis_f32", "kpf_mano_fit_mesh_gn_plane_f32")
_X = 4096  # any non-null address: a refused call reads nothing


def _lib():
    from keypointfusion_amd import lib as L
    return L, L.load()


def test_header_library_and_binding_agree_on_the_surface_entries():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 30 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    for name in NAMES:
        assert name in L.EXPORTS and re.search(r"\bint %s\(" % name, hdr) and getattr(lib, name), name
    # the plane entry: the mesh entry's arguments with vert_normal after vert_weight
    gn, pl = L._SIGS["kpf_mano_fit_mesh_gn_f32"], L._SIGS[NAMES[2]]
    assert len(pl) == len(gn) + 1 and pl[:4] == gn[:4] and pl[5:] == gn[4:]


def _refused(lib, name, rc):
    assert rc != 0
    assert lib.kpf_last_error().decode().startswith(name + ": "), lib.kpf_last_error()


def test_normals_refuse_bad_arguments_without_a_launch():
    L, lib = _lib()
    fn = lib.kpf_mano_normals_f32
    for args in ((_X, _X, 0, 1.0, _X, 1), (_X, _X, 2049, 1.0, _X, 1), (_X, _X, 8, 0.0, _X, 1), (_X, _X, 8, 0.5, _X, 1), (_X, _X, 8, float("nan"), _X, 1),
                 (None, _X, 8, 1.0, _X, 1), (_X, None, 8, 1.0, _X, 1), (_X, _X, 8, -1.0, None, 1), (_X, _X, 8, 1.0, _X, 0)):
        _refused(lib, NAMES[0], fn(*args, None))


def test_assoc_vis_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()
    fn = lib.kpf_mano_assoc_vis_f32

    def call(points=_X, verts=_X, normals=_X, gate=400.0, facing=0.0, idx=_X, vt=_X, vw=_X, vis=_X, stats=_X, B=1, N=16):
        return fn(points, None, verts, normals, gate, facing, idx, vt, vw, vis, stats, B, N, None)

    for bad in (dict(N=0), dict(N=4097), dict(facing=1.0), dict(facing=-0.1), dict(facing=float("nan")), dict(normals=None), dict(vis=None),
                dict(stats=None), dict(gate=-1.0), dict(gate=float("nan")), dict(B=0)):
        _refused(lib, NAMES[1], call(**bad))


def test_plane_fit_refuses_normals_without_a_vertex_term_and_names_itself():
    L, lib = _lib()
    fn = getattr(lib, NAMES[2])
    cfg = L.ManoFitMeshGnCfg(iters=2, mu=0.1, nu=1e-2, lambda_shape=1.0, lambda_pose=0.0, init_trans=1, joint_map=(C.c_int * 21)(*range(21)), lambda_verts=1.0)

    def call(target=_X, vt=_X, vw=_X, vn=_X, config=cfg, B=1):
        return fn(target, None, vt, vw, vn, *[_X] * 6, C.byref(config), _X, _X, _X, None, _X, None, _X, _X, None, None, None, B, None)

    _refused(lib, NAMES[2], call(vt=None, vw=None))            # normals without a vertex term
    _refused(lib, NAMES[2], call(vt=None, vw=None, vn=None, target=None))
    _refused(lib, NAMES[2], call(vw=None))
    _refused(lib, NAMES[2], call(B=0))
    bad = L.ManoFitMeshGnCfg(iters=65, mu=0.1, nu=1e-2, lambda_shape=1.0, lambda_pose=0.0, init_trans=1, joint_map=(C.c_int * 21)(*range(21)), lambda_verts=1.0)
    _refused(lib, NAMES[2], call(config=bad))


def test_fit_cloud_plane_needs_the_gauss_newton_rounds():
    """the check comes before anything touches the device"""
    from keypointfusion_amd.mano_fit import ManoFitter
    f = ManoFitter.__new__(ManoFitter)
    for kw in (dict(metric="plane", cloud_solver="adam"), dict(metric="plane"), dict(metric="line", cloud_solver="gn")):
        with pytest.raises(ValueError):
            f.fit_cloud(None, None, **kw)


def test_faces_are_kept_as_int32():
    from keypointfusion_amd.heads import mano_faces
    for sd, F in ((S.surface_sd(), 1552), (M.model_sd(), 1538)):
        f = mano_faces(sd, "cpu")
        assert f.dtype == torch.int32 and tuple(f.shape) == (F, 3) and f.is_contiguous()
        assert np.array_equal(f.numpy(), S.faces_of(sd))
    assert mano_faces({}, "cpu") is None
    with pytest.raises(ValueError):
        mano_faces({"mano_layer.th_faces": torch.zeros(2049, 3, dtype=torch.int64)}, "cpu")


def test_surface_model_is_closed_outward_and_hand_sized():
    m = S.surface_hand_model()
    v, f = m["v_template"], m["f"].astype(np.int64)
    assert v.shape == (778, 3) and f.shape == (1552, 3) and f.min() == 0 and f.max() == 777
    edges = {}
    for a, b, c in f:
        for e in ((a, b), (b, c), (c, a)):
            edges[e] = edges.get(e, 0) + 1
    assert all(n == 1 for n in edges.values()) and all((b, a) in edges for a, b in edges)  # every directed edge once, its reverse once
    assert S.signed_volume(v, f) > 0
    ext = (v.max(0) - v.min(0)) * 1000
    assert 60 < ext[0] < 120 and 150 < ext[1] < 220 and 20 < ext[2] < 50
    assert np.allclose(m["weights"].sum(1), 1) and np.allclose(m["J_regressor"].sum(1), 1) and m["weights"].min() >= 0
    assert list(m["kintree_table"][0][1:]) == [0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
    # the zero pose: every float64 normal points away from the centroid
    sd = S.surface_sd()
    verts = S.layer(sd, torch.float64, torch.zeros(1, 48), torch.zeros(1, 10), torch.zeros(1, 3))[0].numpy()
    n = S.normals_host(verts, f, dtype=np.float64)
    assert np.allclose(np.linalg.norm(n, axis=-1), 1)
    assert bool((((verts - verts.mean(1, keepdims=True)) * n).sum(-1) > 0).all())
    # and the template comes back from the layer
    assert np.allclose(verts[0], v * 1000, atol=1e-4)


def test_fp32_normals_follow_float64_on_the_surface_model():
    """B = 3 random poses.  Per component within 8 * 2^-24 relative to the unit normal wherever the float64 sum is longer than 1e-3 of sum |fn| over the
    vertex's corners -- and no vertex of the surface model is under that cut."""
    verts, faces = S.surface_poses().numpy(), S.faces_of(S.surface_sd())
    n32 = S.normals_host(verts, faces)
    n64, S64, mag = S.normals_host(verts, faces, dtype=np.float64, with_sums=True)
    rel = np.linalg.norm(S64, axis=-1) / mag
    print("MANO-SURFACE normals: min |S| / sum|fn| %.3f, max |n32 - n64| %.3e" % (rel.min(), np.abs(n32 - n64).max()))
    assert bool((rel > 1e-3).all())
    assert np.abs(n32.astype(np.float64) - n64).max() <= 8 * 2.0 ** -24
    assert np.array_equal(S.normals_host(verts, faces, sign=-1.0), -n32)
    # an outward normal of a mesh 600 mm in front of the camera: roughly half the vertices face it
    vis = S.visible_host(verts, n32, 0.0)
    assert bool(((vis.sum(1) > 250) & (vis.sum(1) < 530)).all())


@pytest.mark.parametrize("facing_min", [0.0, 0.5])
def test_fp32_visibility_and_argmin_follow_float64(facing_min):
    """every vertex whose float64 visibility margin (n . V + facing_min |V|) / |V| exceeds 1e-3 in size, and every point whose float64 gap between its
    two nearest visible vertices exceeds 1e-3 (1 + d2_first) (DESIGN.md 4.12's rule), is decided alike; the test cloud is drawn to leave no point out"""
    verts, faces = S.surface_poses().numpy(), S.faces_of(S.surface_sd())
    n32 = S.normals_host(verts, faces)
    vis = S.visible_host(verts, n32, facing_min)
    vis64, margin = S.visible_host(verts.astype(np.float64), n32.astype(np.float64), facing_min, np.float64, with_margin=True)
    sure = np.abs(margin) > 1e-3
    print("MANO-SURFACE visibility at facing_min %.1f: %s visible, %d of %d vertices under the margin" % (facing_min, vis.sum(1).tolist(), int((~sure).sum()), sure.size))
    assert np.array_equal(vis[sure], vis64[sure]) and int((~sure).sum()) < 0.02 * sure.size
    pts = S.decided_cloud(verts, faces, vis)
    i64, d1, d2 = S.argmin_vis64(pts, verts, vis)
    assert bool(((d2 - d1) > 1e-3 * (1.0 + d1)).all())  # none left out
    idx, vt, vw, vis2, stats = S.associate_vis_host(pts, None, verts, n32, 400.0, facing_min)
    assert np.array_equal(vis2, vis)
    matched = idx >= 0
    assert np.array_equal(idx[matched], i64[matched]) and bool((d1[~matched] > 400.0 * (1 - 1e-3)).all())
    assert bool((vis[np.arange(3)[:, None], np.where(matched, idx, 0)][matched] == 1).all())
    assert bool((stats[:, 0] > 900).all()) and bool((stats[:, 2] <= stats[:, 1]).all()) and np.array_equal(stats[:, 3], vis.sum(1).astype(np.float32))


def test_plane_reference_without_normals_is_the_mesh_reference():
    c = M.fit_inputs()
    t, w, vt, u = MM.mesh_targets("both")
    for dt in (torch.float64, torch.float32):
        a = S.fit_mesh_gn_plane_reference(dt, t, w, vt, u, None, c.starts["near"], 2)
        b = MG.mesh_gn_reference(dt, t, w, vt, u, c.starts["near"], 2)
        assert set(a) == set(b)
        for k in b:
            assert torch.equal(a[k], b[k]), (dt, k)
    # the restatement for any model, on the synthetic hand without normals, follows it (another Jacobian call: not the bits)
    r = S.fit_mesh_gn_plane_reference(torch.float64, t, w, vt, u, None, c.starts["near"], 2, sd=M.model_sd())
    for k in ("pose_aa", "betas", "trans", "verts", "history", "residual"):
        assert float((r[k] - b[k].double()).abs().max()) < 1e-3, k


def test_plane_reference_statuses_and_rows():
    c = M.fit_inputs()
    t, w, vt, u = MM.mesh_targets("both")
    n = S.plane_normals("near").clone()
    n[1, 7, 2] = float("nan")
    u = u.clone()
    u[2, 9] = 0.0
    n[2, 9] = float("nan")  # under weight 0: selected out
    r = S.fit_mesh_gn_plane_reference(torch.float64, t, w, vt, u, n, c.starts["near"], 1)
    assert r["status"].tolist() == [0, 2, 0]
    assert torch.equal(r["pose_aa"][1], c.starts["near"][0][1].double()) and bool(torch.isfinite(r["verts"]).all())
    # the distance along the normal is no longer than the distance
    p = S.fit_mesh_gn_plane_reference(torch.float64, t, w, vt, torch.ones(3, 778), S.plane_normals("near"), c.starts["near"], 0)
    q = MG.mesh_gn_reference(torch.float64, t, w, vt, torch.ones(3, 778), c.starts["near"], 0)
    assert bool((p["residual"][:, 2] <= q["residual"][:, 2]).all()) and torch.equal(p["residual"][:, :2], q["residual"][:, :2])


def test_reference_chain_point_against_plane_on_a_one_sided_cloud():
    """The convergence finding on the CPU restatement chain (float64): the surface model, B = 3, 1024 points inside the camera-facing faces of the true mesh
    + 0.5 mm, joints = truth + 0.1 mm, the "near" start, gate 20 mm, the Adam joint stage, rounds=6, iters_cloud=2, cloud_solver="gn".  Mean error of ALL 778
    vertices against the true mesh, measured: point 3.44 / 2.73 / 2.92 mm, plane 1.99 / 2.39 / 1.82 mm."""
    point = S.mean_error_all_vertices(S.fit_cloud_surface_reference(torch.float64, "point"))
    plane = S.mean_error_all_vertices(S.fit_cloud_surface_reference(torch.float64, "plane"))
    print("MANO-SURFACE chain, mean error of all vertices (mm): point", [round(float(x), 3) for x in point], "plane", [round(float(x), 3) for x in plane])
    assert bool(torch.isfinite(point).all()) and bool(torch.isfinite(plane).all())
    assert bool((plane < point).all())
