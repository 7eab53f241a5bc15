"""Host side of the mesh fit and the association (ABI 27): the references the GPU tests hold the kernels to (tests/mano_mesh_cases.py), checked against float64
and against hand-made cases, and the two entries' refusals without a launch.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import torch

import mano_cases as M
import mano_mesh_cases as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from keypointfusion_amd import lib as L
    return L, L.load()


def test_header_library_and_binding_agree_on_the_mesh_entries():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 27 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    for name in ("kpf_mano_fit_mesh_f32", "kpf_mano_assoc_f32"):
        assert name in L.EXPORTS and re.search(r"\bint %s\(" % name, hdr) and getattr(lib, name)
    # the mesh configuration is the joint fit's, field for field, plus lambda_verts -- in the header and in the binding
    assert C.sizeof(L.ManoFitMeshCfg) == C.sizeof(L.ManoFitCfg) + 4

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        return re.findall(r"(\w+)(?:\[21\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))

    assert fields("kpf_mano_fit_mesh_cfg") == fields("kpf_mano_fit_cfg") + ["lambda_verts"] == [n for n, _ in L.ManoFitMeshCfg._fields_]


_X = 4096  # any non-null address: a refused call reads nothing


def _mesh_cfg(L, **kw):
    v = dict(iters=10, lr_pose=0.02, lr_shape=0.05, lr_trans=1.0, beta1=0.9, beta2=0.999, eps=1.0, lambda_shape=1.0, lambda_pose=0.0, init_trans=1,
             joint_map=list(range(21)), lambda_verts=1.0)
    v.update(kw)
    v["joint_map"] = (C.c_int * 21)(*v["joint_map"])
    return L.ManoFitMeshCfg(**v)


def _mesh_args(config, **kw):
    a = dict(target=_X, weight=None, vt=_X, vw=_X, m=[_X] * 6, cfg=C.byref(config), state=[_X] * 3, verts=None, joints=_X, rotmat=None, residual=_X, status=_X, B=1)
    a.update(kw)
    return [a["target"], a["weight"], a["vt"], a["vw"]] + a["m"] + [a["cfg"]] + a["state"] + [a["verts"], a["joints"], a["rotmat"], a["residual"], a["status"],
                                                                                          a["B"], None]


def test_fit_mesh_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()
    ok = _mesh_cfg(L)
    for bad in (dict(cfg=None), dict(joints=None), dict(residual=None), dict(status=None), dict(state=[_X, None, _X]), dict(B=0), dict(m=[_X] * 5 + [None]),
                dict(vt=None), dict(vw=None)):  # one of the vertex pair without the other
        assert lib.kpf_mano_fit_mesh_f32(*_mesh_args(ok, **bad)) != 0, bad
        assert lib.kpf_last_error().decode().startswith("kpf_mano_fit_mesh_f32: ")
    for cfg, word in ((_mesh_cfg(L, iters=-1), "iters"), (_mesh_cfg(L, iters=1001), "iters"), (_mesh_cfg(L, joint_map=[0] + list(range(20))), "permutation"),
                      (_mesh_cfg(L, beta2=1.0), "Adam"), (_mesh_cfg(L, lambda_verts=-1.0), "lambda_verts")):
        assert lib.kpf_mano_fit_mesh_f32(*_mesh_args(cfg)) != 0
        assert word in lib.kpf_last_error().decode()


def test_assoc_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()

    def call(points=_X, pw=None, verts=_X, gate=400.0, idx=_X, vt=_X, vw=_X, stats=_X, B=1, N=16):
        return lib.kpf_mano_assoc_f32(points, pw, verts, gate, idx, vt, vw, stats, B, N, None)

    for bad, word in ((dict(points=None), "null"), (dict(verts=None), "null"), (dict(idx=None), "null"), (dict(vt=None), "null"), (dict(vw=None), "null"),
                      (dict(stats=None), "null"), (dict(B=0), "bad shape"), (dict(N=0), "bad shape"), (dict(N=4097), "bad shape"), (dict(N=-1), "bad shape"),
                      (dict(gate=-1.0), "max_dist2"), (dict(gate=float("nan")), "max_dist2")):
        assert call(**bad) != 0, bad
        msg = lib.kpf_last_error().decode()
        assert msg.startswith("kpf_mano_assoc_f32: ") and word in msg, msg


# ----------------------------------------------------------------------------------------------------------------------------------------
# associate_host
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_associate_host_picks_the_float64_nearest_vertex():
    """The cloud of the three hands against their true mesh.  A point is compared where the float64 gap between its two nearest vertices satisfies
    d2_second - d2_first > 1e-3 (1 + d2_first); on this cloud (vertex spacing 1.4 mm at the least, 0.5 mm noise) the float64 reference leaves out none, which
    is asserted, so the noise did not have to shrink."""
    pts, verts = MM.cloud().numpy(), MM.true_mesh().numpy()
    i64, first, second = MM.argmin64(pts, verts)
    clear = (second - first) > 1e-3 * (1.0 + first)
    print("MANO-ASSOC host: %d of %d points under the gap" % (int((~clear).sum()), clear.size))
    assert int((~clear).sum()) == 0  # at most 1 % may be left out; none is
    idx, vt, vw, stats = MM.associate_host(pts, None, verts, np.inf)
    assert bool((idx[clear] == i64[clear]).all())
    # every point is matched, the weights count them and the centroids are inside the noise
    assert stats[:, 0].tolist() == [pts.shape[1]] * 3 and vw.sum(1).tolist() == [pts.shape[1]] * 3
    assert float(np.abs(stats[:, 1] - np.sqrt(first).mean(1)).max()) < 1e-4
    hit = vw > 0
    assert float(np.linalg.norm(vt[hit] - verts[hit], axis=-1).max()) < 6 * MM.CLOUD_SIGMA


def test_associate_host_on_the_hand_made_cases():
    p, w, verts = MM.hand_made()
    idx, vt, vw, stats = MM.associate_host(p.numpy(), w.numpy(), verts.numpy(), 400.0)
    assert idx[0].tolist() == [5, 5, -1, -1, -1, 700, 12]  # two on one vertex, gated, NaN, weight 0, the tie's lower index, an exact hit
    P, f = p.numpy()[0], np.float32
    assert vw[0, 5] == f(4.0) and vw[0, 700] == f(1.0) and vw[0, 12] == f(1.0) and float(vw.sum()) == 6.0
    want = (f(1.0) * P[0] + f(3.0) * P[1]) / f(4.0)  # in point order: 0 + 1 p0, then + 3 p1
    assert np.array_equal(vt[0, 5], want.astype(np.float32))
    assert np.array_equal(vt[0, 700], P[5]) and np.array_equal(vt[0, 12], P[6])
    untouched = np.ones(MM.NV, bool)
    untouched[[5, 700, 12]] = False
    assert not vt[0][untouched].any() and not vw[0][untouched].any()  # 701 among them: the tie went to 700
    d = [np.sqrt(f(f(0.25) ** 2 + f(0.125) ** 2)), np.sqrt(f(f(0.125) ** 2 + f(0.25) ** 2))]
    assert stats[0, 0] == 4 and abs(float(stats[0, 1]) - float(d[0] + d[1]) / 4) < 1e-3
    # the gate's two ends: only exact hits, and no gate (the far point joins; NaN and weight 0 never do)
    idx0 = MM.associate_host(p.numpy(), w.numpy(), verts.numpy(), 0.0)
    assert idx0[0][0].tolist() == [-1, -1, -1, -1, -1, 700, 12] and idx0[3][0].tolist() == [2.0, 0.0]
    idxi = MM.associate_host(p.numpy(), w.numpy(), verts.numpy(), np.inf)[0]
    assert idxi[0, 2] >= 0 and idxi[0, 3] == -1 and idxi[0, 4] == -1


# ----------------------------------------------------------------------------------------------------------------------------------------
# fit_mesh_reference
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_fit_mesh_reference_without_vertices_is_fit_reference():
    c = M.fit_inputs()
    for dt in (torch.float64, torch.float32):
        for start, iters in (("zeros", 10), ("near", 1)):
            want = M.fit_reference(dt, c.target, c.weight, c.starts[start], iters)
            got = MM.fit_mesh_reference(dt, c.target, c.weight, None, None, c.starts[start], iters)
            for k in ("pose_aa", "betas", "trans", "joints", "verts"):
                assert torch.equal(got[k], want[k]), (dt, start, k)
            assert torch.equal(got["residual"][:, :2], want["residual"]) and not bool(got["residual"][:, 2:].any())
            assert got["status"].tolist() == [0, 0, 0]


def test_vertex_targets_lower_the_vertex_error_of_the_float64_fit():
    """zeros start, 50 iterations, the inputs of the GPU case "both": asserted on the reference; the figures are whatever it gives"""
    joints_only = M.fit_pair("zeros", 50)[0]
    for kind in ("both", "verts", "third"):
        ref, plain = MM.mesh_pair(kind, "zeros", 50)
        assert all(bool(torch.isfinite(v).all()) for v in ref.values()) and ref["status"].tolist() == [0, 0, 0]
        e0, e1 = MM.mean_vertex_error(joints_only["verts"]), MM.mean_vertex_error(ref["verts"])
        print("MANO-MESH reference %-5s mean vertex error %s -> %s mm; residual %s" % (kind, [round(float(v), 2) for v in e0], [round(float(v), 2) for v in e1],
                                                                                  ref["residual"].tolist()))
        assert bool((e1 < e0).all())
        assert bool((ref["residual"][:, 3] < ref["residual"][:, 2]).all())
        if kind == "verts":
            assert not bool(ref["residual"][:, :2].any())  # a term without weight reports 0
        e = M.fit_errors({k: v for k, v in plain.items()}, ref, plain)
        assert e["joints"][1] < 1e-2 and e["verts"][1] < 1e-2  # fp32 follows float64 here too: the 4 x e_plain bound is a tight one


def test_fit_mesh_reference_status_rules():
    c = M.fit_inputs()
    t, w, vt, u = MM.mesh_targets("both")
    w = w.clone()
    w[1] = 0.0  # joints off, vertices on: still a fit (vertex-only), no bit
    u = u.clone()
    u[2] = 0.0
    w[2] = 0.0  # both off: bit 1
    vt = vt.clone()
    vt[0, 100, 1] = float("nan")  # under weight 1: bit 2
    r = MM.fit_mesh_reference(torch.float64, t, w, vt, u, c.starts["near"], 5)
    assert r["status"].tolist() == [2, 0, 1]
    for k, s0 in zip(("pose_aa", "betas", "trans"), c.starts["near"]):
        assert torch.equal(r[k][0], s0[0].double()) and torch.equal(r[k][2], s0[2].double()) and not torch.equal(r[k][1], s0[1].double())
    assert not bool(r["residual"][2].any()) and float(r["residual"][1, 0]) == 0.0 and float(r["residual"][1, 3]) > 0.0


def test_the_cloud_pulls_the_reference_mesh_in_by_a_factor_of_two():
    """What test_mano_fit_mesh_gpu.py::test_fit_cloud_lowers_the_cloud_distance rests on: the float64 / host chain from the "near" start (why not from zeros:
    mano_mesh_cases.fit_cloud_reference) lowers the mean point-to-vertex distance by at least a factor of two, so fp32 noise cannot decide the comparison."""
    before, after, _ = MM.fit_cloud_reference(torch.float64, MM.cloud(), MM.CLOUD_START, 3, 50, 50)
    print("MANO-CLOUD reference: %s -> %s mm" % (before[:, 1].tolist(), after[:, 1].tolist()))
    assert bool((2.0 * after[:, 1] < before[:, 1]).all())
