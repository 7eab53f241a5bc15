"""Host side of the Gauss-Newton mesh fit (ABI 29): the export, the header and the binding, the entry's refusals without a launch, and what the float64
reference (tests/mano_mesh_gn_cases.py) says about the iteration -- without a vertex term it is the joint fit's reference, 8 iterations from zeros put the
mesh within 1 mm where 50 Adam iterations leave 2.6 - 4.2 mm, and six short rounds on the cloud reach the noise's floor.  No GPU."""
import ctypes as C
import os
import re

import torch

import mano_cases as M
import mano_gn_cases as G
import mano_mesh_cases as MM
import mano_mesh_gn_cases as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kpf_mano_fit_mesh_gn_f32"


def _lib():
    from keypointfusion_amd import lib as L
    return L, L.load()


def test_header_library_and_binding_agree_on_the_mesh_gn_entry():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 29 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    assert NAME in L.EXPORTS and re.search(r"\bint %s\(" % NAME, hdr) and getattr(lib, NAME)
    body = re.search(r"typedef struct kpf_mano_fit_mesh_gn_cfg \{(.*?)\} kpf_mano_fit_mesh_gn_cfg;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[21\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in L.ManoFitGnCfg._fields_] + ["lambda_verts"] == [n for n, _ in L.ManoFitMeshGnCfg._fields_]
    assert C.sizeof(L.ManoFitMeshGnCfg) == C.sizeof(L.ManoFitGnCfg) + 4
    # the arguments of kpf_mano_fit_mesh_f32, then history, jacobian and vert_jacobian, then B and the stream
    mesh, gn = L._SIGS["kpf_mano_fit_mesh_f32"], L._SIGS[NAME]
    assert len(gn) == len(mesh) + 3 and gn[:10] == mesh[:10] and gn[11:19] == mesh[11:19] and gn[-2:] == mesh[-2:]


_X = 4096  # any non-null address: a refused call reads nothing


def _cfg(L, **kw):
    v = dict(iters=8, mu=0.1, nu=1e-2, lambda_shape=1.0, lambda_pose=0.0, init_trans=1, joint_map=list(range(21)), lambda_verts=1.0)
    v.update(kw)
    v["joint_map"] = (C.c_int * 21)(*v["joint_map"])
    return L.ManoFitMeshGnCfg(**v)


def _args(config, **kw):
    a = dict(target=_X, weight=None, vt=_X, vw=_X, m=[_X] * 6, cfg=C.byref(config), state=[_X] * 3, verts=None, joints=_X, rotmat=None, residual=_X, status=_X,
             history=None, jacobian=None, vjacobian=None, B=1)
    a.update(kw)
    return [a["target"], a["weight"], a["vt"], a["vw"]] + a["m"] + [a["cfg"]] + a["state"] + [
        a["verts"], a["joints"], a["rotmat"], a["residual"], a["status"], a["history"], a["jacobian"], a["vjacobian"], a["B"], None]


def test_fit_mesh_gn_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()
    fn = getattr(lib, NAME)
    ok = _cfg(L)
    for bad in (dict(cfg=None), dict(joints=None), dict(residual=None), dict(status=None), dict(state=[_X, None, _X]), dict(B=0), dict(m=[_X] * 5 + [None]),
                dict(vt=None), dict(vw=None), dict(target=None, vt=None, vw=None), dict(vt=None, vw=None, vjacobian=_X)):
        assert fn(*_args(ok, **bad)) != 0, bad
        assert lib.kpf_last_error().decode().startswith(NAME + ": "), bad
    for cfg, word in ((_cfg(L, iters=-1), "iters"), (_cfg(L, iters=65), "iters"), (_cfg(L, joint_map=[0] + list(range(20))), "permutation"),
                      (_cfg(L, mu=-0.1), "damping"), (_cfg(L, nu=float("nan")), "damping"), (_cfg(L, mu=float("inf")), "damping"),
                      (_cfg(L, lambda_verts=-1.0), "lambda_verts"), (_cfg(L, lambda_verts=float("nan")), "lambda_verts")):
        assert fn(*_args(cfg)) != 0
        assert word in lib.kpf_last_error().decode()


def test_reference_without_a_vertex_term_is_the_joint_fits():
    c = M.fit_inputs()
    for start, iters in (("zeros", 3), ("near", 2)):
        for dt in (torch.float64, torch.float32):
            a = MG.mesh_gn_reference(dt, c.target, c.weight, None, None, c.starts[start], iters)
            b = G.gn_reference(dt, c.target, c.weight, c.starts[start], iters, jacobian=False)
            for k in ("pose_aa", "betas", "trans", "joints", "verts", "status"):
                assert torch.equal(a[k], b[k]), (start, dt, k)
            assert torch.equal(a["history"][..., 0], b["history"]) and torch.equal(a["residual"][:, :2], b["residual"])
            assert not bool(a["history"][..., 1].any()) and not bool(a["residual"][:, 2:].any())


def test_reference_puts_the_mesh_within_a_millimetre_in_eight_iterations():
    """ "both" from zeros: measured 0.47 / 0.36 / 0.29 mm after 8 iterations (31 / 31 / 24 mm before); 50 Adam iterations are asserted at 2.6 - 4.2 mm
    (test_mano_mesh_host.py), and two Gauss-Newton iterations are already below that"""
    ref = MG.mesh_gn_pair("both", "zeros", 8)[0]
    err = MM.mean_vertex_error(ref["verts"])
    h = ref["history"]
    print("MANO-MESH-GN reference vertex history (mm):", [[round(float(v), 3) for v in row] for row in h[..., 1]], "vertex error:",
          [round(float(v), 3) for v in err])
    assert ref["status"].tolist() == [0, 0, 0] and tuple(h.shape) == (3, 9, 2)
    assert bool((err <= 1.0).all())
    assert bool((h[:, 1:, 1] < h[:, :-1, 1]).all())
    assert torch.equal(ref["residual"], torch.stack([h[:, 0, 0], h[:, -1, 0], h[:, 0, 1], h[:, -1, 1]], 1))
    # a shorter run is the head of the longer one
    short = MG.mesh_gn_pair("both", "zeros", 3)[0]
    assert torch.equal(short["history"], h[:, :4])


def test_reference_statuses_and_fp32_follows_float64():
    c = M.fit_inputs()
    t, w, vt, u = MM.mesh_targets("both")
    w, u, vt = w.clone(), u.clone(), vt.clone()
    w[1] = 0.0
    u[1] = 0.0          # sample 1: both sums 0
    vt[2, 7, 1] = float("nan")  # sample 2: a vertex target under weight 1
    r = MG.mesh_gn_reference(torch.float64, t, w, vt, u, c.starts["near"], 1)
    assert r["status"].tolist() == [0, 1, 2]
    for k, s0 in zip(("pose_aa", "betas", "trans"), c.starts["near"]):
        assert torch.equal(r[k][1:], s0[1:].double()) and not torch.equal(r[k][0], s0[0].double())
    for kind in ("both", "verts"):
        ref, plain = MG.mesh_gn_pair(kind, "zeros", 8)
        for k in ("pose_aa", "betas", "trans", "verts"):
            e = float((plain[k].double() - ref[k]).abs().max())
            print("MANO-MESH-GN reference %-5s %-8s fp32 - float64 %.3e" % (kind, k, e))
            assert e < 1e-3, (kind, k, e)


def test_reference_chain_reaches_a_quarter_of_the_first_cloud_distance():
    """from "near" with the Adam joint stage, rounds=6, iters_cloud=2, gate 20 mm: measured 5.4 - 5.7 -> 0.80 - 0.83 mm, the 0.5 mm noise's own floor"""
    before, after, out = MG.fit_cloud_gn_reference(torch.float64, MM.cloud(), MM.CLOUD_START, rounds=6, iters=50, iters_cloud=2)
    print("MANO-MESH-GN reference chain (mm):", [round(float(v), 3) for v in before[:, 1]], "->", [round(float(v), 3) for v in after[:, 1]])
    assert out["status"].tolist() == [0, 0, 0]
    assert bool((torch.from_numpy(after[:, 1]) < torch.from_numpy(before[:, 1]) / 4).all())
