"""Host side of the Gauss-Newton joint fit (ABI 28): the export, the header and the binding, the entry's refusals without a launch, and what the float64
reference (tests/mano_gn_cases.py) says about the iteration itself -- it falls monotonically, it passes 50 Adam iterations within 6, it needs its damping,
and fp32 follows float64.  No GPU."""
import ctypes as C
import os
import re

import torch

import mano_cases as M
import mano_gn_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from keypointfusion_amd import lib as L
    return L, L.load()


def test_header_library_and_binding_agree_on_the_gn_entry():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 28 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    assert "kpf_mano_fit_gn_f32" in L.EXPORTS and re.search(r"\bint kpf_mano_fit_gn_f32\(", hdr) and lib.kpf_mano_fit_gn_f32
    body = re.search(r"typedef struct kpf_mano_fit_gn_cfg \{(.*?)\} kpf_mano_fit_gn_cfg;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[21\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["iters", "mu", "nu", "lambda_shape", "lambda_pose", "init_trans", "joint_map"] == [n for n, _ in L.ManoFitGnCfg._fields_]
    assert C.sizeof(L.ManoFitGnCfg) == 4 * (6 + 21)
    # the arguments of kpf_mano_fit_f32, then history and jacobian, then B and the stream
    adam, gn = L._SIGS["kpf_mano_fit_f32"], L._SIGS["kpf_mano_fit_gn_f32"]
    assert len(gn) == len(adam) + 2 and gn[:8] == adam[:8] and gn[9:17] == adam[9:17] and gn[-2:] == adam[-2:]


_X = 4096  # any non-null address: a refused call reads nothing


def _cfg(L, **kw):
    v = dict(iters=8, mu=0.1, nu=1e-2, lambda_shape=1.0, lambda_pose=0.0, init_trans=1, joint_map=list(range(21)))
    v.update(kw)
    v["joint_map"] = (C.c_int * 21)(*v["joint_map"])
    return L.ManoFitGnCfg(**v)


def _args(config, **kw):
    a = dict(target=_X, weight=None, m=[_X] * 6, cfg=C.byref(config), state=[_X] * 3, verts=None, joints=_X, rotmat=None, residual=_X, status=_X, history=None,
             jacobian=None, B=1)
    a.update(kw)
    return [a["target"], a["weight"]] + a["m"] + [a["cfg"]] + a["state"] + [a["verts"], a["joints"], a["rotmat"], a["residual"], a["status"], a["history"],
                                                                           a["jacobian"], a["B"], None]


def test_fit_gn_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()
    ok = _cfg(L)
    for bad in (dict(target=None), dict(cfg=None), dict(joints=None), dict(residual=None), dict(status=None), dict(state=[_X, None, _X]), dict(B=0),
                dict(m=[_X] * 5 + [None])):
        assert lib.kpf_mano_fit_gn_f32(*_args(ok, **bad)) != 0, bad
        assert lib.kpf_last_error().decode().startswith("kpf_mano_fit_gn_f32: ")
    for cfg, word in ((_cfg(L, iters=-1), "iters"), (_cfg(L, iters=65), "iters"), (_cfg(L, joint_map=[0] + list(range(20))), "permutation"),
                      (_cfg(L, mu=-0.1), "damping"), (_cfg(L, nu=float("nan")), "damping"), (_cfg(L, mu=float("inf")), "damping")):
        assert lib.kpf_mano_fit_gn_f32(*_args(cfg)) != 0
        assert word in lib.kpf_last_error().decode()


def test_reference_falls_monotonically_and_passes_fifty_adam_iterations_within_six():
    ref = G.gn_pair("zeros", G.GN_ITERS)[0]
    h = ref["history"]
    adam = M.fit_pair("zeros", 50)[0]["residual"][:, 1]
    print("MANO-GN reference history (mm):", [[round(float(v), 3) for v in row] for row in h], "Adam after 50:", [round(float(v), 3) for v in adam])
    assert ref["status"].tolist() == [0, 0, 0] and tuple(h.shape) == (3, G.GN_ITERS + 1)
    assert bool((h[:, 1:] < h[:, :-1]).all())
    assert bool((h[:, 6] < adam).all())
    assert torch.equal(ref["residual"], torch.stack([h[:, 0], h[:, -1]], 1))


def test_reference_without_damping_does_not_improve():
    """Undamped (mu = 0 and no floor, the shape prior as it is): the documented reason for the damping.  J^T J + Lambda is singular on these inputs -- a
    finger's twist about its own axis moves no joint, and sample 1 has 57 rows for 61 unknowns -- so no entry of the history improves on the first: in this
    restatement the factorisation fails at once (bit 4) and the state never moves.  (With the floor nu = 1e-2 alone the iteration does converge on these
    inputs; DESIGN.md 4.13 has the figures.)"""
    c = M.fit_inputs()
    ref = G.gn_reference(torch.float64, c.target, c.weight, c.starts["zeros"], G.GN_ITERS, mu=0.0, nu=0.0, jacobian=False)
    h = ref["history"]
    print("MANO-GN reference mu = nu = 0 history (mm):", [[round(float(v), 3) for v in row] for row in h], "status", ref["status"].tolist())
    assert bool((h[:, 1:] >= h[:, :1]).all())


def test_fp32_reference_follows_float64():
    for start in ("zeros", "near"):
        ref, plain = G.gn_pair(start, G.GN_ITERS)
        for k in ("pose_aa", "betas", "trans"):
            e = float((plain[k].double() - ref[k]).abs().max())
            print("MANO-GN reference %-5s %-8s fp32 - float64 %.3e" % (start, k, e))
            assert e < 1e-3, (start, k, e)


def test_reference_status_and_jacobian_conventions():
    """What the GPU tests lean on: bits 1 and 2 leave the state alone; wrist-only weights give zero pose columns, an exact zero pose step with nu > 0 and a
    failed factorisation (bit 4) without any damping; the entry Jacobian's translation block is the identity."""
    c = M.fit_inputs()
    w = c.weight.clone()
    w[1] = 0.0
    y = c.target.clone()
    y[2, 5, 1] = float("nan")
    r = G.gn_reference(torch.float64, y, w, c.starts["near"], 3, jacobian=False)
    assert r["status"].tolist() == [0, 1, 2]
    for k, s0 in zip(("pose_aa", "betas", "trans"), c.starts["near"]):
        assert torch.equal(r[k][1:], s0[1:].double()) and not torch.equal(r[k][0], s0[0].double())
    t, w1, start = G.wrist_only()
    r = G.gn_reference(torch.float64, t, w1, start, G.GN_ITERS)
    assert r["status"].tolist() == [0, 0, 0] and torch.equal(r["pose_aa"], start[0].double()) and not torch.equal(r["betas"], start[1].double())
    assert not bool(r["jacobian"][:, :3, :48].any())  # the wrist's rows
    eye = torch.eye(3, dtype=torch.float64).repeat(21, 1)
    assert torch.equal(r["jacobian"][:, :, 58:], eye.expand(3, 63, 3))
    r = G.gn_reference(torch.float64, t, w1, start, G.GN_ITERS, mu=0.0, nu=0.0, lambda_shape=0.0, jacobian=False)
    assert r["status"].tolist() == [4, 4, 4]
    assert torch.equal(r["pose_aa"], start[0].double()) and torch.equal(r["betas"], start[1].double())
