"""Host side of the MANO backward and fit entries (ABI 26): interface agreement, argument refusals without a launch, and the CPU facts the GPU tests rest on
(tests/mano_cases.py).  No GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import mano_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from keypointfusion_amd import lib as L
    return L, L.load()


def test_header_library_and_binding_agree_on_the_mano_entries():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 26 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    for name in ("kpf_mano_backward_f32", "kpf_mano_fit_f32"):
        assert name in L.EXPORTS and re.search(r"\bint %s\(" % name, hdr) and getattr(lib, name)
    # the binding's structure is the header's: an int, eight floats, an int, 21 ints
    assert C.sizeof(L.ManoFitCfg) == 4 * (1 + 8 + 1 + 21)
    fields = re.search(r"typedef struct kpf_mano_fit_cfg \{(.*?)\} kpf_mano_fit_cfg;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[21\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [n for n, _ in L.ManoFitCfg._fields_]


_X = 4096  # any non-null address: a refused call reads nothing


def _backward_args(**kw):
    a = dict(pose6d=_X, ld6=96, betas=_X, ldb=10, m=[_X] * 6, grads=[None] * 4, d6=_X, ldd6=96, db=_X, lddb=10, B=1)
    a.update(kw)
    return [a["pose6d"], a["ld6"], a["betas"], a["ldb"]] + a["m"] + a["grads"] + [a["d6"], a["ldd6"], a["db"], a["lddb"], a["B"], None]


@pytest.mark.parametrize("bad", [dict(pose6d=None), dict(betas=None), dict(d6=None), dict(db=None)] + [dict(m=[_X] * i + [None] + [_X] * (5 - i)) for i in range(6)] +
                         [dict(B=0), dict(B=-3), dict(ld6=95), dict(ldb=9), dict(ldd6=95), dict(lddb=9)])
def test_backward_refuses_bad_arguments_without_a_launch(bad):
    L, lib = _lib()
    assert lib.kpf_mano_backward_f32(*_backward_args(**bad)) != 0
    msg = lib.kpf_last_error().decode()
    assert msg.startswith("kpf_mano_backward_f32: ") and ("null pointer" in msg or "bad shape" in msg), msg


def _fit_args(config, **kw):
    a = dict(target=_X, weight=None, m=[_X] * 6, cfg=C.byref(config), state=[_X] * 3, verts=None, joints=_X, rotmat=None, residual=_X, status=_X, B=1)
    a.update(kw)
    return [a["target"], a["weight"]] + a["m"] + [a["cfg"]] + a["state"] + [a["verts"], a["joints"], a["rotmat"], a["residual"], a["status"], a["B"], None]


def _cfg(L, **kw):
    v = dict(iters=10, lr_pose=0.02, lr_shape=0.05, lr_trans=1.0, beta1=0.9, beta2=0.999, eps=1.0, lambda_shape=1.0, lambda_pose=0.0, init_trans=1,
             joint_map=list(range(21)))
    v.update(kw)
    v["joint_map"] = (C.c_int * 21)(*v["joint_map"])
    return L.ManoFitCfg(**v)


def test_fit_refuses_bad_arguments_without_a_launch():
    L, lib = _lib()
    ok = _cfg(L)
    for bad in (dict(target=None), dict(cfg=None), dict(joints=None), dict(residual=None), dict(status=None), dict(state=[_X, None, _X]), dict(B=0),
                dict(m=[_X] * 5 + [None])):
        assert lib.kpf_mano_fit_f32(*_fit_args(ok, **bad)) != 0, bad
        assert lib.kpf_last_error().decode().startswith("kpf_mano_fit_f32: ")
    for cfg, word in ((_cfg(L, iters=-1), "iters"), (_cfg(L, iters=1001), "iters"), (_cfg(L, joint_map=[0] + list(range(20))), "permutation"),
                      (_cfg(L, joint_map=list(range(20)) + [21]), "joint_map"), (_cfg(L, beta2=1.0), "Adam")):
        assert lib.kpf_mano_fit_f32(*_fit_args(cfg)) != 0
        assert word in lib.kpf_last_error().decode()


def test_grad_case_takes_every_quaternion_branch_and_has_a_finite_reference():
    c = M.grad_case()
    counts = M.branch_counts(c.pose6d)
    print("MANO grad_case quaternion branches", counts)
    assert sum(counts) == 80 and min(counts) >= 8, counts
    for r in list(c.ref) + [g for pair in c.single.values() for g in pair[0]]:
        assert bool(torch.isfinite(r).all())
    assert all(float(r.abs().max()) > 0 for r in list(c.ref) + [pair[0][0] for pair in c.single.values()])
    e = M.errors(c, c.plain[0], c.plain[1])
    print("MANO grad_case e_plain d_pose6d %.3e d_betas %.3e" % (e["d_pose6d"][1], e["d_betas"][1]))
    assert e["d_pose6d"][1] < 1e-5 and e["d_betas"][1] < 1e-5  # the restatement is well conditioned in fp32 on these inputs: the 4 x e_plain bound is a tight one


def test_identity_reference_is_finite_and_its_forward_is_the_oracles():
    c = M.identity_case()
    sd = M._cast(M.model_sd(), torch.float64)
    for a, b in zip(M.head_tail(sd, c.pose6d.double(), c.betas.double(), safe=True), M.head_tail(sd, c.pose6d.double(), c.betas.double(), safe=False)):
        assert torch.equal(a, b)
    assert all(bool(torch.isfinite(r).all()) for r in c.ref)
    assert float(c.ref[0][0].abs().max()) > 0  # the identity sample does receive a gradient
    plain_nan = M.gradients(c.pose6d, c.betas, c.projs, torch.float64, safe=False)[0]
    assert not bool(torch.isfinite(plain_nan[0]).all())  # the deviation DESIGN 4.11 states: autograd of the reference formula is NaN at identity


@pytest.mark.parametrize("iters", [10, 50])
def test_fit_reference_converges_and_fp32_follows_float64(iters):
    ref, plain = M.fit_pair("zeros", iters)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    assert bool((ref["residual"][:, 1] < ref["residual"][:, 0]).all()) and bool((plain["residual"][:, 1] < plain["residual"][:, 0]).all())
    e = M.fit_errors({k: v for k, v in plain.items()}, ref, plain)
    print("MANO fit_reference iters %d residual %s -> %s mm; e_plain %s" % (iters, ref["residual"][:, 0].tolist(), ref["residual"][:, 1].tolist(),
                                                                              {k: "%.2e" % v[1] for k, v in e.items()}))
    assert e["joints"][1] < 1e-2 and e["verts"][1] < 1e-2  # eps = 1.0 keeps fp32 and float64 on one trajectory (with 1e-8 they part by millimetres)
