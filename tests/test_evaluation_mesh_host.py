"""Host side of the mesh evaluation (ABI 32: kpf_eval_mesh_f32, kpf_eval_mesh_accumulate; keypointfusion_amd/evaluation_mesh.py, the float64 yardstick;
keypointfusion_amd/evaluation_mesh_gpu.py): the yardstick on cases known by hand, the restatement of the kernel's arithmetic (tests/mesh_eval_cases.py)
against the yardstick, the refusals that need no device, the interface, and that the cases are what the GPU comparison assumes.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_eval_cases as MC
from keypointfusion_amd import evaluation_mesh as EM
from keypointfusion_amd.evaluation_mesh_gpu import DeviceMeshEvaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kpf_eval_mesh_f32", "kpf_eval_mesh_accumulate")
_X = 4096  # any non-null address: a refused call reads nothing


def test_f_score_on_three_vertices_by_hand():
    """pred -> gt distances (1, 4, 9): one of three within 2 mm, P = 1/3; gt -> pred (0, 2, 3): two within 2 mm (<= counts the 2), R = 2/3;
    F = 2 (1/3)(2/3) / 1 = 4/9.  At 0.5 mm: P = 0, R = 1/3, F = 0; below every distance: P + R == 0 and F is 0, not 0 / 0."""
    dp, dg = np.array([[1.0, 4.0, 9.0]]), np.array([[0.0, 2.0, 3.0]])
    F, P, R = EM.f_score(dp, dg, 2.0)
    assert P[0] == 1 / 3 and R[0] == 2 / 3 and abs(F[0] - 4 / 9) < 1e-15
    F, P, R = EM.f_score(dp, dg, 0.5)
    assert P[0] == 0.0 and R[0] == 1 / 3 and F[0] == 0.0
    F, P, R = EM.f_score(dp, dg + 1.0, 0.5)
    assert P[0] == 0.0 and R[0] == 0.0 and F[0] == 0.0
    F, P, R = EM.f_score(np.array([[np.nan, np.inf, 1.0]]), dg, 100.0)  # NaN and +inf never count
    assert P[0] == 1 / 3 and R[0] == 1.0
    # from positions: a on the x axis, b its copy moved by 1, 4 and 9 mm along y
    a = np.array([[[0.0, 0.0, 0.0], [100.0, 0.0, 0.0], [200.0, 0.0, 0.0]]])
    b = a + np.array([[[0.0, 1.0, 0.0], [0.0, 4.0, 0.0], [0.0, 9.0, 0.0]]])
    d_ab, i_ab = EM.nearest_vertex(a, b)
    assert np.array_equal(d_ab, [[1.0, 4.0, 9.0]]) and np.array_equal(i_ab, [[0, 1, 2]])
    out = EM.evaluate_meshes(a, b, (0.0, 10.0, 11), (2.0,))
    assert out["precision"][2.0] == 1 / 3 and out["recall"][2.0] == 1 / 3 and abs(out["f_score"][2.0] - 1 / 3) < 1e-15
    assert abs(out["mean_error"] - 14.0 / 3) < 1e-6 and out["samples"] == 1
    assert np.array_equal(out["pck_curve"] * 3, np.array([0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3], np.float64))


def test_nearest_vertex_takes_the_lowest_index_on_a_tie_and_never_a_nan():
    b = np.array([[[5.0, 0.0, 0.0], [-5.0, 0.0, 0.0], [5.0, 0.0, 0.0], [0.0, 7.0, 0.0]]])
    a = np.array([[[0.0, 0.0, 0.0], [5.0, 1.0, 0.0], [0.0, 6.0, 0.0]]])
    d, i = EM.nearest_vertex(a, b)
    assert np.array_equal(i, [[0, 0, 3]]) and np.array_equal(d, [[5.0, 1.0, 1.0]])  # (0,0,0): 0, 1 and 2 tie at 5; (5,1,0): 0 and 2 tie at 1
    bn = b.copy()
    bn[0, 0, 0] = np.nan
    d, i = EM.nearest_vertex(a, bn)
    assert np.array_equal(i, [[1, 2, 3]])  # candidate 0 is NaN: it never wins
    d, i = EM.nearest_vertex(a, np.full_like(b, np.nan))
    assert np.array_equal(i, [[-1, -1, -1]]) and np.isinf(d).all()
    rd, ri = MC._nearest(a[0], b[0])  # the restatement's scan follows the same rule
    assert np.array_equal(ri, [0, 0, 3]) and np.array_equal(rd, np.array([5.0, 1.0, 1.0], np.float32))


def test_mesh_pck_auc_from_counts_equals_the_curve_of_the_raw_errors():
    rng = np.random.default_rng(5)
    errs = np.abs(rng.normal(scale=12.0, size=(7, 50)))
    th = np.linspace(0.0, 50.0, 100)
    counts = (errs[:, :, None] <= th).sum((0, 1))
    curve, auc = EM.mesh_pck_auc_from_counts(counts, errs.size, th)
    want = np.array([np.mean((errs.reshape(-1) <= t).astype(float)) for t in th])
    np.testing.assert_allclose(curve, want, rtol=1e-15)
    np.testing.assert_allclose(auc, np.sum((want[1:] + want[:-1]) * np.diff(th) / 2.0) / 50.0, rtol=1e-14)
    assert 0.0 < auc < 1.0 and curve[-1] > 0.99
    with pytest.raises(ValueError, match="counts must be"):
        EM.mesh_pck_auc_from_counts(counts[:99], errs.size, th)


def test_tree_sum_is_the_kernels_tree():
    rng = np.random.default_rng(3)
    for V in (1, 63, 65, 256, 257, 778, 1024):
        x = rng.normal(size=V) * 10.0 ** rng.integers(-3, 4, size=V)
        part = [0.0] * 256
        for v in range(V):  # ascending v visits every thread's vertices in ascending order
            part[v % 256] = part[v % 256] + float(x[v])
        waves = []
        for w in range(4):
            lanes = part[64 * w:64 * w + 64]
            for o in (32, 16, 8, 4, 2, 1):
                lanes = [lanes[k] + lanes[k ^ o] for k in range(64)]
            waves.append(lanes[0])
        assert MC.tree_sum(x) == ((waves[0] + waves[1]) + waves[2]) + waves[3]
        assert abs(MC.tree_sum(x) - np.sum(x)) <= 1e-12 * np.abs(x).sum()


@pytest.mark.parametrize("with_origins", [False, True])
@pytest.mark.parametrize("name", MC.case_names())
def test_restatement_against_the_yardstick(name, with_origins):
    """Plain: the restatement's err, nn and nn_idx are the yardstick's bits (the same float64 expressions, rounded once).  Aligned: within the tolerance
    the GPU test holds the device to, max(1 ulp32, 1e-7 mm); indices equal wherever the yardstick's two nearest differ by more than 1e-6 mm."""
    r, y = MC.restated_of(name, with_origins, MC.TH_DECIDED), MC.yardstick_of(name, with_origins)
    assert np.array_equal(r["err"][0].view(np.int32), y["err"][0].view(np.int32))
    assert np.array_equal(r["nn"][0].view(np.int32), y["nn"][0].view(np.int32)) and np.array_equal(r["nn_idx"][0], y["nn_idx"][0])
    assert np.array_equal(r["pck_cnt"][0], y["pck_cnt"][0]) and np.array_equal(r["f_cnt"][0], y["f_cnt"][0])
    np.testing.assert_allclose(r["mean_err"][0], y["err"][0].astype(np.float64).mean(1), rtol=1e-14)
    for key in ("err", "nn"):
        ok, diff = MC.within_tolerance(r[key][1], y[key][1])
        assert ok.all(), "%s: aligned %s %.3e mm from the yardstick" % (name, key, diff.max())
    decided = y["gap"][1] > MC.DECIDED_MM
    assert np.array_equal(r["nn_idx"][1][decided], y["nn_idx"][1][decided])
    assert np.array_equal(r["pck_cnt"][1], y["pck_cnt"][1]) and np.array_equal(r["f_cnt"][1], y["f_cnt"][1])


def test_cases_are_what_the_gpu_comparison_assumes():
    """For the yardstick alone: every kind present and as described; the optimal rotation determined ((sigma2 + d sigma3) / sigma1 >= 1e-3) wherever an
    alignment exists; at most 1 % of a case's vertices undecided in their nearest vertex (gap <= 1e-6 mm); every distance that is counted more than
    1e-6 mm from every threshold of TH_DECIDED and F_TH."""
    assert tuple(k for ks in MC.BATCHES for k in ks) == MC.KINDS and all(len(ks) <= 6 for ks in MC.BATCHES)
    worst_gap, worst_margin, worst_cond = 0.0, np.inf, np.inf
    for name in MC.case_names():
        for with_origins in (False, True):
            y = MC.yardstick_of(name, with_origins)
            V = y["err"].shape[2]
            cond = y["conditioning"][np.isfinite(y["conditioning"])]
            if V >= 3:
                assert cond.size and cond.min() >= 1e-3, (name, cond)
                worst_cond = min(worst_cond, cond.min())
            undecided = (y["gap"][1] <= MC.DECIDED_MM).mean()  # the aligned pass: the plain one is compared with the restatement, bit for bit
            worst_gap = max(worst_gap, undecided)
            assert undecided <= 0.01, (name, undecided)
            assert y["margin"].min() > MC.DECIDED_MM, (name, with_origins, y["margin"])
            worst_margin = min(worst_margin, y["margin"].min())
    print("CASES mesh eval: min conditioning %.3e | undecided nearest vertices at worst %.4f %% | closest distance to a threshold %.3e mm"
          % (worst_cond, 100 * worst_gap, worst_margin))
    for i, kinds in enumerate(MC.BATCHES):
        pred, gt, _ = MC.kind_batch(i)
        y = MC.yardstick_of("kinds%d" % i, False)
        p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
        for b, kind in enumerate(kinds):
            e, pa, nn = y["err"][0, b], y["err"][1, b], y["nn"][:, :, b]
            if kind in ("noisy2", "noisy8"):
                sigma = float(kind[5:])
                assert abs(e.mean() / (sigma * 1.5958) - 1.0) < 0.1 and pa.mean() < e.mean()  # the mean norm of a 3-d Gaussian is sigma sqrt(8 / pi)
            elif kind == "similarity":
                assert pa.max() < 1e-3 < 10.0 < e.mean()
            elif kind == "mirrored":
                H = (p64[b] - p64[b].mean(0)).T @ (g64[b] - g64[b].mean(0))
                assert np.linalg.det(H) < 0 and pa.mean() > 1.0
            elif kind == "permuted":
                assert (nn[0] == 0.0).all() and e.mean() > 10.0 and np.array_equal(y["f_cnt"][0, b], np.full((2, 2), 778))
            elif kind == "shifted":
                assert np.abs(e - np.sqrt(29.0)).max() < 1e-4 and pa.max() < 1e-3  # float32 coordinates at 600 mm: 3e-5 mm of rounding
            elif kind == "equal":
                assert np.array_equal(pred[b], gt[b]) and (e == 0.0).all() and (nn[0] == 0.0).all() and pa.max() < 1e-6
            elif kind == "coincident":
                assert np.isnan(pa).all() and np.isfinite(e).all() and (y["nn_idx"][1, :, b] == -1).all() and np.isinf(nn[1]).all()
                assert not y["pck_cnt"][1, b].any() and not y["f_cnt"][1, b].any() and y["pck_cnt"][0, b].any()
            elif kind == "duplicate":
                assert np.array_equal(gt[b, MC.DUP[0]], gt[b, MC.DUP[1]])
                assert (y["nn_idx"][0, 0, b] == MC.DUP[0]).any() and not (y["nn_idx"][:, 0, b] == MC.DUP[1]).any()  # the copy never wins
    # the hands are half a metre away, so the root-relative run subtracts something: its plain errors differ from the absolute ones
    assert not np.array_equal(MC.yardstick_of("kinds0", True)["err"][0], MC.yardstick_of("kinds0", False)["err"][0])


def test_evaluate_meshes_scores_a_log_like_the_values_it_computes_itself():
    pred, gt, _ = MC.kind_batch(0)
    y = MC.yardstick_of("kinds0", False)
    th = EM.threshold_table(MC.TH_DECIDED)
    valid = np.array([1, 0, 1, 1, 1], np.uint8)
    a = EM.evaluate_meshes(pred, gt, th, MC.F_TH, valid=valid)
    b = EM.evaluate_meshes(None, None, MC.TH_DECIDED, MC.F_TH, valid=valid, logged=(y["err"], y["nn"]))
    assert a.keys() == b.keys() and a["samples"] == 4 and a["batches"] == 1
    for k in a:
        if isinstance(a[k], dict):
            assert a[k] == b[k] and set(a[k]) == set(MC.F_TH), k
        else:
            assert np.array_equal(a[k], b[k]), k
    keep = valid.astype(bool)
    np.testing.assert_allclose(a["mean_error"], y["err"][0][keep].astype(np.float64).mean(), rtol=1e-14)
    assert a["per_vertex_mean"].shape == (778,) and a["pck_curve"].shape == (100,) and 0.0 < a["pa_auc"] <= 1.0
    assert a["pa_mean_error"] < a["mean_error"] and a["pa_f_score"][5.0] >= a["f_score"][5.0]


def test_device_mesh_evaluator_refuses_bad_inputs_without_a_device():
    ev = DeviceMeshEvaluator()
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)  # noqa: E731
    ok = dict(pred_verts=f(2, 778, 3), gt_verts=f(2, 778, 3))
    call = lambda **kw: ev.update(**{**ok, **kw})  # noqa: E731
    assert ev.check_inputs(**ok) == 2 and ev.check_inputs(valid=torch.ones(2, dtype=torch.uint8), pred_origin=f(2, 3), gt_origin=f(2, 3), **ok) == 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()  # well-formed, but host tensors: evaluation_mesh.evaluate_meshes is the host path
    with pytest.raises(TypeError, match="pred_verts must be torch.float32"):
        call(pred_verts=ok["pred_verts"].double())
    with pytest.raises(TypeError, match="gt_verts must be a torch tensor"):
        call(gt_verts=np.zeros((2, 778, 3), np.float32))
    with pytest.raises(ValueError, match="V = 778 vertices"):
        call(gt_verts=f(2, 777, 3))
    with pytest.raises(ValueError, match=r"pred_verts must be \[2\]\[778\]\[3\]"):
        call(pred_verts=f(3, 778, 3))
    with pytest.raises(ValueError, match="given together"):
        call(pred_origin=f(2, 3))
    with pytest.raises(ValueError, match="gt_origin has shape"):
        call(pred_origin=f(2, 3), gt_origin=f(2, 1, 3))
    with pytest.raises(TypeError, match="pred_origin must be torch.float32"):
        call(pred_origin=f(2, 3).double(), gt_origin=f(2, 3))
    with pytest.raises(TypeError, match="valid must be torch.uint8"):
        call(valid=torch.ones(2, dtype=torch.bool))
    with pytest.raises(ValueError, match="valid has shape"):
        call(valid=torch.ones(3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(valid=torch.ones(2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        ev.summary()
    with pytest.raises(TypeError, match="expected a DeviceMeshEvaluator"):
        ev.merge(object())
    with pytest.raises(ValueError, match="differ"):
        ev.merge(DeviceMeshEvaluator(f_thresholds=(5.0,)))
    assert ev.state() is None and ev.merge(DeviceMeshEvaluator()) is ev and ev.state() is None  # nothing to add, and no device touched
    for kw, word in ((dict(verts=0), "verts = 0"), (dict(verts=1025), "verts = 1025"), (dict(thresholds=(0.0, 50.0, 257)), "thresholds"),
                     (dict(thresholds=(0.0, 50.0, 1)), "thresholds"), (dict(thresholds=(5.0, 5.0, 10)), "thresholds"), (dict(f_thresholds=()), "f_thresholds"),
                     (dict(f_thresholds=tuple(range(9))), "f_thresholds"), (dict(f_thresholds=(5.0, 5.0)), "f_thresholds"),
                     (dict(f_thresholds=(float("nan"),)), "f_thresholds")):
        with pytest.raises(ValueError, match=word):
            DeviceMeshEvaluator(**kw)


def _lib():
    from keypointfusion_amd import lib as L
    return L, L.load()


def test_header_library_and_binding_agree_on_the_mesh_entries():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 32 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    for name in NAMES:
        assert name in L.EXPORTS and re.search(r"\bint %s\(" % name, hdr) and getattr(lib, name), name
        args = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(L._SIGS[name]) == args.count(",") + 1, name  # one ctypes type per declared argument


def test_mesh_entries_refuse_bad_arguments_without_a_launch():
    """The limits of the interface (1 <= V <= 1024, 1 <= T <= 256, 1 <= Tf <= 8, both origins or neither) are checked before anything is launched: the
    pointers here are not addresses of anything."""
    L, lib = _lib()

    def mesh(po=None, go=None, T=100, Tf=2, B=1, V=778, err=_X):
        return lib.kpf_eval_mesh_f32(_X, _X, po, go, _X, T, _X, Tf, B, V, err, _X, _X, _X, _X, _X, None)

    for bad in (dict(V=0), dict(V=1025), dict(V=-1), dict(T=0), dict(T=257), dict(Tf=0), dict(Tf=9), dict(B=0), dict(po=_X), dict(go=_X), dict(err=None)):
        assert mesh(**bad) != 0
        assert lib.kpf_last_error().decode().startswith(NAMES[0] + ": "), lib.kpf_last_error()

    def acc(B=1, V=778, T=100, Tf=2, state=_X):
        return lib.kpf_eval_mesh_accumulate(_X, _X, _X, _X, None, B, V, T, Tf, _X, _X, _X, state, _X, _X, None)

    for bad in (dict(V=0), dict(V=1025), dict(T=0), dict(T=257), dict(Tf=0), dict(Tf=9), dict(B=0), dict(state=None)):
        assert acc(**bad) != 0
        assert lib.kpf_last_error().decode().startswith(NAMES[1] + ": "), lib.kpf_last_error()
