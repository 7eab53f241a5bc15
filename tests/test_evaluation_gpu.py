"""Device-resident evaluation (keypointfusion_amd/evaluation_gpu.py, kpf_eval_* of include/kpf.h) against its yardsticks: float64 numpy for the per-sample
errors (`evaluation.rigid_align`, pinned to the reference's own code by tests/golden/metrics.npz), a sequential float64 Python loop for the sums, numpy
comparisons for the PCK counts, `evaluation.pck_auc` / `evaluation.evaluate_batch` for the summary.  Inputs: tests/eval_cases.py.

The per-sample comparison prints one "ERR ..." line per batch size before it asserts (`-s` shows them; profiles/eval_kernel_errors.txt is where a run is kept)."""
import os

import numpy as np
import pytest
import torch

import eval_cases as EC
from conftest import GOLDEN, synthetic_sd
from keypointfusion_amd import evaluation as EV
from keypointfusion_amd.evaluation_gpu import DeviceEvaluator

S6 = (3, 3, 3, 3, 3, 3)  # six stages that already hold xyz joints


# ---------------------------------------------------------------------------------------------------------------- host
def test_pck_auc_from_counts_equals_pck_auc_on_the_reference_fixture():
    z = np.load(os.path.join(GOLDEN, "metrics.npz"))
    errs, th = z["errs"], np.linspace(0.0, 50.0, 20)
    counts = (errs[:, :, None] <= th[None, None, :]).sum(1)
    assert counts.shape == (21, 20) and counts.dtype.kind == "i"
    auc, curve, th2, sub = EV.pck_auc_from_counts(counts, errs.shape[1], th)
    want = EV.pck_auc([list(r) for r in errs], 0.0, 50.0, 20)
    for got, ref in ((auc, want[0]), (curve, want[1]), (th2, want[2]), (sub, want[3]), (auc, float(z["auc"])), (curve, z["curve"]), (sub, float(z["sub"]))):
        np.testing.assert_allclose(got, ref, rtol=1e-12)
    with pytest.raises(ValueError, match="counts must be"):
        EV.pck_auc_from_counts(counts[:, :19], errs.shape[1], th)


def _host_batch(B=2, J=21):
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return dict(results=[f(B, 105, 16, 16), f(B, 105, 16, 16)] + [f(B, J, 3) for _ in range(4)], img=f(B, 1, 128, 128), xyz_gt=f(B, J, 3), center=f(B, 3),
                M=f(B, 3, 3), cube=f(B, 3), cam_para=f(B, 4))


def test_device_evaluator_refuses_bad_inputs_without_a_device():
    ev = DeviceEvaluator()
    ok = _host_batch()
    call = lambda **kw: ev.update(**{**ok, **kw})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()  # well-formed, but host tensors: evaluation.evaluate_batch is the host-driven path
    with pytest.raises(TypeError, match="xyz_gt must be torch.float32"):
        call(xyz_gt=ok["xyz_gt"].double())
    with pytest.raises(TypeError, match=r"results\[3\] must be torch.float32"):
        call(results=ok["results"][:3] + [ok["results"][3].half()] + ok["results"][4:])
    with pytest.raises(TypeError, match="cube must be a torch tensor"):
        call(cube=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="list of 6 stage outputs"):
        call(results=ok["results"][:5])
    with pytest.raises(ValueError, match="J = 21 joints"):
        call(xyz_gt=torch.zeros(2, 23, 3))
    with pytest.raises(ValueError, match=r"results\[5\].*J = 21 joints"):
        call(results=ok["results"][:5] + [torch.zeros(2, 23, 3)])
    with pytest.raises(ValueError, match=r"results\[0\] \(stage type 1\)"):
        call(results=[torch.zeros(2, 21, 3)] + ok["results"][1:])
    with pytest.raises(ValueError, match="M has shape"):
        call(M=torch.zeros(2, 9))
    with pytest.raises(TypeError, match="valid must be torch.uint8"):
        call(valid=torch.ones(2, dtype=torch.bool))
    with pytest.raises(TypeError, match="valid must be torch.uint8"):
        call(valid=torch.ones(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="valid has shape"):
        call(valid=torch.ones(3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(valid=torch.ones(2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        ev.summary()
    # stages that hold xyz need no image, centre, crop matrix or camera
    ev3 = DeviceEvaluator(stage_type=S6, joints=23, score_joints=EV.NYU_SCORED_JOINTS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev3.update([torch.zeros(2, 23, 3)] * 6, None, torch.zeros(2, 23, 3), None, None, torch.zeros(2, 3), None)
    for kw, word in ((dict(stage_type=(1,) * 9), "stages"), (dict(stage_type=(1, 4)), "stage types"), (dict(joints=65, stage_type=S6), "joints = 65"),
                     (dict(joints=23), "dense stages decode 21"), (dict(score_joints=(0, 21)), "score_joints"), (dict(thresholds=(0.0, 50.0, 9)), "thresholds")):
        with pytest.raises(ValueError, match=word):
            DeviceEvaluator(**kw)


def test_cases_are_of_the_six_kinds_and_well_conditioned():
    """The inputs of the GPU comparison are what its bounds assume: six kinds in every batch of 32, the optimal rotation of every sample determined
    ((sigma2 + d sigma3) / sigma1 >= 1e-3, so that two correct SVDs must agree), reflections and rank-2 covariances present."""
    gt, pred, cube, kinds = EC.make_batch(32, seed=7)
    assert set(kinds) == set(EC.KINDS) and kinds[:6] == list(EC.KINDS)
    assert EC.conditioning(pred, gt).min() >= 1e-3
    A0, B0 = pred.astype(np.float64) - pred.astype(np.float64).mean(1, keepdims=True), gt.astype(np.float64) - gt.astype(np.float64).mean(1, keepdims=True)
    H = np.einsum("bji,bjk->bik", A0, B0) / 21
    assert all(np.linalg.det(H[b]) < 0 for b in range(32) if kinds[b] == "mirrored")
    assert all(np.linalg.svd(H[b])[1][2] < 1e-9 for b in range(32) if kinds[b] == "planar")
    assert all(np.array_equal(pred[b], gt[b]) for b in range(32) if kinds[b] == "equal")
    plain, pa = EC.yardstick(pred, gt, cube)
    assert all(pa[b].max() < 1e-4 < plain[b].min() for b in range(32) if kinds[b] == "similarity")


# ----------------------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stages(pred, gt, S=6):
    """S stage tensors: stage s is the prediction pulled towards the ground truth by s / (2 S) (so that the stages differ), the last one the prediction itself."""
    out = []
    for s in range(S):
        w = np.float32((S - 1 - s) / (2.0 * S))
        out.append((pred * (1 - w) + gt * w).astype(np.float32) if s < S - 1 else pred.copy())
    return out


def _update3(ev, stages, gt, cube, valid=None):
    e, p = ev.update([_dev(s) for s in stages], None, _dev(gt), None, None, _dev(cube), None, None if valid is None else _dev(np.asarray(valid, np.uint8)))
    return e.cpu().numpy().copy(), p.cpu().numpy().copy()


_REF = {}


def _case(B, seed=7):
    """One batch, its stages and the float64 yardstick, computed once per (B, seed)."""
    if (B, seed) not in _REF:
        gt, pred, cube, kinds = EC.make_batch(B, seed=seed)
        stages = _stages(pred, gt)
        want = [EC.yardstick(s, gt, cube) for s in stages]
        _REF[(B, seed)] = (gt, pred, cube, kinds, stages, want)
    return _REF[(B, seed)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 32])
def test_per_sample_errors_against_float64(B):
    """Plain errors within 1 float32 ulp of the float64 yardstick (double rounding), aligned errors within max(1 ulp, 1e-7 mm) (the floor: samples whose
    aligned error is rounding residue).  The kernel's alignment code compiled for the host gives, on these inputs, float32 results bit-equal to the yardstick
    (<= 3.2e-12 mm apart on the rounding-residue kinds); no figures from the MI355X have been recorded yet."""
    gt, pred, cube, kinds, stages, want = _case(B if B > 3 else 6)  # B = 1, 3: every kind is still covered, as the leading samples of successive batches
    ev = DeviceEvaluator(stage_type=S6)
    n = 6 if B <= 3 else B
    worst_plain = worst_pa_ulp = worst_pa_abs = 0.0
    cond_min = np.inf
    for lo in range(0, n, B):
        sl = slice(lo, lo + B)
        e, p = _update3(ev, [s[sl] for s in stages], gt[sl], cube[sl])
        assert e.shape == p.shape == (6, B, 21) and e.dtype == np.float32
        for s in range(6):
            cond = EC.conditioning(stages[s][sl], gt[sl])
            cond_min = min(cond_min, cond.min())
            assert cond.min() >= 1e-3, "stage %d: the optimal rotation of a sample is not determined; two correct SVDs need not agree" % s
            yp, ya = want[s][0][sl], want[s][1][sl]
            dp = np.abs(e[s].astype(np.float64) - yp) / EC.ulp32(yp)
            da = np.abs(p[s].astype(np.float64) - ya)
            worst_plain, worst_pa_abs = max(worst_plain, dp.max()), max(worst_pa_abs, da.max())
            worst_pa_ulp = max(worst_pa_ulp, (da / EC.ulp32(ya))[ya > 1e-3].max(initial=0.0))
            assert np.isfinite(e[s]).all() and np.isfinite(p[s]).all()
            assert (dp <= 1.0).all(), "stage %d plain error %.3g ulp from float64" % (s, dp.max())
            assert (da <= np.maximum(EC.ulp32(ya), 1e-7)).all(), "stage %d aligned error %.3g mm from float64" % (s, da.max())
        for b in range(lo, min(lo + B, n)):
            if kinds[b] == "equal":
                assert (e[5][b - lo] == 0.0).all()  # pred == gt bit for bit: exactly zero
    print("ERR eval B=%d plain max %.3f ulp | aligned max %.3f ulp (errors > 1e-3 mm), max %.3e mm overall | min (s2 + d s3) / s1 %.3e"
          % (B, worst_plain, worst_pa_ulp, worst_pa_abs, cond_min))


def _sequential_state(logs, valids, th, S, Jq):
    """The state after the batches `logs` = [(err [S][B][Jq], pa [S][B][Jq]) float32], in the order include/kpf.h states, in Python floats (float64)."""
    T = len(th)
    st = dict(n_samples=0, n_batches=0, sum_err=np.zeros((S, Jq)), sum_pa=np.zeros((S, Jq)), sum_batch_mean=np.zeros(S), sum_batch_pa_mean=np.zeros(S),
              pck=np.zeros((S, Jq, T), np.int64), pck_pa=np.zeros((S, Jq, T), np.int64))
    for (e, p), valid in zip(logs, valids):
        keep = [b for b in range(e.shape[1]) if valid is None or valid[b]]
        if not keep:
            continue
        st["n_samples"] += len(keep)
        st["n_batches"] += 1
        for arr, ksum, kmean, kpck in ((e, "sum_err", "sum_batch_mean", "pck"), (p, "sum_pa", "sum_batch_pa_mean", "pck_pa")):
            for s in range(S):
                acc = 0.0
                for b in keep:
                    for j in range(Jq):
                        x = float(arr[s, b, j])
                        st[ksum][s, j] = float(st[ksum][s, j]) + x
                        acc = acc + x
                st[kmean][s] = float(st[kmean][s]) + acc / float(len(keep) * Jq)
                st[kpck][s] += (arr[s][keep].astype(np.float64)[:, :, None] <= th[None, None, :]).sum(0)
    return st


def _assert_state(ev, want):
    got = {k: v.cpu().numpy() for k, v in ev.state().items()}
    assert int(got["n_samples"][0]) == want["n_samples"] and int(got["n_batches"][0]) == want["n_batches"]
    for k in ("sum_err", "sum_pa", "sum_batch_mean", "sum_batch_pa_mean"):
        assert got[k].dtype == np.float64 and np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k  # bit-equal
    for k in ("pck", "pck_pa"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    return got


@pytest.mark.gpu
def test_accumulation_is_exact_and_summary_matches_pck_auc():
    gt, pred, cube, kinds, stages, _ = _case(12, seed=11)
    assert kinds[4] == "equal"
    valids = [None, None, [1, 1, 0, 0]]
    ev = DeviceEvaluator(stage_type=S6)
    logs = [_update3(ev, [s[4 * i:4 * i + 4] for s in stages], gt[4 * i:4 * i + 4], cube[4 * i:4 * i + 4], valids[i]) for i in range(3)]
    want = _sequential_state(logs, valids, ev.thresholds, 6, 21)
    assert want["n_samples"] == 10 and want["n_batches"] == 3
    got = _assert_state(ev, want)
    assert (got["pck"][5, :, 0] >= 1).all()  # the pred == gt sample (batch 1, row 0) has error 0.0 <= threshold 0.0
    assert got["pck"].max() <= 10 and got["pck_pa"].max() <= 10
    # summary against pck_auc on the concatenated per-joint lists, and both mean conventions against their formulas
    summ = ev.summary()
    assert len(summ) == 6
    keep = [(i, b) for i in range(3) for b in range(4) if valids[i] is None or valids[i][b]]
    for s in range(6):
        for which, pre in ((0, ""), (1, "pa_")):
            rows = np.array([logs[i][which][s, b] for i, b in keep])  # [10][21] float32
            auc, curve, th, sub = EV.pck_auc([list(rows[:, j]) for j in range(21)], 0.0, 50.0, 20)
            np.testing.assert_allclose(summ[s][pre + "auc"], auc, rtol=1e-12)
            np.testing.assert_allclose(summ[s][pre + "pck_curve"], curve, rtol=1e-12)
            np.testing.assert_allclose(summ[s][pre + "auc_20_50"], sub, rtol=1e-12)
            np.testing.assert_allclose(summ[s][pre + "mean_error"], rows.astype(np.float64).mean(), rtol=1e-12)
            np.testing.assert_allclose(summ[s][pre + "per_joint_mean"], rows.astype(np.float64).mean(0), rtol=1e-12)
            bm = [np.mean([logs[i][which][s, b].astype(np.float64) for b in range(4) if valids[i] is None or valids[i][b]]) for i in range(3)]
            np.testing.assert_allclose(summ[s][pre + "mean_error_of_batch_means"], np.mean(bm), rtol=1e-12)
        assert summ[s]["samples"] == 10 and summ[s]["batches"] == 3
    # a batch without a valid sample adds nothing and is not counted
    _update3(ev, [s[:4] for s in stages], gt[:4], cube[:4], [0, 0, 0, 0])
    _assert_state(ev, want)
    # merge: two evaluators that saw batches {0, 1} and {2}
    a, b = DeviceEvaluator(stage_type=S6), DeviceEvaluator(stage_type=S6)
    for i, part in ((0, a), (1, a), (2, b)):
        _update3(part, [s[4 * i:4 * i + 4] for s in stages], gt[4 * i:4 * i + 4], cube[4 * i:4 * i + 4], valids[i])
    pa_, pb_ = ({k: v.cpu().numpy().copy() for k, v in part.state().items()} for part in (a, b))
    a.merge(b)
    m = {k: v.cpu().numpy() for k, v in a.state().items()}
    for k in ("n_samples", "n_batches", "pck", "pck_pa"):
        assert np.array_equal(m[k], got[k]), k
    for k in ("sum_err", "sum_pa", "sum_batch_mean", "sum_batch_pa_mean"):
        assert np.array_equal(m[k], pa_[k] + pb_[k]), k
        np.testing.assert_allclose(m[k], got[k], rtol=1e-14)
    with pytest.raises(ValueError, match="differ"):
        a.merge(DeviceEvaluator(stage_type=S6, thresholds=(0.0, 40.0, 20)))
    # reset
    ev.reset()
    assert all(int(v.abs().sum()) == 0 for k, v in ev.state().items() if k.startswith(("n_", "pck"))) and float(ev.state()["sum_err"].abs().sum()) == 0.0


@pytest.mark.gpu
def test_update_is_capturable_and_replay_equals_eager():
    """A successful capture is also the check that update() neither synchronises nor allocates."""
    gt, pred, cube, kinds, stages, _ = _case(12, seed=11)
    batches = [([s[4 * i:4 * i + 4] for s in stages], gt[4 * i:4 * i + 4], cube[4 * i:4 * i + 4]) for i in range(3)]
    valid = _dev(np.array([1, 1, 1, 0], np.uint8))
    eager = DeviceEvaluator(stage_type=S6)
    for st, g, c in batches:
        eager.update([_dev(s) for s in st], None, _dev(g), None, None, _dev(c), None, valid)
    want = {k: v.cpu().numpy().copy() for k, v in eager.state().items()}

    ev = DeviceEvaluator(stage_type=S6)
    s_st, s_gt, s_cube = [_dev(s) for s in batches[0][0]], _dev(batches[0][1]), _dev(batches[0][2])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.update(s_st, None, s_gt, None, None, s_cube, None, valid)  # eager warm-up: buffers, state and library are in place
        ev.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e, p = ev.update(s_st, None, s_gt, None, None, s_cube, None, valid)
    ev.reset()  # (whatever the capture itself left)
    for st, g, c in batches:
        for dst, src in zip(s_st + [s_gt, s_cube], st + [g, c]):
            dst.copy_(_dev(src))
        graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in ev.state().items()}
    assert int(got["n_samples"][0]) == 9 and int(got["n_batches"][0]) == 3
    for k in want:
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k
    le, lp = eager.update([_dev(s) for s in batches[2][0]], None, _dev(batches[2][1]), None, None, _dev(batches[2][2]), None, valid)
    assert torch.equal(e, le) and torch.equal(p, lp)  # the replay's log of the last batch


@pytest.mark.gpu
def test_end_to_end_with_the_decode_matches_evaluate_batch():
    """As tests/test_evaluation.py::test_decode_and_evaluate_batch_on_device: the oracle's results of the synthetic ConvNeXt-tiny batch, the real STAGE_TYPE."""
    from oracle import kpf_oracle as O
    from keypointfusion_amd.weights import synthetic_batch
    dev = torch.device(DEV)
    sd = synthetic_sd("KPFusion-convnext-tiny")
    b = {k: torch.from_numpy(v) for k, v in synthetic_batch(2, 128, seed=9).items()}
    ref, _ = O.kpfusion_forward(sd, b["img_rgb"], b["img"], b["pcl"], b["center"], b["M"], b["cube"], b["cam_para"], 0.8)
    d = {k: v.to(dev) for k, v in b.items()}
    res = [r.to(dev).contiguous() for r in ref]
    gt = (ref[5] + 0.01).to(dev)
    want = EV.evaluate_batch(res, d["img"], gt, d["center"], d["M"], d["cube"], d["cam_para"])
    ev = DeviceEvaluator()
    e, p = ev.update(res, d["img"], gt, d["center"], d["M"], d["cube"], d["cam_para"])
    assert e.shape == (6, 2, 21)
    summ = ev.summary()
    for s in range(6):
        assert np.abs(e[s].cpu().numpy() - want[s]["joint_errors"]).max() < 1e-3
        assert abs(summ[s]["mean_error"] - want[s]["mean_error"]) < 1e-3
        assert abs(summ[s]["pa_mean_error"] - want[s]["pa_mean_error"]) < 1e-3
        assert abs(summ[s]["mean_error_of_batch_means"] - want[s]["mean_error"]) < 1e-3  # one batch: the two conventions coincide
    assert abs(summ[5]["mean_error"] - 0.01 * 125.0 * 3 ** 0.5) < 1e-3 and summ[5]["pa_mean_error"] < 1e-3


@pytest.mark.gpu
def test_nyu_selection_scores_14_of_23_joints_and_aligns_on_all_23():
    z = np.load(os.path.join(GOLDEN, "metrics_xyz2error.npz"))
    pred, gt, cube = z["pred23"], z["gt23"], z["cube23"]
    ev = DeviceEvaluator(stage_type=(3,), joints=23, score_joints=EV.NYU_SCORED_JOINTS)
    e, p = ev.update([_dev(pred)], None, _dev(gt), None, None, _dev(cube), None)
    e, p = e.cpu().numpy(), p.cpu().numpy()
    assert e.shape == p.shape == (1, 5, 14)
    np.testing.assert_allclose(e[0], z["err23"], rtol=0, atol=2e-3)  # mm; the reference adds a ~600 mm centre to both sides in fp32 first
    sel = list(EV.NYU_SCORED_JOINTS)
    plain, pa = EC.yardstick(pred, gt, cube)  # aligned on all 23 joints, then the selection
    assert EC.conditioning(pred, gt).min() >= 1e-3
    assert (np.abs(e[0].astype(np.float64) - plain[:, sel]) <= EC.ulp32(plain[:, sel])).all()
    assert (np.abs(p[0].astype(np.float64) - pa[:, sel]) <= np.maximum(EC.ulp32(pa[:, sel]), 1e-7)).all()
    pa14 = EC.yardstick(pred[:, sel], gt[:, sel], cube)[1]  # aligning on the 14 scored joints alone gives another answer: the test can tell the two apart
    assert np.abs(pa14 - pa[:, sel]).max() > 1e-2
    assert ev.summary()[0]["per_joint_mean"].shape == (14,)


@pytest.mark.gpu
def test_a_samples_errors_do_not_depend_on_the_batch():
    gt, pred, cube, kinds, stages, _ = _case(32)
    e32, p32 = _update3(DeviceEvaluator(stage_type=S6), stages, gt, cube)
    for b in (0, 1):  # a noisy and a mirrored sample
        e1, p1 = _update3(DeviceEvaluator(stage_type=S6), [s[b:b + 1] for s in stages], gt[b:b + 1], cube[b:b + 1])
        assert np.array_equal(e1[:, 0].view(np.int32), e32[:, b].view(np.int32)) and np.array_equal(p1[:, 0].view(np.int32), p32[:, b].view(np.int32))
