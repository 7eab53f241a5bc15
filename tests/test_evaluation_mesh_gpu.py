"""Device-resident mesh evaluation (keypointfusion_amd/evaluation_mesh_gpu.py, kpf_eval_mesh_* of include/kpf.h) against its yardsticks: the numpy
restatement of the kernel's arithmetic for the plain pass (bit for bit), keypointfusion_amd/evaluation_mesh.py in float64 (LAPACK's SVD) for the aligned pass,
a sequential numpy loop for the accumulated state, `evaluation_mesh.evaluate_meshes` for the summary.  Inputs, restatement and yardstick calls:
tests/mesh_eval_cases.py; that they are what the bounds here assume: tests/test_evaluation_mesh_host.py.

The comparisons with the yardstick print one "ERR ..." line before they assert (`-s` shows them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_eval_cases as MC
from keypointfusion_amd import evaluation_mesh as EM
from keypointfusion_amd import lib as L
from keypointfusion_amd.evaluation_mesh_gpu import DeviceMeshEvaluator

DEV = "cuda:0"
LOGGED = ("err", "nn", "nn_idx", "mean_err", "pck_cnt", "f_cnt")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _update(ev, pred, gt, with_origins=False, valid=None):
    """one update -> numpy copies of everything it logged"""
    po, go = MC.origins(pred, gt) if with_origins else (None, None)
    out = ev.update(_dev(pred), _dev(gt), None if valid is None else _dev(np.asarray(valid, np.uint8)), None if po is None else _dev(po),
                    None if go is None else _dev(go))
    return {k: out[k].cpu().numpy().copy() for k in LOGGED}


_DEVICE = {}


def _device(name, with_origins, thresholds):
    """the device's log of one case, computed once per (case, origins, threshold table)"""
    key = (name, with_origins, thresholds)
    if key not in _DEVICE:
        pred, gt = MC.case(name)
        _DEVICE[key] = _update(DeviceMeshEvaluator(verts=pred.shape[1], thresholds=thresholds, f_thresholds=MC.F_TH), pred, gt, with_origins)
    return _DEVICE[key]


def _bits(a):
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@pytest.mark.gpu
@pytest.mark.parametrize("with_origins", [False, True])
@pytest.mark.parametrize("name", MC.case_names())
def test_plain_outputs_are_the_restatements_bits(name, with_origins):
    """err, nn, nn_idx, mean_err, pck_cnt and f_cnt of the plain pass, for every kind and every V that straddles a lane, wave, thread-stride or LDS
    boundary, with and without origins.  The threshold table starts at 0.0, which `equal`'s error 0.0 meets."""
    got, want = _device(name, with_origins, MC.TH_PLAIN), MC.restated_of(name, with_origins, MC.TH_PLAIN)
    for k in LOGGED:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(_bits(got[k][0]), _bits(want[k][0])), "%s: plain %s differs from the restatement" % (name, k)
    if name == "kinds1":
        b = MC.BATCHES[1].index("equal")
        assert (got["err"][0, b] == 0.0).all() and (got["pck_cnt"][0, b] == 778).all() and (got["nn_idx"][0, :, b] == np.arange(778)).all()
        b = MC.BATCHES[1].index("duplicate")
        assert (got["nn_idx"][0, 0, b] == MC.DUP[0]).any() and not (got["nn_idx"][:, 0, b] == MC.DUP[1]).any()  # of two identical candidates the lower index
    if name == "kinds0" and not with_origins:  # (each set's own vertex 0 as origin moves the shuffled set against the other)
        b = MC.BATCHES[0].index("permuted")
        assert (got["nn"][0, :, b] == 0.0).all() and (got["f_cnt"][0, b] == 778).all() and got["mean_err"][0, b] > 10.0


def _all_cases():
    return [(n, o) for n in MC.case_names() for o in (False, True)]


@pytest.mark.gpu
def test_aligned_values_against_float64():
    """Aligned err and nn within max(1 ulp32, 1e-7 mm) of the float64 yardstick, the tolerance of tests/test_evaluation_gpu.py: the float64 path's own error
    is many orders below half a float32 ulp, and a minimum is 1-Lipschitz in its candidates.  NaN (no alignment: `coincident`, V = 1) and +inf (nothing
    won) must match as such.  The plain values are held to the same yardstick on the way.  On one MI355X: at most 1.8e-12 mm apart (rounding residue of
    `equal` / `shifted`), no value above 1e-3 mm differs in a bit."""
    worst = {"err": 0.0, "nn": 0.0}
    worst_ulp = 0.0
    for name, org in _all_cases():
        got, y = _device(name, org, MC.TH_DECIDED), MC.yardstick_of(name, org)
        for key in ("err", "nn"):
            assert np.array_equal(_bits(got[key][0]), _bits(y[key][0])), "%s: plain %s" % (name, key)
            ok, diff = MC.within_tolerance(got[key][1], y[key][1])
            worst[key] = max(worst[key], diff.max())
            big = np.isfinite(y[key][1]) & (y[key][1] > 1e-3)
            worst_ulp = max(worst_ulp, (diff[big] / MC.ulp32(y[key][1][big])).max(initial=0.0))
            assert ok.all(), "%s (origins %s): aligned %s %.3e mm from float64" % (name, org, key, diff.max())
    print("ERR mesh eval aligned: err max %.3e mm, nn max %.3e mm from float64; max %.3f ulp32 on values > 1e-3 mm" % (worst["err"], worst["nn"], worst_ulp))


@pytest.mark.gpu
def test_aligned_nearest_indices_against_float64():
    """Equal at every vertex whose nearest and second-nearest distance differ by more than 1e-6 mm in float64 (the host test shows that this leaves out at
    most 1 % of a case's vertices)."""
    left_out = total = 0
    for name, org in _all_cases():
        got, y = _device(name, org, MC.TH_DECIDED), MC.yardstick_of(name, org)
        decided = y["gap"][1] > MC.DECIDED_MM
        left_out, total = left_out + int((~decided).sum()), total + decided.size
        assert np.array_equal(got["nn_idx"][1][decided], y["nn_idx"][1][decided]), name
        assert np.array_equal(got["nn_idx"][0], y["nn_idx"][0]), name
    print("ERR mesh eval aligned nn_idx: %d of %d vertices left out as undecided" % (left_out, total))
    assert left_out <= 0.01 * total


@pytest.mark.gpu
def test_aligned_counts_against_float64():
    """pck_cnt and f_cnt equal the yardstick's: no yardstick distance lies within 1e-6 mm of a threshold of these tables (the host test)."""
    for name, org in _all_cases():
        got, y = _device(name, org, MC.TH_DECIDED), MC.yardstick_of(name, org)
        assert y["margin"].min() > MC.DECIDED_MM
        for k in ("pck_cnt", "f_cnt"):
            assert np.array_equal(got[k], y[k]), "%s (origins %s): %s" % (name, org, k)


@pytest.mark.gpu
def test_coincident_prediction_has_no_alignment():
    """Aligned err and mean_err NaN; nothing wins the aligned nearest-vertex scan (nn_idx -1, nn +inf: include/kpf.h); aligned counts 0; the plain figures
    and the other samples finite.  Accumulated: the aligned sums are NaN from then on, the plain ones are not."""
    pred, gt, kinds = MC.kind_batch(1)
    b = kinds.index("coincident")
    ev = DeviceMeshEvaluator()
    got = _update(ev, pred, gt)
    assert np.isnan(got["err"][1, b]).all() and np.isnan(got["mean_err"][1, b])
    assert (got["nn_idx"][1, :, b] == -1).all() and np.isposinf(got["nn"][1, :, b]).all()
    assert not got["pck_cnt"][1, b].any() and not got["f_cnt"][1, b].any()
    others = [i for i in range(len(kinds)) if i != b]
    assert np.isfinite(got["err"][0]).all() and np.isfinite(got["nn"][0]).all() and np.isfinite(got["mean_err"][0]).all() and got["pck_cnt"][0, b].any()
    assert np.isfinite(got["err"][1, others]).all() and np.isfinite(got["nn"][1][:, others]).all() and (got["nn_idx"][1][:, others] >= 0).all()
    want = MC.restated_of("kinds1", False, MC.TH_PLAIN)
    assert np.array_equal(_bits(got["err"][0]), _bits(want["err"][0])) and np.array_equal(got["pck_cnt"][0], want["pck_cnt"][0])
    st = {k: v.cpu().numpy() for k, v in ev.state().items()}
    assert np.isfinite(st["sum_mean_err"][0]) and np.isnan(st["sum_mean_err"][1]) and np.isfinite(st["sum_vert"][0]).all() and np.isnan(st["sum_vert"][1]).all()
    assert np.isfinite(st["sum_f"]).all() and st["pck"][1].max() <= 778 * len(others)
    s = ev.summary()
    assert np.isfinite(s["mean_error"]) and np.isnan(s["pa_mean_error"]) and s["samples"] == len(kinds)


def _sequential_state(ev, logs, valids):
    """The state after the batches `logs`, from their logged float32 err and nn alone, in the order include/kpf.h states, in Python floats (float64)."""
    V, th, fth = ev.verts, ev.thresholds, ev.f_thresholds
    st = dict(n_samples=0, n_batches=0, sum_mean_err=np.zeros(2), sum_vert=np.zeros((2, V)), pck=np.zeros((2, len(th)), np.int64), sum_f=np.zeros((2, len(fth), 3)))
    for log, valid in zip(logs, valids):
        keep = [b for b in range(log["err"].shape[1]) if valid is None or valid[b]]
        if not keep:
            continue
        st["n_samples"] += len(keep)
        st["n_batches"] += 1
        for a in range(2):
            for b in keep:
                e = log["err"][a, b].astype(np.float64)
                st["sum_mean_err"][a] = float(st["sum_mean_err"][a]) + float(MC.tree_sum(e) / float(V))
                st["sum_vert"][a] = st["sum_vert"][a] + e  # elementwise: one chain per vertex
                st["pck"][a] += (e[:, None] <= th[None, :]).sum(0)
                for k, tau in enumerate(fth):
                    hp, hg = (int((log["nn"][a, d, b].astype(np.float64) <= tau).sum()) for d in range(2))
                    P, R = hp / float(V), hg / float(V)
                    F = 2.0 * P * R / (P + R) if P + R > 0 else 0.0
                    for c, x in enumerate((F, P, R)):
                        st["sum_f"][a, k, c] = float(st["sum_f"][a, k, c]) + x
    return st


def _assert_state(ev, want):
    got = {k: v.cpu().numpy() for k, v in ev.state().items()}
    assert int(got["n_samples"][0]) == want["n_samples"] and int(got["n_batches"][0]) == want["n_batches"]
    for k in ("sum_mean_err", "sum_vert", "sum_f"):
        assert got[k].dtype == np.float64 and np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k  # bit-equal
    assert got["pck"].dtype == np.int64 and np.array_equal(got["pck"], want["pck"])
    return got


def _three_batches():
    """kinds0 whole, kinds1 without its `coincident` sample (so that the aligned sums stay finite), kinds0 again with no sample valid"""
    (p0, g0, _), (p1, g1, k1) = MC.kind_batch(0), MC.kind_batch(1)
    mask = [0 if k == "coincident" else 1 for k in k1]
    return [(p0, g0, None), (p1, g1, mask), (p0, g0, [0] * len(p0))]


@pytest.mark.gpu
def test_accumulation_is_exact_and_summary_matches_evaluate_meshes():
    batches = _three_batches()
    ev = DeviceMeshEvaluator(thresholds=MC.TH_DECIDED, f_thresholds=MC.F_TH)
    logs = [_update(ev, p, g, valid=v) for p, g, v in batches[:2]]
    want = _sequential_state(ev, logs, [v for _, _, v in batches[:2]])
    assert want["n_samples"] == 8 and want["n_batches"] == 2
    got = _assert_state(ev, want)
    assert got["pck"].max() <= 8 * 778 and got["pck"][0, -1] > 0
    logs.append(_update(ev, *batches[2][:2], valid=batches[2][2]))  # a batch without a valid sample adds nothing and is not counted
    _assert_state(ev, want)
    assert np.array_equal(_bits(logs[2]["err"]), _bits(logs[0]["err"]))  # its log is written all the same
    # the summary: against evaluate_meshes on the device's own log (the aggregation alone) and on the inputs (the whole path in float64)
    keep = [(i, b) for i, (_, _, v) in enumerate(batches[:2]) for b in range(len(batches[i][0])) if v is None or v[b]]
    pred, gt = np.stack([batches[i][0][b] for i, b in keep]), np.stack([batches[i][1][b] for i, b in keep])
    err, nn = np.stack([logs[i]["err"][:, b] for i, b in keep], 1), np.stack([logs[i]["nn"][:, :, b] for i, b in keep], 2)
    summ = ev.summary()
    assert summ["samples"] == 8 and summ["batches"] == 2
    of_log = EM.evaluate_meshes(None, None, MC.TH_DECIDED, MC.F_TH, logged=(err, nn))
    of_inputs = EM.evaluate_meshes(pred, gt, MC.TH_DECIDED, MC.F_TH)
    assert set(summ) == set(of_log) == set(of_inputs)
    for key in summ:
        if key == "batches":
            continue
        for want_, exact in ((of_log, True), (of_inputs, key not in ("pa_mean_error", "pa_per_vertex_mean"))):
            g_, w_ = (np.array([d[key][t] for t in MC.F_TH]) for d in (summ, want_)) if isinstance(summ[key], dict) else (summ[key], want_[key])
            if exact:
                np.testing.assert_allclose(g_, w_, rtol=1e-12, atol=0, err_msg=key)
            else:  # means of aligned errors that are each within max(1 ulp32, 1e-7 mm) of the yardstick's
                np.testing.assert_allclose(g_, w_, rtol=2.0 ** -23, atol=1e-7, err_msg=key)
    assert summ["f_score"][15.0] >= summ["f_score"][5.0] and summ["pa_mean_error"] < summ["mean_error"]
    ev.reset()
    assert all(int(v.view(torch.int64).abs().sum()) == 0 for v in ev.state().values())


@pytest.mark.gpu
def test_merge_adds_the_integer_state_exactly():
    batches = _three_batches()
    whole, a, b = (DeviceMeshEvaluator(thresholds=MC.TH_DECIDED) for _ in range(3))
    for part, idx in ((whole, (0, 1, 2)), (a, (0, 2)), (b, (1,))):
        for i in idx:
            _update(part, *batches[i][:2], valid=batches[i][2])
    sa, sb, sw = ({k: v.cpu().numpy().copy() for k, v in e.state().items()} for e in (a, b, whole))
    assert a.merge(b) is a
    m = {k: v.cpu().numpy() for k, v in a.state().items()}
    for k in ("n_samples", "n_batches", "pck"):
        assert np.array_equal(m[k], sw[k]) and np.array_equal(m[k], sa[k] + sb[k]), k
    for k in ("sum_mean_err", "sum_vert", "sum_f"):
        assert np.array_equal(m[k], sa[k] + sb[k]), k
        np.testing.assert_allclose(m[k], sw[k], rtol=1e-14)
    assert int(m["n_samples"][0]) == 8 and int(m["n_batches"][0]) == 2
    fresh = DeviceMeshEvaluator(thresholds=MC.TH_DECIDED).merge(b)  # into an evaluator that has seen nothing
    assert all(torch.equal(v, b.state()[k]) for k, v in fresh.state().items())


@pytest.mark.gpu
def test_a_samples_bits_do_not_depend_on_the_batch():
    (p0, g0, _), (p1, g1, _) = MC.kind_batch(0), MC.kind_batch(1)
    pred, gt = np.concatenate([p0, p1])[:6], np.concatenate([g0, g1])[:6]
    for org in (False, True):
        six = _update(DeviceMeshEvaluator(), pred, gt, org)
        for b in (0, 3, 5):  # noisy2, mirrored, shifted
            one = _update(DeviceMeshEvaluator(), pred[b:b + 1], gt[b:b + 1], org)
            for k in LOGGED:
                ax = 2 if k in ("nn", "nn_idx") else 1  # the axis of B
                assert np.array_equal(_bits(np.take(six[k], b, axis=ax)), _bits(np.take(one[k], 0, axis=ax))), (k, b, org)


@pytest.mark.gpu
def test_update_is_capturable_and_replay_equals_eager():
    """A successful capture is also the check that update() neither synchronises nor allocates."""
    (p0, g0, _), (p1, g1, _) = MC.kind_batch(0), MC.kind_batch(1)
    batches = [(p0[:4], g0[:4]), (p1[:4], g1[:4])]
    valid = _dev(np.array([1, 1, 0, 1], np.uint8))  # drops `similarity`, then `coincident`
    eager = DeviceMeshEvaluator()
    for p, g in batches:
        last = eager.update(_dev(p), _dev(g), valid, _dev(MC.origins(p, g)[0]), _dev(MC.origins(p, g)[1]))
    want = {k: v.cpu().numpy().copy() for k, v in eager.state().items()}
    want_log = {k: last[k].cpu().numpy().copy() for k in LOGGED}

    ev = DeviceMeshEvaluator()
    s_p, s_g = _dev(batches[0][0]), _dev(batches[0][1])
    s_po, s_go = (_dev(o) for o in MC.origins(*batches[0]))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.update(s_p, s_g, valid, s_po, s_go)  # eager warm-up: buffers, state and library are in place
        ev.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ev.update(s_p, s_g, valid, s_po, s_go)
    ev.reset()  # (whatever the capture itself left)
    for p, g in batches:
        for dst, src in zip((s_p, s_g, s_po, s_go), (p, g) + MC.origins(p, g)):
            dst.copy_(_dev(src))
        graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in ev.state().items()}
    assert int(got["n_samples"][0]) == 6 and int(got["n_batches"][0]) == 2
    for k in want:
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k
    for k in LOGGED:
        assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(want_log[k])), k  # the replay's log of the last batch


@pytest.mark.gpu
def test_c_entries_refuse_bad_arguments_and_write_nothing():
    lib = L.load()
    B, V, T, Tf = 2, 778, 100, 2
    pred, gt = MC.kind_batch(0)[0][:B], MC.kind_batch(0)[1][:B]
    d = dict(pred=_dev(pred), gt=_dev(gt), po=_dev(pred[:, 0]), go=_dev(gt[:, 0]), th=_dev(np.linspace(0.0, 50.0, 256)), fth=_dev(np.arange(1.0, 9.0)))
    outs = dict(err=torch.full((2, B, 1024), -7.0, device=DEV), nn=torch.full((2, 2, B, 1024), -7.0, device=DEV),
                nn_idx=torch.full((2, 2, B, 1024), -7, device=DEV, dtype=torch.int32), mean_err=torch.full((2, B), -7.0, device=DEV, dtype=torch.float64),
                pck_cnt=torch.full((2, B, 256), -7, device=DEV, dtype=torch.int32), f_cnt=torch.full((2, B, 8, 2), -7, device=DEV, dtype=torch.int32))
    st = torch.cuda.current_stream().cuda_stream

    def call(po=None, go=None, T=T, Tf=Tf, B=B, V=V):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        return lib.kpf_eval_mesh_f32(p(d["pred"]), p(d["gt"]), p(po), p(go), p(d["th"]), T, p(d["fth"]), Tf, B, V, *(p(outs[k]) for k in LOGGED), st)

    for bad, word in ((dict(V=0), "V = 0"), (dict(V=1025), "V = 1025"), (dict(T=257), "T = 257"), (dict(T=0), "T = 0"), (dict(Tf=9), "Tf = 9"),
                      (dict(po=d["po"]), "given together"), (dict(go=d["go"]), "given together"), (dict(B=0), "bad shape")):
        assert call(**bad) != 0, bad
        msg = lib.kpf_last_error().decode()
        assert msg.startswith("kpf_eval_mesh_f32: ") and word in msg, msg
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs.values())  # nothing was written
    assert call() == 0 and call(po=d["po"], go=d["go"]) == 0  # the same buffers, accepted
    torch.cuda.synchronize()
    assert bool((outs["err"].view(-1)[:2 * B * V] >= 0).all()) and bool((outs["err"].view(-1)[2 * B * V:] == -7).all())
