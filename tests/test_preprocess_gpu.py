"""The device preprocessing path (keypointfusion_amd/preprocess_gpu.py on kpf_prep_* of libkpf_hip.so) against the host path it reproduces
(keypointfusion_amd/preprocess.py::prepare_rgbd, project_to_crop, uncrop_points) on the same inputs: the demo frame (whole, and as a window with an
origin) and the synthetic frames of tests/prep_cases.py, mixed inside one launch at B = 1, 7 and 32.

Bounds: integer decisions and both images bit-equal; center / M within one float32 ulp and com within 1e-12 relative (the device sums integers, the host
sums float64 coordinates pairwise); candidate points within 2.4e-7 (two float32 ulp at 1.0: both sides compute in double and round once, the allowance is
for the clip boundary); un-cropped pixels within 1e-3 px.  The point sample is not numpy's RandomState stream: it is checked by its properties."""
import numpy as np
import pytest
import torch

import prep_cases as PC
from keypointfusion_amd import preprocess as P

pytestmark = pytest.mark.gpu
NAMES = list(PC.CASES)
_HOST = {}


def _dev():
    return torch.device("cuda:0")


def _host(name):
    if name not in _HOST:
        rgb, depth, bbox, cam = PC.synth_frame(name)
        _HOST[name] = (rgb, depth, bbox, cam, PC.host_record(rgb, depth, bbox, cam))
    return _HOST[name]


def _batch(names, seeds):
    fr = [_host(n) for n in names]
    dev = _dev()
    return (torch.from_numpy(np.stack([f[0] for f in fr])).to(dev), torch.from_numpy(np.stack([f[1] for f in fr])).to(dev),
            torch.tensor([f[2] for f in fr], dtype=torch.float64, device=dev), torch.tensor([f[3] for f in fr], dtype=torch.float64, device=dev),
            torch.tensor(list(seeds), dtype=torch.int64, device=dev))


def _cpu(prep):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in prep.items()}


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32).ravel() + 0.0, np.ascontiguousarray(b, np.float32).ravel() + 0.0  # (+ 0.0: -0 and +0 are the same value)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


def _check_sample(d, b, h, n=1024):
    """Sample b of a device result d (numpy) against the host record h: every bound of the module docstring, and the properties of the sample."""
    assert np.array_equal(d["bounds"][b, :4], h["bounds"]) and np.array_equal(d["bounds"][b, 4:], h["sz"])
    assert np.array_equal(d["img"][b], h["img"]) and np.array_equal(d["img_rgb"][b], h["img_rgb"])
    N = len(h["candidates"])
    assert int(d["pcl_count"][b]) == N
    assert _ulps(d["center"][b], h["center"]) <= 1 and _ulps(d["M"][b], h["M"]) <= 1
    assert np.abs(d["com"][b] - h["com"]).max() <= 1e-12 * np.abs(h["com"]).max()
    assert np.array_equal(d["cube"][b], h["cube"]) and np.array_equal(d["cam_para"][b], h["cam_para"])
    cand = d["candidates"][b, :N]
    if N:
        err = float(np.abs(cand.astype(np.float64) - h["candidates"]).max())
        print("candidates %d, max deviation %.3g" % (N, err))
        assert err <= 2.4e-7  # same count, same (np.where) order
    idx, pcl = d["pcl_index"][b], d["pcl"][b]
    if N == 0:
        assert not pcl.any() and (idx == -1).all()
        return
    assert idx.min() >= 0 and idx.max() < N
    assert np.array_equal(pcl.view(np.int32), cand[idx].view(np.int32))  # bit for bit
    mult = np.bincount(idx, minlength=N)
    if N >= n:
        assert mult.max() == 1
    else:
        q, r = divmod(n, N)
        assert mult.min() >= q and mult.max() <= q + 1 and int((mult == q + 1).sum()) == r


@pytest.fixture(scope="module")
def pre():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    return DevicePreprocessor(img_size=128, sample_num=1024, cube=PC.CUBE, debug_candidates=True)


@pytest.mark.parametrize("B", [1, 7, 32])
def test_mixed_batches_match_the_host_path(pre, B):
    """Cases mixed inside one launch (per-sample control flow: tiling, empty clouds, zero padding, letterboxing) against prepare_rgbd sample by sample."""
    lists = [[n] for n in NAMES] if B == 1 else [[NAMES[(i * 3 + 1) % len(NAMES)] for i in range(B)]] if B == 32 else [NAMES[:7]]
    if B == 7:
        lists.append(NAMES[1:8])
    for names in lists:
        d = _cpu(pre.prepare(*_batch(names, range(100, 100 + len(names)))))
        for b, name in enumerate(names):
            print(B, b, name)
            _check_sample(d, b, _host(name)[4])


def test_results_do_not_depend_on_the_batch(pre):
    """Same frame and seed alone and at several positions of a B = 32 batch: every output bit-identical; another seed: another order of the sample."""
    names = [NAMES[i % len(NAMES)] for i in range(32)]
    seeds = [7 + (i % len(NAMES)) for i in range(32)]
    big = _cpu(pre.prepare(*_batch(names, seeds)))
    again = _cpu(pre.prepare(*_batch(names, seeds)))
    for k in big:
        assert np.array_equal(big[k], again[k], equal_nan=False), k  # run to run
    for i, name in enumerate(NAMES):
        one = _cpu(pre.prepare(*_batch([name], [7 + i])))
        N = int(one["pcl_count"][0])
        for b in range(i, 32, len(NAMES)):  # the same (frame, seed) at four batch positions
            for k in one:
                a, c = one[k][0], big[k][b]
                if k == "candidates":
                    a, c = a[:N], c[:N]
                assert np.array_equal(a, c), (name, b, k)
        other = _cpu(pre.prepare(*_batch([name], [1007 + i])))
        assert np.array_equal(other["img"], one["img"]) and other["pcl_count"][0] == N
        if N:
            assert not np.array_equal(other["pcl_index"], one["pcl_index"]), name


def test_demo_frame_whole_and_as_a_window(pre):
    """The reference's sample frame as the zero-embedded 1920 x 1080 frame and as its 460 x 500 window with an origin: identical outputs, equal to the host's."""
    rw, dw, bbox, cam, org, fs = PC.demo_window()
    rgb, depth = PC.embed(rw, dw, org, fs)
    h = PC.host_record(rgb, depth, bbox, cam)
    dev = _dev()
    t = lambda a, dt=None: torch.tensor(a, dtype=dt, device=dev) if dt else torch.from_numpy(a).to(dev)
    bb, cm, sd = t([bbox], torch.float64), t([cam], torch.float64), t([3], torch.int64)
    full = _cpu(pre.prepare(t(rgb[None]), t(depth[None]), bb, cm, sd))
    win = _cpu(pre.prepare(t(rw[None]), t(dw[None]), bb, cm, sd, origin=org, frame_size=fs))
    N = int(full["pcl_count"][0])
    for k in full:
        a, c = (full[k][:, :N], win[k][:, :N]) if k == "candidates" else (full[k], win[k])
        assert np.array_equal(a, c), k
    _check_sample(full, 0, h)
    _check_sample(win, 0, h)
    # round trip of the centre of mass: the cube's centre (normalised joint 0) projects to com and must come back to it through M and M^-1
    crop_px, frame_px = pre.uncrop(torch.zeros(1, 1, 3, device=dev), pre.prepare(t(rw[None]), t(dw[None]), bb, cm, sd, origin=org, frame_size=fs))
    back = frame_px.cpu().numpy()[0, 0]
    print("com round trip", back[:2] - h["com"][:2])
    assert np.abs(back[:2] - h["com"][:2]).max() < 1.2e-4 and abs(back[2] - h["com"][2]) < 1.2e-4
    c = crop_px.cpu().numpy()[0, 0]
    assert abs(c[0] - 64) < 1.5 and abs(c[1] - 64) < 1.5


def test_sample_is_uniform_and_in_random_order(pre):
    """`centre` (N = 2969), 256 fixed seeds.  Inclusion counts per candidate: Pearson chi-square against 256 n / N below dof + 6 sqrt(2 dof), dof = N - 1
    (sampling without replacement only lowers the variance, so the bound is safe).  Order: the correlation between output slot and candidate index over
    the 256 n draws below 6 / sqrt(256 n) — DESA's ball query keeps the first 64 hits in index order, a raster-ordered sample would bias every ball."""
    n, draws = 1024, 256
    N = len(_host("centre")[4]["candidates"])
    counts = np.zeros(N, np.int64)
    slots, cands = [], []
    for r in range(draws // 32):
        d = _cpu(pre.prepare(*_batch(["centre"] * 32, range(5000 + 32 * r, 5000 + 32 * (r + 1)))))
        assert (d["pcl_count"] == N).all()
        for b in range(32):
            counts += np.bincount(d["pcl_index"][b], minlength=N)
            slots.append(np.arange(n))
            cands.append(d["pcl_index"][b])
    E = draws * n / N
    chi2, dof = float(((counts - E) ** 2 / E).sum()), N - 1
    corr = float(np.corrcoef(np.concatenate(slots).astype(np.float64), np.concatenate(cands).astype(np.float64))[0, 1])
    print("chi2 %.1f (dof %d, bound %.1f); slot/candidate correlation %.2e (bound %.2e)" % (chi2, dof, dof + 6 * np.sqrt(2 * dof), corr, 6 / np.sqrt(draws * n)))
    assert chi2 < dof + 6 * np.sqrt(2 * dof)
    assert abs(corr) < 6 / np.sqrt(draws * n)


def test_uncrop_matches_the_host_in_float64(pre):
    names = NAMES[:7]
    prep = pre.prepare(*_batch(names, range(7)))
    g = np.random.RandomState(3)
    joints = (g.rand(7, 21, 3) * 1.6 - 0.8).astype(np.float32)
    crop_px, frame_px = pre.uncrop(torch.from_numpy(joints).to(_dev()), prep)
    d = _cpu(prep)
    crop_px, frame_px = crop_px.cpu().numpy(), frame_px.cpu().numpy()
    worst = 0.0
    for b in range(7):
        want_c = P.project_to_crop(joints[b], d["center"][b], d["M"][b], d["cube"][b], d["cam_para"][b])
        want_f = P.uncrop_points(want_c, d["M"][b])
        worst = max(worst, float(np.abs(crop_px[b] - want_c).max()), float(np.abs(frame_px[b] - want_f).max()))
    print("uncrop: max deviation %.3g px" % worst)
    assert worst < 1e-3


# ---- through the model -------------------------------------------------------------------------------------------------------------------------------

_MODEL = {}


def _model():
    if not _MODEL:
        from conftest import synthetic_sd
        from keypointfusion_amd.model.model import KPFusion
        net = "KPFusion-convnext-tiny"
        sd = synthetic_sd(net)
        m = KPFusion(net, "", 21, "dexycb", "")
        m.load_state_dict(sd)
        _MODEL["m"], _MODEL["sd"] = m.to(_dev()).eval(), sd
    return _MODEL["m"], _MODEL["sd"]


def test_demo_frame_through_the_model_matches_the_oracle():
    """Demo frame -> DevicePreprocessor.prepare -> plan.forward -> uncrop, against the CPU oracle fed the device-produced inputs: the bars of
    test_preprocess.py::test_demo_crop_through_the_model_matches_oracle (1e-3 relative on the eight outputs, frame pixels within 0.05 px)."""
    from keypointfusion_amd.preprocess_gpu import MODEL_INPUTS, DevicePreprocessor
    from oracle.compare import oracle_with_device_decisions
    m, sd = _model()
    dev = _dev()
    pre = DevicePreprocessor()
    rw, dw, bbox, cam, org, fs = PC.demo_window()
    prep = pre.prepare(torch.from_numpy(rw[None]).to(dev), torch.from_numpy(dw[None]).to(dev), torch.tensor([bbox], dtype=torch.float64, device=dev),
                       torch.tensor([cam], dtype=torch.float64, device=dev), torch.tensor([0], dtype=torch.int64, device=dev), origin=org, frame_size=fs)
    plan = m._plan(dev)
    with torch.no_grad():
        res, sws, ctx = plan.forward(*[prep[k] for k in MODEL_INPUTS], 0.8, 128, 1, want_aux=True)
    crop_px, frame_px = pre.uncrop(res[5], prep)
    b = {k: prep[k].cpu() for k in MODEL_INPUTS}
    ref, rsw, _, report = oracle_with_device_decisions(sd, b, ctx)
    for o, r in zip(res + sws, ref + rsw):
        assert float((o.cpu() - r).abs().max() / r.abs().max()) < 1e-3
    pn = {k: v.numpy()[0] for k, v in b.items()}
    full_ref = P.uncrop_points(P.project_to_crop(ref[5].numpy()[0], pn["center"], pn["M"], pn["cube"], pn["cam_para"]), pn["M"])
    got = frame_px.cpu().numpy()[0]
    assert np.isfinite(got).all()
    print("frame pixels against the oracle's: %.4f px" % np.abs(got[:, :2] - full_ref[:, :2]).max())
    assert np.abs(got[:, :2] - full_ref[:, :2]).max() < 0.05


def test_prepare_and_forward_in_one_graph():
    """prepare + forward captured in ONE graph; replayed with a second set of frames, boxes and seeds written into the static input buffers, the outputs are
    bit-identical to the eager run on those inputs."""
    from keypointfusion_amd.preprocess_gpu import MODEL_INPUTS, DevicePreprocessor
    m, _ = _model()
    dev = _dev()
    plan = m._plan(dev)
    first, second = _batch(["centre", "corner"], [11, 12]), _batch(["fx_ne_fy", "far_small"], [21, 22])
    pre_e, pre_g = DevicePreprocessor(), DevicePreprocessor()

    def run(pre, ins):
        prep = pre.prepare(*ins)
        res, sws, _ = plan.forward(*[prep[k] for k in MODEL_INPUTS], 0.8, 128, 1)
        crop_px, frame_px = pre.uncrop(res[5], prep)
        return [prep[k] for k in ("img", "img_rgb", "pcl", "pcl_index", "center", "M")] + list(res) + list(sws) + [crop_px, frame_px]

    with torch.no_grad():
        want = [t.clone() for t in run(pre_e, second)]
        static = [t.clone() for t in first]
        warm = torch.cuda.Stream(device=dev)
        warm.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(warm):
            run(pre_g, static)
            run(pre_g, static)
        torch.cuda.current_stream(dev).wait_stream(warm)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = run(pre_g, static)
        for s, t in zip(static, second):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize(dev)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
    assert int(pre_g.prepare(*static)["pcl_count"][1]) == 357  # (the replay really saw the second batch: far_small)


def test_submit_frames_equals_prepare_then_submit():
    """PipelinedEval.submit_frames, two batches in flight over four batches, against prepare followed by submit."""
    from keypointfusion_amd.preprocess_gpu import MODEL_INPUTS, DevicePreprocessor
    from keypointfusion_amd.serving import PipelinedEval
    m, _ = _model()
    dev = _dev()
    pre = DevicePreprocessor()
    batches = [_batch([NAMES[(2 * i + j) % len(NAMES)] for j in range(2)], [50 + 2 * i, 51 + 2 * i]) for i in range(4)]
    pe = PipelinedEval(m, depth=2)
    with torch.no_grad(), torch.cuda.stream(pe.feed_stream(dev)):
        want = []
        for ins in batches:
            prep = pre.prepare(*ins)
            res, sws, _ = pe.collect(pe.submit(*[prep[k] for k in MODEL_INPUTS[:3]], None, *[prep[k] for k in MODEL_INPUTS[3:]]))
            want.append([t.clone() for t in res + sws] + list(pre.uncrop(res[5], prep)))
        tickets = [pe.submit_frames(pre, *ins) for ins in batches]  # all four enqueued before the first is collected
        got = []
        for ticket, keep in tickets:
            res, sws, _ = pe.collect(ticket)
            got.append(list(res + sws) + list(pre.uncrop(res[5], keep)))
    torch.cuda.synchronize(dev)
    for g, w in zip(got, want):
        assert len(g) == len(w) == 10
        for a, c in zip(g, w):
            assert torch.equal(a, c)
