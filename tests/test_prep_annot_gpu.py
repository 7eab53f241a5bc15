"""Preprocessing by the dataset protocol on the device (DevicePreprocessor.prepare_annotated on kpf_prep_annot_u16 + kpf_prep_pcl_sample, uncrop on
kpf_prep_uncrop_mirror_f32) against the host path it reproduces (keypointfusion_amd/preprocess.py::prepare_annotated, itself pinned to the reference's dataset
items by tests/test_prep_annot_host.py) on the frames of tests/annot_cases.py, mixed inside one launch.

Bounds: img, img_rgb, bounds, M, M64, center, com, cube, cam_para, joint and joint_img BIT-EQUAL (every operation is an IEEE +, -, *, / in a stated order and
the centre is a 21-term sequential sum, not a reduction over pixels: no ulp allowance, no floor-margin condition); pcl_count equal; candidate points within
2.4e-7 (the bound of tests/test_preprocess_gpu.py: both sides compute in double and round once, the allowance is for the clip boundary); sampled rows
bit-equal to candidates[pcl_index] with the multiplicities of sample_points; un-cropped pixels within 1e-3 px of the float64 host (that file's bound)."""
import numpy as np
import pytest
import torch

import annot_cases as AC
import prep_cases as PC
from keypointfusion_amd import preprocess as P

pytestmark = pytest.mark.gpu
BIT_EQUAL = ("img", "img_rgb", "M", "M64", "center", "com", "cube", "cam_para", "joint", "joint_img")
_HOST = {}


def _dev():
    return torch.device("cuda:0")


def _inputs(name, centred=False):
    """synth()'s tuple; centred: every case gets a GIVEN centre (the 'given' case its own, the others one a few mm off the joint mean), because the centre
    is given or not for a whole launch.  hd_left is its window embedded in zeros, so that the whole frame and the window hold the same pixels."""
    rgb, depth, joints_mm, cam, mirror, center = AC.synth(name)
    if name == "hd_left":
        (x0, y0), (Hs, Ws) = AC.HD_WINDOW
        rgb, depth = PC.embed(rgb[y0:y0 + Hs, x0:x0 + Ws], depth[y0:y0 + Hs, x0:x0 + Ws], (x0, y0), depth.shape)
    if not centred:
        center = None
    elif center is None:
        center = (joints_mm.astype(np.float64).mean(0) + np.array([5.0, -3.0, 2.0])).astype(np.float32)
    return rgb, depth, joints_mm, cam, mirror, center


def _host(name, centred=False, S=128, n=1024):
    key = (name, centred, S, n)
    if key not in _HOST:  # computed once, shared by the tests, never modified
        ins = _inputs(name, centred)
        _HOST[key] = (ins, AC.host_record(*ins, img_size=S, sample_num=n))
    return _HOST[key]


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) if dt is None else torch.tensor(a, dtype=dt, device=_dev())


def _batch(items, seeds):
    """items: synth()-style tuples -> the keyword arguments of prepare_annotated (center_xyz only when every item has one)."""
    kw = dict(rgb=_t(np.stack([i[0] for i in items])), depth=_t(np.stack([i[1] for i in items])), joints_mm=_t(np.stack([i[2] for i in items])),
              cam=_t(np.stack([i[3] for i in items])), seed=_t(list(seeds), torch.int64), mirror=_t(np.array([i[4] for i in items], np.uint8)))
    if items[0][5] is not None:
        kw["center_xyz"] = _t(np.stack([i[5] for i in items]))
    return kw


def _cpu(prep):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in prep.items() if isinstance(v, torch.Tensor)}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_sample(d, b, h, n=1024):
    """Sample b of a device result d (numpy) against the host record h: every bound of the module docstring, and the properties of the sample."""
    assert np.array_equal(d["bounds"][b, :4], h["bounds"]) and np.array_equal(d["bounds"][b, 4:], h["sz"])
    for k in BIT_EQUAL:
        want = h[k][None] if k == "img" and h[k].ndim == 2 else h[k]
        assert _same_bits(d[k][b], want), (k, d[k][b], want)
    assert bool(d["mirror"][b]) == h["mirror"]
    N = len(h["candidates"])
    assert int(d["pcl_count"][b]) == N
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


def _assert_equal(a, c, what=""):
    """Two device results (numpy): every output bit-identical (candidate rows beyond the count are not written)."""
    assert set(a) == set(c)
    for k in a:
        x, y = a[k], c[k]
        if k == "candidates":
            for b in range(len(x)):
                N = int(a["pcl_count"][b])
                assert _same_bits(x[b, :N], y[b, :N]), (what, k, b)
        else:
            assert _same_bits(x, y), (what, k)


@pytest.fixture(scope="module")
def pre():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    return DevicePreprocessor(img_size=128, sample_num=1024, cube=AC.CUBE, debug_candidates=True)


@pytest.mark.parametrize("B", [1, 5, 32])
def test_mixed_batches_match_prepare_annotated(pre, B):
    """Cases interleaved inside one launch (right and left hands, padding, letterboxing, tiling, empty clouds), with the centre from the joints and with a
    given centre, against prepare_annotated sample by sample."""
    S = AC.SMALL
    if B == 1:
        lists = [([n], False) for n in AC.CASES] + [(["given"], True), (["left"], True)]
    elif B == 5:
        lists = [(S[0:10:2], False), (S[1:10:2], False), (S[3:8], True)]
    else:
        lists = [([S[(i * 3 + 1) % len(S)] for i in range(B)], False), ([S[(i * 7 + 2) % len(S)] for i in range(B)], True)]
    for names, centred in lists:
        d = _cpu(pre.prepare_annotated(**_batch([_host(n, centred)[0] for n in names], range(100, 100 + len(names)))))
        for b, name in enumerate(names):
            print(B, b, name, centred)
            _check_sample(d, b, _host(name, centred)[1])


def test_results_do_not_depend_on_the_batch(pre):
    """The same (frame, annotation, seed) alone and at positions 0, 13 and 31 of a B = 32 batch: every output bit-identical; two runs bit-identical."""
    S = AC.SMALL
    names = [S[(i * 3) % len(S)] for i in range(32)]
    for pos, name in ((0, "left_edge"), (13, "far"), (31, "near")):
        names[pos] = name
    seeds = [7 + i for i in range(32)]
    items = [_host(n)[0] for n in names]
    big = _cpu(pre.prepare_annotated(**_batch(items, seeds)))
    _assert_equal(big, _cpu(pre.prepare_annotated(**_batch(items, seeds))), "run to run")
    for pos in (0, 13, 31):
        one = _cpu(pre.prepare_annotated(**_batch([items[pos]], [seeds[pos]])))
        _assert_equal(one, {k: v[pos:pos + 1] for k, v in big.items()}, names[pos])
    # the same sample at the three positions of ONE launch
    items3 = list(items)
    items3[0] = items3[13] = items3[31] = _host("left")[0]
    seeds3 = list(seeds)
    seeds3[0] = seeds3[13] = seeds3[31] = 99
    d = _cpu(pre.prepare_annotated(**_batch(items3, seeds3)))
    alone = _cpu(pre.prepare_annotated(**_batch([_host("left")[0]], [99])))
    for pos in (0, 13, 31):
        _assert_equal(alone, {k: v[pos:pos + 1] for k, v in d.items()}, pos)
    _check_sample(d, 13, _host("left")[1])


def test_mirror_equals_the_preflipped_frame(pre):
    """mirror = 1 on X against mirror = 0 on X[:, ::-1] with the annotations moved with it: every output, for whole frames and for the 1080 x 1920 case
    uploaded as a window with origin / frame_size (the window itself is NOT flipped: the mirror acts on the logical frame)."""
    for name in ("left", "left_edge", "hd_left"):
        rgb, depth, joints_mm, cam, mirror, _ = _host(name)[0]
        frgb, fdepth, fj, fc = AC.flipped(rgb, depth, joints_mm, cam)
        want = _cpu(pre.prepare_annotated(**_batch([(frgb, fdepth, fj, cam, False, fc)], [5])))
        got = _cpu(pre.prepare_annotated(**_batch([(rgb, depth, joints_mm, cam, True, None)], [5])))
        want["mirror"] = got["mirror"]  # (the flag itself is the one difference)
        _assert_equal(got, want, name)
        _check_sample(got, 0, _host(name)[1])
    (x0, y0), (Hs, Ws) = AC.HD_WINDOW
    kw = _batch([(rgb[y0:y0 + Hs, x0:x0 + Ws], depth[y0:y0 + Hs, x0:x0 + Ws], joints_mm, cam, True, None)], [5])
    win = _cpu(pre.prepare_annotated(**kw, origin=(x0, y0), frame_size=depth.shape))
    _assert_equal(win, got, "window")
    assert int(win["pcl_count"][0]) > 500 and win["bounds"][0, 1] - win["bounds"][0, 0] > Ws  # the cube is wider than the window: zero padding on both sides


def test_given_centre_without_joints(pre):
    """HO3D's evaluation split has no ground truth: with joints_mm=None the images and the geometry equal the run with joints, the labels are zeros."""
    items = [_host(n, True)[0] for n in ("given", "corner", "far")]
    kw = _batch(items, [1, 2, 3])
    a = _cpu(pre.prepare_annotated(**kw))
    b = _cpu(pre.prepare_annotated(**{**kw, "joints_mm": None}))
    assert a["joint"].any() and a["joint_img"].any() and not b["joint"].any() and not b["joint_img"].any() and b["joint"].shape == (3, 21, 3)
    a["joint"], a["joint_img"] = b["joint"], b["joint_img"]
    _assert_equal(a, b)


def test_two_hands_on_one_stored_frame(pre):
    """frame_index: a right and a left hand annotated on ONE stored frame equal the same two hands on two copies of it."""
    from keypointfusion_amd.preprocess_gpu import make_frame_index
    r, l = _host("right")[0], _host("left")[0]
    assert np.array_equal(r[1], l[1])  # the same frame
    kw = _batch([r, l], [21, 22])
    two = _cpu(pre.prepare_annotated(**kw))
    one = _cpu(pre.prepare_annotated(**{**kw, "rgb": kw["rgb"][:1].contiguous(), "depth": kw["depth"][:1].contiguous()},
                                     frame_index=make_frame_index([0, 0], 1, _dev())))
    _assert_equal(one, two)
    _check_sample(one, 0, _host("right")[1])
    _check_sample(one, 1, _host("left")[1])


def test_crop_size_64_with_512_samples():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    pre64 = DevicePreprocessor(img_size=64, sample_num=512, cube=AC.CUBE, debug_candidates=True)
    names = ["left_edge", "fx_ne_fy", "far", "wall", "near", "left"]
    d = _cpu(pre64.prepare_annotated(**_batch([_host(n, False, 64, 512)[0] for n in names], range(6))))
    for b, name in enumerate(names):
        _check_sample(d, b, _host(name, False, 64, 512)[1], n=512)


def test_uncrop_takes_mirrored_samples_back_to_the_frame(pre):
    """uncrop on a batch with mirrored samples against project_to_crop + uncrop_points_mirrored in float64: below 1e-3 px (the bound of the existing uncrop
    test); un-mirrored samples of the same batch are the bits of kpf_prep_uncrop_f32."""
    names = ["right", "left", "corner", "left_edge", "fx_ne_fy", "far"]
    prep = pre.prepare_annotated(**_batch([_host(n)[0] for n in names], range(6)))
    g = np.random.RandomState(3)
    joints = (g.rand(6, 21, 3) * 1.6 - 0.8).astype(np.float32)
    crop_px, frame_px = pre.uncrop(_t(joints), prep)
    plain_c, plain_f = pre.uncrop(_t(joints), {k: prep[k] for k in ("center", "M", "cube", "cam_para")})  # kpf_prep_uncrop_f32
    d = _cpu(prep)
    crop_px, frame_px, plain_c, plain_f = (t.cpu().numpy() for t in (crop_px, frame_px, plain_c, plain_f))
    assert _same_bits(crop_px, plain_c)
    worst = 0.0
    for b, name in enumerate(names):
        mirror = bool(d["mirror"][b])
        assert mirror == ("left" in name)
        want_c = P.project_to_crop(joints[b], d["center"][b], d["M"][b], d["cube"][b], d["cam_para"][b])
        want_f = P.uncrop_points_mirrored(want_c, d["M"][b], mirror, prep["frame_w"])
        worst = max(worst, float(np.abs(crop_px[b] - want_c).max()), float(np.abs(frame_px[b] - want_f).max()))
        if mirror:
            assert not np.array_equal(frame_px[b, :, 0], plain_f[b, :, 0]) and _same_bits(frame_px[b, :, 1:], plain_f[b, :, 1:])
        else:
            assert _same_bits(frame_px[b], plain_f[b])
    print("uncrop: max deviation %.3g px" % worst)
    assert worst < 1e-3
    # the labels of a left hand, un-cropped, land on the annotation in the camera's own frame
    _, back = pre.uncrop(prep["joint"], prep)
    ann = P._project_f32(_host("left")[0][2], _host("left")[0][3])
    assert np.abs(back.cpu().numpy()[1, :, :2] - ann[:, :2]).max() < 1e-2


def test_prepare_annotated_and_uncrop_in_one_graph():
    """prepare_annotated + uncrop captured once on one stream; replayed with new frames, annotations, mirror flags and seeds written into the static inputs,
    every output is bit-identical to the eager run on those inputs."""
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    dev = _dev()
    first = _batch([_host(n)[0] for n in ("right", "corner", "left")], [11, 12, 13])
    second = _batch([_host(n)[0] for n in ("left_edge", "far", "fx_ne_fy")], [21, 22, 23])
    pre_e, pre_g = DevicePreprocessor(cube=AC.CUBE), DevicePreprocessor(cube=AC.CUBE)
    keys = ("img", "img_rgb", "pcl", "pcl_index", "pcl_count", "center", "M", "M64", "com", "bounds", "joint", "joint_img", "cam_para")

    def run(pre, kw):
        prep = pre.prepare_annotated(**kw)
        return [prep[k] for k in keys] + list(pre.uncrop(prep["joint"], prep))

    want = [t.clone() for t in run(pre_e, second)]
    static = {k: v.clone() for k, v in first.items()}
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(pre_g, static)
        run(pre_g, static)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(pre_g, static)
    for k in static:
        static[k].copy_(second[k])
    graph.replay()
    torch.cuda.synchronize(dev)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
    assert outs[4].tolist() == [len(_host(n)[1]["candidates"]) for n in ("left_edge", "far", "fx_ne_fy")]  # (the replay really saw the second batch)


def test_labels_feed_the_device_evaluator(pre):
    """Evaluator wiring without a model.  A stage equal to prep["joint"] has errors of exactly 0, from DeviceEvaluator and from evaluation.evaluate_batch
    alike (bit-equal: both are +0.0 everywhere).  A stage prep["joint"] + delta has |delta| * cube / 2: DeviceEvaluator within one float32 ulp of the
    float64 value (its documented rounding: double inside, rounded once), evaluate_batch (float32 throughout) within the 1e-3 mm of
    tests/test_evaluation_gpu.py::test_end_to_end_with_the_decode_matches_evaluate_batch."""
    from keypointfusion_amd import evaluation as EV
    from keypointfusion_amd.evaluation_gpu import DeviceEvaluator
    names = ["right", "left", "corner", "fx_ne_fy"]
    prep = pre.prepare_annotated(**_batch([_host(n)[0] for n in names], range(4)))
    g = np.random.RandomState(5)
    delta = _t((g.rand(4, 21, 3) * 0.2 - 0.1).astype(np.float32))
    stages = [prep["joint"].clone(), prep["joint"] + delta]
    ev = DeviceEvaluator(stage_type=(2, 3))
    args = (prep["img"], prep["joint"], prep["center"], prep["M"], prep["cube"], prep["cam_para"])
    e, _ = ev.update(stages, *args)
    host = EV.evaluate_batch(stages, *args, stage_type=(2, 3))
    e = e.cpu().numpy()
    assert e.shape == (2, 4, 21) and _same_bits(e[0], np.zeros((4, 21), np.float32)) and _same_bits(host[0]["joint_errors"], e[0])
    d64 = (stages[1].cpu().numpy().astype(np.float64) - prep["joint"].cpu().numpy().astype(np.float64)) * (prep["cube"].cpu().numpy().astype(np.float64)[:, None] / 2)
    want = np.sqrt((d64 ** 2).sum(-1))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    print("evaluator: device %.3g ulp from float64, evaluate_batch %.3g mm from the device" % (
        (np.abs(e[1] - want) / ulp).max(), np.abs(host[1]["joint_errors"] - e[1]).max()))
    assert (np.abs(e[1].astype(np.float64) - want) <= ulp).all()
    assert np.abs(host[1]["joint_errors"] - e[1]).max() < 1e-3
    summ = ev.summary()
    assert summ[0]["mean_error"] == 0.0 and abs(summ[1]["mean_error"] - host[1]["mean_error"]) < 1e-3


def test_submit_annotated_equals_prepare_annotated_then_submit():
    """PipelinedEval.submit_annotated, two batches in flight over three batches, against prepare_annotated followed by submit."""
    from conftest import synthetic_sd
    from keypointfusion_amd.model.model import KPFusion
    from keypointfusion_amd.preprocess_gpu import MODEL_INPUTS, DevicePreprocessor
    from keypointfusion_amd.serving import PipelinedEval
    dev = _dev()
    net = "KPFusion-convnext-tiny"
    m = KPFusion(net, "", 21, "dexycb", "")
    m.load_state_dict(synthetic_sd(net))
    m = m.to(dev).eval()
    pre = DevicePreprocessor(cube=AC.CUBE)
    S = AC.SMALL
    batches = [_batch([_host(S[(2 * i + j) % len(S)])[0] for j in range(2)], [50 + 2 * i, 51 + 2 * i]) for i in range(3)]
    pe = PipelinedEval(m, depth=2)
    with torch.no_grad(), torch.cuda.stream(pe.feed_stream(dev)):
        want = []
        for kw in batches:
            prep = pre.prepare_annotated(**kw)
            res, sws, _ = pe.collect(pe.submit(*[prep[k] for k in MODEL_INPUTS[:3]], None, *[prep[k] for k in MODEL_INPUTS[3:]]))
            want.append([t.clone() for t in res + sws] + list(pre.uncrop(res[5], prep)) + [prep["joint"].clone(), prep["joint_img"].clone()])
        tickets = [pe.submit_annotated(pre, **kw) for kw in batches]  # all enqueued before the first is collected
        got = []
        for ticket, keep in tickets:
            res, sws, _ = pe.collect(ticket)
            got.append(list(res + sws) + list(pre.uncrop(res[5], keep)) + [keep["joint"], keep["joint_img"]])
    torch.cuda.synchronize(dev)
    for g, w in zip(got, want):
        assert len(g) == len(w) == 12
        for a, c in zip(g, w):
            assert torch.equal(a, c)
