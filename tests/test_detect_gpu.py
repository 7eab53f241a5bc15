"""The hand detector's kernels (keypointfusion_amd/detect.py::HandDetector on kpf_detect_hands_u16 and kpf_detect_assign_f64 of libkpf_hip.so, DESIGN.md
4.21) against detect.detect_hands_host and detect.assign_host: every output word equal at every pixel, with no tolerance and nothing left out; frames of a
batch independent; a second call on the same buffers the same bits; a captured and replayed sequence equal to the eager one; and
TrackedStream(detector=...), never given a box, eager and graphed, equal to a plain stream reseeded by hand with the host detector's boxes."""
import numpy as np
import pytest
import torch

import detect_cases as DC
import track_cases as TC
from keypointfusion_amd import detect as D

pytestmark = pytest.mark.gpu
OUT = ("boxes", "valid", "info", "labels", "stats")
_HOST = {}


def _dev():
    return torch.device("cuda:0")


def _host(name):
    if name not in _HOST:
        depth, cam, params = DC.build(name)
        _HOST[name] = D.detect_hands_host(depth, cam, **params)
    return _HOST[name]


def _np(out):
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy().copy() for k in OUT}


def _same(got, want, what):
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k, np.argwhere(got[k] != want[k])[:8].tolist())


def _device(depth, cam, params):
    det = D.HandDetector(cam, depth.shape[1:], _dev(), **params)
    return _np(det.detect(torch.from_numpy(depth).to(_dev()))), det


@pytest.mark.parametrize("name", list(DC.CASES))
def test_kernels_give_the_host_rules_words(name):
    depth, cam, params = DC.build(name)
    got, _ = _device(depth, cam, params)
    print(name, got["stats"].tolist(), got["valid"].tolist())
    _same(got, _host(name), name)


@pytest.mark.parametrize("slots", [1, 8])
def test_fewer_and_more_slots_than_candidates(slots):
    for name in ("many", "random", "step"):
        depth, cam, params = DC.build(name)
        params = dict(params, slots=slots)
        got, _ = _device(depth, cam, params)
        _same(got, D.detect_hands_host(depth, cam, **params), (name, slots))


def test_frames_of_a_batch_are_independent():
    depth, cam, params = DC.build("ragged_three")
    got, _ = _device(depth, cam, params)
    for f in range(3):
        one, _ = _device(depth[f:f + 1], cam[f:f + 1], params)
        for k in OUT:
            assert np.array_equal(one[k][0].view(np.uint8), got[k][f].view(np.uint8)), (f, k)
    assert len({tuple(s) for s in got["stats"].tolist()}) == 3


def test_a_second_call_on_the_same_buffers_gives_the_same_bits():
    """every word a call reads it has written itself: the call before leaves no trace, also behind an empty frame and behind another scene"""
    depth, cam, params = DC.build("random")
    other = DC.build("comb")[0]
    dev = _dev()
    det = D.HandDetector(cam, depth.shape[1:], dev, **params)
    x, y, zero = torch.from_numpy(depth).to(dev), torch.from_numpy(other).to(dev), torch.zeros(depth.shape, dtype=torch.int16, device=dev).view(torch.uint16)
    first, again = _np(det.detect(x)), _np(det.detect(x))
    empty = _np(det.detect(zero))
    third = _np(det.detect(x))
    comb = _np(det.detect(y))
    fourth = _np(det.detect(x))
    _same(first, _host("random"), "first")
    for what, o in (("again", again), ("after the empty frame", third), ("after another scene", fourth)):
        _same(o, first, what)
    assert not empty["stats"].any() and not empty["valid"].any() and (empty["labels"] == -1).all() and not empty["boxes"].any()
    _same(comb, D.detect_hands_host(other, cam, **params), "comb")


def test_a_captured_sequence_equals_the_eager_one():
    depth, cam, params = DC.build("ragged_three")
    dev = _dev()
    frames = [torch.from_numpy(np.ascontiguousarray(np.roll(depth, s, axis=0))).to(dev) for s in range(3)]  # the scenes change places
    want = [D.detect_hands_host(np.roll(depth, s, axis=0), cam, **params) for s in range(3)]
    eager_det = D.HandDetector(cam, depth.shape[1:], dev, **params)
    for t, x in enumerate(frames):
        _same(_np(eager_det.detect(x)), want[t], ("eager", t))
    det = D.HandDetector(cam, depth.shape[1:], dev, **params)
    static = torch.zeros(depth.shape, dtype=torch.int16, device=dev).view(torch.uint16)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        static.copy_(frames[0])
        o = det.detect(static)  # the first call, eager
        ptrs = [o[k].data_ptr() for k in OUT]
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            o2 = det.detect(static)
        assert [o2[k].data_ptr() for k in OUT] == ptrs
        for t, x in enumerate(frames):
            static.copy_(x)
            g.replay()
            stream.synchronize()
            _same({k: o2[k].cpu().numpy() for k in OUT}, want[t], ("replay", t))
    torch.cuda.synchronize()


# ---- the assignment ---------------------------------------------------------------------------------------------------------------------------------------

def _assign_case(seed, F, K, B):
    """random slots and tracks: boxes around random centroids, about a third of the tracks live on a slot, a third free, the rest live elsewhere"""
    g = np.random.RandomState(seed)
    valid = (g.rand(F, K) < 0.7).astype(np.int32)
    info = np.zeros((F, K, 8))
    info[:, :, 5], info[:, :, 6] = g.rand(F, K) * 600 + 20, g.rand(F, K) * 440 + 20
    boxes = np.concatenate([info[:, :, 5:7] - 20.0, np.full((F, K, 2), 40.0)], -1) * valid[:, :, None]
    index = g.randint(0, F, B).astype(np.int32)
    bbox = g.rand(B, 4) * 100
    for b in range(B):
        if g.rand() < 0.4:  # stand on a slot of the own frame; some exactly at the half-open edges
            k = g.randint(K)
            u, v = info[index[b], k, 5:7]
            bbox[b] = [(u - 30, v - 30, 60, 60), (u, v, 5, 5), (u - 5, v - 5, 5, 5)][g.randint(3)]
    return boxes, valid, info, index, bbox, g.randint(0, 5, B).astype(np.int32), (g.rand(B) < 0.7).astype(np.int32)


@pytest.mark.parametrize("F,K,B,reseed_after", [(1, 4, 2, 3), (1, 1, 5, 1), (3, 4, 9, 2), (32, 8, 64, 3), (2, 8, 3, 4)])
def test_the_assignment_equals_the_host_rule(F, K, B, reseed_after):
    dev = _dev()
    det = D.HandDetector(np.tile(np.array([600.0, 600.0, 320.0, 240.0], np.float32), (F, 1)), (30, 40), dev, slots=K)  # (its frames are not read here)
    for seed in range(4):
        boxes, valid, info, index, bbox, lost, seeded = _assign_case(100 * F + seed, F, K, B)
        want = D.assign_host(boxes, valid, info, (30, 40), index, bbox, lost, seeded, reseed_after)
        det.boxes.copy_(torch.from_numpy(boxes))
        det.valid.copy_(torch.from_numpy(valid))
        det.info.copy_(torch.from_numpy(info))
        t = [torch.from_numpy(a.copy()).to(dev) for a in (index, bbox, lost, seeded)] + [torch.full((B,), -5, dtype=torch.int32, device=dev)]
        det.assign(*t, reseed_after)
        torch.cuda.synchronize()
        for name, got, w in zip(("bbox", "lost", "seeded", "reseeded"), t[1:], want):
            assert np.array_equal(got.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (seed, name, got.cpu().numpy().tolist(), w.tolist())


# ---- TrackedStream(detector=...) ------------------------------------------------------------------------------------------------------------------------

KEYS = ("frame_px", "crop_px", "cam_mm", "bbox_used", "bbox", "status", "lost", "com", "bounds", "pcl_count")
_VIDEO = {}


def _video():
    if not _VIDEO:
        fr = [TC.frame(t) for t in range(TC.FRAMES)]
        _VIDEO["rgb"] = [torch.from_numpy(r[None]).to(_dev()) for r, _ in fr]
        _VIDEO["depth"] = [torch.from_numpy(d[None]).to(_dev()) for _, d in fr]
        _VIDEO["depth_host"] = [d for _, d in fr]
        _VIDEO["host0"] = D.detect_hands_host(fr[0][1], np.array(TC.CAM, np.float32))
    return _VIDEO


class AnalyticForward:
    """tests/track_cases.py's forward on the device, as tests/test_tracking_gpu.py has it: joints on a ring of 0.8 r around each disc's centre at frame
    `frame_no`, normalised to the cube of the crop they are asked for.  Reads device memory only, so it can be captured and replayed."""

    def __init__(self, dev):
        t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=dev)  # noqa: E731
        self.c0, self.vel = t([d[:2] for d, _ in TC.DISCS]), t([v for _, v in TC.DISCS])
        self.ring = t(TC.RING)[None] * t([0.8 * d[3] for d, _ in TC.DISCS]).view(2, 1, 1)  # [2][J][2]

    def __call__(self, prep, frame_no):
        px = (self.c0 + self.vel * frame_no.to(torch.float64)).unsqueeze(1) + self.ring
        center, cube, cam = prep["center"].double().unsqueeze(1), prep["cube"].double().unsqueeze(1), prep["cam_para"].double().unsqueeze(1)
        z = center[..., 2]
        x = (px[..., 0] - cam[..., 2]) * z / cam[..., 0]
        y = (px[..., 1] - cam[..., 3]) * z / cam[..., 1]
        return torch.stack([(x - center[..., 0]) / (cube[..., 0] / 2), (y - center[..., 1]) / (cube[..., 1] / 2), torch.zeros_like(x)], -1).float()


def _stream(graph, detector, reseed_after=2):
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    from keypointfusion_amd.tracking import TrackedStream
    dev = _dev()
    cam = torch.tensor([TC.CAM, TC.CAM], dtype=torch.float64, device=dev)
    det = D.HandDetector(np.array([TC.CAM], np.float32), (TC.H, TC.W), dev) if detector else None
    return TrackedStream(None, DevicePreprocessor(img_size=128, sample_num=1024, cube=TC.CUBE), cam, frame_size=(TC.H, TC.W), frames=1, frame_index=[0, 0],
                         seed=40, graph=graph, forward=AnalyticForward(dev), detector=det, reseed_after=reseed_after)


def _run(ts, frames, depth_of=None):
    v = _video()
    shots = []
    for t in range(frames):
        out = ts.step(v["rgb"][t], v["depth"][t] if depth_of is None else depth_of(t))
        torch.cuda.synchronize()
        assert ("detections" in out) == (ts.detector is not None) == ("reseeded" in out) == ("seeded" in out)
        shot = {k: out[k].cpu().clone() for k in KEYS}
        if ts.detector is not None:
            shot.update(reseeded=out["reseeded"].cpu().clone(), seeded=out["seeded"].cpu().clone(),
                        detections={k: out["detections"][k].cpu().numpy().copy() for k in OUT})
        shots.append(shot)
    return shots


def test_a_stream_starts_without_a_box_from_outside():
    """the analytic video with the analytic forward: a stream with a detector that is never given a box seeds both tracks on frame 0 and then equals, bit
    for bit, a plain stream reseeded by hand with the host detector's boxes; eager equals graphed"""
    v = _video()
    assert v["host0"]["valid"][0].tolist() == [1, 1, 0, 0]
    plain = _stream(False, False)
    plain.reseed(torch.from_numpy(v["host0"]["boxes"][0, :2].copy()).to(_dev()))
    want = _run(plain, TC.FRAMES)
    eager = _run(_stream(False, True), TC.FRAMES)
    ts = _stream(True, True)
    graphed = _run(ts, TC.FRAMES)
    assert ts.graph_replays == TC.FRAMES - 2 and ts.frames_done == TC.FRAMES
    for t in range(TC.FRAMES):
        for shots in (eager, graphed):
            s = shots[t]
            assert s["status"].tolist() == [0, 0] and s["lost"].tolist() == [0, 0] and s["seeded"].tolist() == [1, 1], (t, s["status"], s["lost"])
            assert s["reseeded"].tolist() == ([1, 1] if t == 0 else [0, 0]), (t, s["reseeded"])
            for k in KEYS:
                assert np.array_equal(s[k].numpy().view(np.uint8), want[t][k].numpy().view(np.uint8)), (t, k)
        for k in OUT:
            assert np.array_equal(eager[t]["detections"][k].view(np.uint8), graphed[t]["detections"][k].view(np.uint8)), (t, k)
        assert int(want[t]["pcl_count"].min()) > 0
    _same(eager[0]["detections"], v["host0"], "frame 0")
    _same(eager[7]["detections"], D.detect_hands_host(v["depth_host"][7], np.array(TC.CAM, np.float32)), "frame 7")


def test_a_lost_track_is_seeded_again_and_the_other_is_undisturbed():
    """the second disc vanishes from the depth of frames 3 .. 5: its track's `lost` rises, it is free from lost = 2 on, finds nothing while the disc is
    away, and takes the disc's slot the frame it returns; the first track's outputs are those of the undisturbed stream throughout"""
    v = _video()
    gone = (3, 4, 5)

    def depth_of(t):
        if t not in gone:
            return v["depth"][t]
        d = v["depth_host"][t].copy()
        d[d > 650] = 0  # the 700 mm disc (665 .. 735 mm); the 600 mm one ends at 635
        return torch.from_numpy(d[None]).to(_dev())

    calm = _run(_stream(False, True), TC.FRAMES)
    for graph in (False, True):
        shots = _run(_stream(graph, True), TC.FRAMES, depth_of)
        for t in range(TC.FRAMES):
            s = shots[t]
            for k in KEYS:  # track 0 never notices
                assert np.array_equal(s[k][:1].numpy().view(np.uint8), calm[t][k][:1].numpy().view(np.uint8)), (graph, t, k)
            if t in gone:
                assert int(s["status"][1]) != 0 and int(s["lost"][1]) == t - 2 and int(s["reseeded"][1]) == 0, (graph, t, s["status"], s["lost"])
                assert s["detections"]["valid"][0].tolist() == [1, 0, 0, 0]
                assert torch.equal(s["bbox"][1], shots[2]["bbox"][1])  # the box stays what it was
            else:
                assert int(s["status"][1]) == 0 and int(s["lost"][1]) == 0, (graph, t, s["status"], s["lost"])
            assert int(s["reseeded"][1]) == (1 if t in (0, 6) else 0) and int(s["reseeded"][0]) == (1 if t == 0 else 0), (graph, t, s["reseeded"])
        back = D.detect_hands_host(v["depth_host"][6], np.array(TC.CAM, np.float32))
        assert np.array_equal(shots[6]["bbox_used"][1].numpy(), back["boxes"][0, 1])  # frame 6 was cropped with the returned disc's slot


def test_a_stream_refuses_a_detector_of_other_frames():
    from keypointfusion_amd.tracking import TrackedStream
    dev = _dev()
    cam = torch.zeros(1, 4, dtype=torch.float64, device=dev)
    one = np.array([TC.CAM], np.float32)
    for det in (D.HandDetector(one, (TC.H, TC.W + 1), dev), D.HandDetector(np.concatenate([one, one]), (TC.H, TC.W), dev)):
        with pytest.raises(ValueError):
            TrackedStream(None, None, cam, (TC.H, TC.W), 1, forward=lambda p, n: None, detector=det)
    with pytest.raises(ValueError):
        TrackedStream(None, None, cam, (TC.H, TC.W), 1, forward=lambda p, n: None, detector=D.HandDetector(one, (TC.H, TC.W), dev), reseed_after=0)
    ts = TrackedStream(None, None, cam, (TC.H, TC.W), 1, forward=lambda p, n: None)  # no detector: no tensor and no output of its
    assert ts.detector is None and ts.seeded is None and ts.reseeded is None
