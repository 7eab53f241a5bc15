"""Device-resident tracking (keypointfusion_amd/tracking.py on kpf_track_step_f32 and kpf_prep_crop_u16_indexed of libkpf_hip.so) against the host: the
un-cropped pixels are the bits of kpf_prep_uncrop_f32, the camera-space joints the bits of the torch-CPU expression, the next box the bits of
`tracking.next_bbox` (which tests/test_tracking_host.py pins to the reference) of the device's own frame pixels, the status bits and the state what
include/kpf.h says; a sample does not depend on its batch; tracks that share a stored frame equal tracks on duplicated frames; and the loop of
`TrackedStream`, eager and as a replayed graph, follows the host path frame by frame with the analytic forward of tests/track_cases.py and with the model."""
import numpy as np
import pytest
import torch

import prep_cases as PC
import track_cases as TC
from keypointfusion_amd import lib as L
from keypointfusion_amd.tracking import next_bbox

pytestmark = pytest.mark.gpu
NAMES = list(PC.CASES)
J = 21
_FRAMES = {}


def _dev():
    return torch.device("cuda:0")


def _case(name):
    if name not in _FRAMES:
        _FRAMES[name] = PC.synth_frame(name)
    return _FRAMES[name]


def _batch(names, seeds):
    fr = [_case(n) for n in names]
    dev = _dev()
    return (torch.from_numpy(np.stack([f[0] for f in fr])).to(dev), torch.from_numpy(np.stack([f[1] for f in fr])).to(dev),
            torch.tensor([f[2] for f in fr], dtype=torch.float64, device=dev), torch.tensor([f[3] for f in fr], dtype=torch.float64, device=dev),
            torch.tensor(list(seeds), dtype=torch.int64, device=dev))


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def pre():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    return DevicePreprocessor(img_size=128, sample_num=1024, cube=PC.CUBE)


# ---- 1, 2: the kernel ---------------------------------------------------------------------------------------------------------------------------------

KINDS = ("good", "equal", "far", "nan")
EMPTY = ("empty", "background_wall")  # the cases of tests/prep_cases.py whose crop has no foreground


def _joints(kinds, seed):
    """[B][J][3] float32: random in [-1, 1]^3; `equal`: all joints one point; `far`: 40 cube half-sizes to the right of the crop (finite pixels far outside
    the frame); `nan`: one joint's u is NaN."""
    g = np.random.RandomState(seed)
    j = (g.rand(len(kinds), J, 3) * 2 - 1).astype(np.float32)
    for b, k in enumerate(kinds):
        if k == "equal":
            j[b] = j[b, 0]
        elif k == "far":
            j[b, :, 0] = 40.0 + 0.1 * j[b, :, 0]
        elif k == "nan":
            j[b, 7, 0] = np.nan
    return j


def _track(prep, joints, state, stride=5):
    """One kpf_track_step_f32 launch on a prepare() result.  state = (bbox, seed, lost) device tensors, updated in place.  Returns the outputs."""
    dev = _dev()
    B = joints.shape[0]
    out = dict(crop_px=torch.zeros(B, J, 3, device=dev), frame_px=torch.zeros(B, J, 3, device=dev), cam_mm=torch.zeros(B, J, 3, device=dev),
               bbox_used=torch.zeros(B, 4, dtype=torch.float64, device=dev), status=torch.full((B,), -1, dtype=torch.int32, device=dev))
    bbox, seed, lost = state
    L.check(L.load().kpf_track_step_f32(joints.data_ptr(), prep["center"].data_ptr(), prep["M"].data_ptr(), prep["cube"].data_ptr(), prep["cam_para"].data_ptr(),
                                        prep["pcl_count"].data_ptr(), B, J, 640, 480, 1.5, stride, bbox.data_ptr(), seed.data_ptr(), lost.data_ptr(),
                                        out["crop_px"].data_ptr(), out["frame_px"].data_ptr(), out["cam_mm"].data_ptr(), out["bbox_used"].data_ptr(),
                                        out["status"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "kpf_track_step_f32")
    torch.cuda.synchronize()
    return out


def _expect_status(frame_px, pcl_count):
    """(status, next box or None) of one sample by the rules of include/kpf.h, from the device's own frame pixels."""
    st = 2 if pcl_count == 0 else 0
    if not np.isfinite(frame_px[:, :2]).all():
        return st | 4, None
    nb = next_bbox(frame_px, 640, 480, 1.5)
    return (st | 1, None) if nb is None else (st, nb)


def _check_launch(pre, names, kinds, seed):
    dev = _dev()
    B = len(names)
    ins = _batch(names, range(B))
    prep = pre.prepare(*ins)
    joints = torch.from_numpy(_joints(kinds, seed)).to(dev)
    box0 = ins[2].clone()
    state = (ins[2].clone(), torch.arange(B, dtype=torch.int64, device=dev) * 1000, torch.full((B,), 3, dtype=torch.int32, device=dev))
    out = _track(prep, joints, state)
    want_c, want_f = pre.uncrop(joints, prep)
    assert np.array_equal(_bits(out["crop_px"]), _bits(want_c)) and np.array_equal(_bits(out["frame_px"]), _bits(want_f))
    good = [b for b, k in enumerate(kinds) if k != "nan"]
    assert torch.equal(out["crop_px"][good], want_c[good]) and torch.equal(out["frame_px"][good], want_f[good])
    cam_mm = joints.cpu() * prep["cube"].cpu().unsqueeze(1) / 2 + prep["center"].cpu().unsqueeze(1)  # demo_RGBD.py:133 on the CPU
    assert np.array_equal(out["cam_mm"].cpu().numpy(), cam_mm.numpy(), equal_nan=True)
    assert torch.equal(out["cam_mm"][good].cpu(), cam_mm[good])
    assert np.array_equal(_bits(out["bbox_used"]), _bits(box0))
    assert state[1].cpu().tolist() == [1000 * b + 5 for b in range(B)]
    fp, cnt, status = out["frame_px"].cpu().numpy(), prep["pcl_count"].cpu().numpy(), out["status"].cpu().numpy()
    newbox, lost = state[0].cpu().numpy(), state[2].cpu().numpy()
    for b, (name, kind) in enumerate(zip(names, kinds)):
        st, nb = _expect_status(fp[b], int(cnt[b]))
        assert int(status[b]) == st, (b, name, kind, status[b], st)
        assert ((st & 2) != 0) == (name in EMPTY), (name, st)
        if kind in ("equal", "far"):
            assert (st & ~2) == 1, (name, kind, st)
        elif kind == "nan":
            assert (st & ~2) == 4, (name, kind, st)
        else:
            assert (st & ~2) == 0, (name, kind, st)
        if st == 0:
            assert np.array_equal(newbox[b].view(np.int64), nb.view(np.int64)) and lost[b] == 0, (b, name, newbox[b], nb)
        else:
            assert np.array_equal(newbox[b].view(np.int64), box0[b].cpu().numpy().view(np.int64)) and lost[b] == 4, (b, name, kind)
    # lost counts up while a track stays bad, and returns to 0 on the next good frame
    out2 = _track(prep, joints, state)
    assert torch.equal(out2["status"], out["status"])
    assert state[2].cpu().tolist() == [0 if st == 0 else 5 for st in status]
    out3 = _track(prep, torch.from_numpy(_joints(["good"] * B, seed + 1)).to(dev), state)
    assert out3["status"].cpu().tolist() == [2 if n in EMPTY else 0 for n in names]
    assert state[2].cpu().tolist() == [(0 if st == 0 else 6) if n in EMPTY else 0 for n, st in zip(names, status)]
    assert state[1].cpu().tolist() == [1000 * b + 15 for b in range(B)]
    return status


@pytest.mark.parametrize("B", [1, 7, 32])
def test_kernel_matches_the_host_rule(pre, B):
    """Random joints on the prepare records of the mixed synthetic cases, with the crafted samples in the same launches: all joints equal and joints far
    outside the frame (status 1), the `empty` case (bit 2), one NaN joint (4).  The old box is kept bit for bit and `lost` counts."""
    if B == 1:
        seen = [int(_check_launch(pre, [n], [k], 11 + i)[0]) for i, (n, k) in enumerate(
            [("centre", "good"), ("centre", "equal"), ("fx_ne_fy", "far"), ("empty", "good"), ("corner", "nan"), ("empty", "nan")])]
        assert seen == [0, 1, 1, 2, 4, 6]
        return
    names = NAMES[:7] if B == 7 else [NAMES[(i * 3 + 1) % len(NAMES)] for i in range(B)]
    kinds = [KINDS[1 + (i // 2) % 3] if i % 2 else "good" for i in range(B)]
    status = _check_launch(pre, names, kinds, 20 + B)
    assert {0, 1, 4} <= set(int(s) & ~2 for s in status) and any(int(s) & 2 for s in status)


def test_a_sample_does_not_depend_on_its_batch(pre):
    """The same (frame, joints, state) alone and at positions 0, 13 and 31 of B = 32: every output and the state identical."""
    dev = _dev()
    for name, kind in (("centre", "good"), ("fx_ne_fy", "far"), ("empty", "nan")):
        one_j = _joints([kind], 5)
        ins1 = _batch([name], [9])
        prep1 = {k: v.clone() for k, v in pre.prepare(*ins1).items()}
        st1 = (ins1[2].clone(), torch.tensor([77], dtype=torch.int64, device=dev), torch.tensor([2], dtype=torch.int32, device=dev))
        o1 = _track(prep1, torch.from_numpy(one_j).to(dev), st1)
        names = [NAMES[i % len(NAMES)] for i in range(32)]
        kinds = [KINDS[i % 4] for i in range(32)]
        seeds = list(range(32))
        joints = _joints(kinds, 6)
        for pos in (0, 13, 31):
            names[pos], seeds[pos], joints[pos] = name, 9, one_j[0]
        ins = _batch(names, seeds)
        prep = pre.prepare(*ins)
        seed0 = torch.arange(32, dtype=torch.int64, device=dev)
        lost0 = torch.arange(32, dtype=torch.int32, device=dev)
        for pos in (0, 13, 31):
            seed0[pos], lost0[pos] = 77, 2
        st = (ins[2].clone(), seed0, lost0)
        o = _track(prep, torch.from_numpy(joints).to(dev), st)
        for pos in (0, 13, 31):
            for k in o:
                assert np.array_equal(_bits(o[k][pos]), _bits(o1[k][0])), (name, pos, k)
            for a, c in zip(st, st1):
                assert np.array_equal(_bits(a[pos]), _bits(c[0])), (name, pos)


# ---- 3: several tracks on one stored frame ------------------------------------------------------------------------------------------------------------

def test_tracks_on_shared_frames_equal_tracks_on_duplicated_frames(pre):
    from keypointfusion_amd.preprocess_gpu import make_frame_index
    dev = _dev()
    rgb2, depth2, _, _, _ = _batch(["centre", "fx_ne_fy"], [0, 0])
    index = [0, 1, 1, 0]
    rgb4, depth4, _, _, _ = _batch([("centre", "fx_ne_fy")[i] for i in index], [0] * 4)  # the same frames, stored once per track
    boxes = [_case("centre")[2], _case("fx_ne_fy")[2], [250.0, 150.0, 100.0, 110.0], [260.5, 180.25, 120.0, 120.0]]
    cams = [_case("centre")[3], _case("fx_ne_fy")[3], _case("fx_ne_fy")[3], _case("centre")[3]]
    bbox, cam = torch.tensor(boxes, dtype=torch.float64, device=dev), torch.tensor(cams, dtype=torch.float64, device=dev)
    seed = torch.tensor([3, 4, 5, 6], dtype=torch.int64, device=dev)
    dup = {k: v.clone() for k, v in pre.prepare(rgb4, depth4, bbox, cam, seed).items()}
    shared = pre.prepare(rgb2, depth2, bbox, cam, seed, frame_index=make_frame_index(index, 2, dev))
    torch.cuda.synchronize()
    assert set(shared) == set(dup) and int(dup["pcl_count"].min()) > 0
    for k in dup:
        assert torch.equal(shared[k], dup[k]), k
    assert not torch.equal(dup["img"][0], dup["img"][3])  # (same stored frame, another box: another crop)


# ---- 4 - 6: the loop ---------------------------------------------------------------------------------------------------------------------------------

_VIDEO = {}


def _video():
    if not _VIDEO:
        dev = _dev()
        fr = [TC.frame(t) for t in range(TC.FRAMES)]
        _VIDEO["host"] = fr
        _VIDEO["dev"] = [(torch.from_numpy(r[None]).to(dev), torch.from_numpy(d[None]).to(dev)) for r, d in fr]
    return _VIDEO


class AnalyticForward:
    """tests/track_cases.py's forward on the device: joints on a ring of 0.8 r around each disc's centre at frame `frame_no`, as joints normalised to the cube
    of the crop they are asked for.  Reads device memory only (frame_no is a device tensor), so it can be captured and replayed."""

    def __init__(self, dev):
        t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=dev)
        self.c0, self.vel = t([d[:2] for d, _ in TC.DISCS]), t([v for _, v in TC.DISCS])
        self.ring = t(TC.RING)[None] * t([0.8 * d[3] for d, _ in TC.DISCS]).view(2, 1, 1)  # [2][J][2]

    def __call__(self, prep, frame_no):
        px = (self.c0 + self.vel * frame_no.to(torch.float64)).unsqueeze(1) + self.ring
        center, cube, cam = prep["center"].double().unsqueeze(1), prep["cube"].double().unsqueeze(1), prep["cam_para"].double().unsqueeze(1)
        z = center[..., 2]
        x = (px[..., 0] - cam[..., 2]) * z / cam[..., 0]
        y = (px[..., 1] - cam[..., 3]) * z / cam[..., 1]
        return torch.stack([(x - center[..., 0]) / (cube[..., 0] / 2), (y - center[..., 1]) / (cube[..., 1] / 2), torch.zeros_like(x)], -1).float()


def _stream(graph, model=None, forward=None, pre=None):
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    from keypointfusion_amd.tracking import TrackedStream
    dev = _dev()
    cam = torch.tensor([TC.CAM, TC.CAM], dtype=torch.float64, device=dev)
    ts = TrackedStream(model, pre or DevicePreprocessor(img_size=128, sample_num=1024, cube=TC.CUBE), cam, frame_size=(TC.H, TC.W), frames=1,
                       frame_index=[0, 0], seed=40, graph=graph, forward=forward)
    ts.reseed(torch.tensor(TC.FIRST_BOX, dtype=torch.float64, device=dev))
    return ts


KEYS = ("frame_px", "crop_px", "cam_mm", "bbox_used", "bbox", "status", "lost", "com", "bounds", "pcl_count")


def _snapshot(out):
    torch.cuda.synchronize()
    assert set(KEYS) <= set(out)
    return {k: out[k].cpu().clone() for k in KEYS}


def _check_frame(s, t):
    """One frame's snapshot against the host path fed the DEVICE's box: bounds and count equal, com within 1e-12 relative, and the next box by the rule."""
    rgb, depth = _video()["host"][t]
    for k in range(2):
        used = [float(v) for v in s["bbox_used"][k]]
        h = PC.host_record(rgb, depth, used, TC.CAM)
        assert PC.floor_margin(h["com"], TC.CAM) >= 1e-6
        assert np.array_equal(s["bounds"][k, :4].numpy(), h["bounds"]) and np.array_equal(s["bounds"][k, 4:].numpy(), h["sz"])
        assert int(s["pcl_count"][k]) == len(h["candidates"])
        assert np.abs(s["com"][k].numpy() - h["com"]).max() <= 1e-12 * np.abs(h["com"]).max()
        st, nb = _expect_status(s["frame_px"][k].numpy(), int(s["pcl_count"][k]))
        assert int(s["status"][k]) == st
        want = nb if st == 0 else s["bbox_used"][k].numpy()
        assert np.array_equal(s["bbox"][k].numpy().view(np.int64), want.view(np.int64)), (t, k, s["bbox"][k], want)


def _run(ts, frames, between=None):
    shots = []
    for t in range(frames):
        if between is not None:
            between(ts, t)
        shots.append(_snapshot(ts.step(*_video()["dev"][t])))
    return shots


def test_analytic_loop_eager_and_graphed_follow_the_host():
    dev = _dev()
    eager = _run(_stream(False, forward=AnalyticForward(dev)), TC.FRAMES)
    ts = _stream(True, forward=AnalyticForward(dev))
    graphed = _run(ts, TC.FRAMES)
    assert ts.graph_replays == 8 and ts.frames_done == 10
    for t, (e, g) in enumerate(zip(eager, graphed)):
        _check_frame(e, t)
        for k in KEYS:
            assert torch.equal(e[k], g[k]), (t, k)
        assert e["status"].tolist() == [0, 0] and e["lost"].tolist() == [0, 0]
        for k in range(2):  # the forward's joints came back as the ring, and the centre of mass stayed on the disc
            assert np.abs(e["frame_px"][k, :, :2].numpy() - TC.ring_px(k, t)).max() < 1e-2
            assert np.abs(e["com"][k, :2].numpy() - TC.centre(k, t)).max() <= 1.5
        if t:
            assert torch.equal(e["bbox_used"], eager[t - 1]["bbox"])
    assert int(ts.seed[1]) == 41 + 2 * TC.FRAMES and int(ts.frame_no) == TC.FRAMES


def test_masked_reseed_between_replays_reaches_one_track():
    dev = _dev()
    fresh = torch.tensor([[0.0, 0.0, 1.0, 1.0], [TC.centre(1, 3)[0] - 70.0, TC.centre(1, 3)[1] - 70.0, 140.0, 140.0]], dtype=torch.float64, device=dev)
    mask = torch.tensor([False, True], device=dev)

    def between(ts, t):
        if t == 3:
            assert ts.graph_replays == 1  # frame 2 was the first replay: this write lands between two replays
            ts.reseed(fresh, mask)

    shots = _run(_stream(True, forward=AnalyticForward(dev)), 5, between)
    assert torch.equal(shots[3]["bbox_used"][1], fresh[1].cpu()) and not torch.equal(shots[2]["bbox"][1], fresh[1].cpu())
    assert torch.equal(shots[3]["bbox_used"][0], shots[2]["bbox"][0])  # the other track went on from its own box
    assert torch.equal(shots[4]["bbox_used"], shots[3]["bbox"])
    for t in (3, 4):
        _check_frame(shots[t], t)
        assert shots[t]["status"].tolist() == [0, 0]


def test_model_loop_eager_equals_graphed():
    """ConvNeXt-T with synthetic weights, B = 2 tracks on one frame, 5 frames.  The joints of untrained weights are arbitrary: this pins the pipeline — eager
    and graphed identical in every output of every frame, and every frame consistent with the host path and the rule — not accuracy."""
    from conftest import synthetic_sd
    from keypointfusion_amd.model.model import KPFusion
    net = "KPFusion-convnext-tiny"
    m = KPFusion(net, "", 21, "dexycb", "")
    m.load_state_dict(synthetic_sd(net))
    m = m.to(_dev()).eval()
    eager = _run(_stream(False, model=m), 5)
    ts = _stream(True, model=m)
    graphed = _run(ts, 5)
    assert ts.graph_replays == 3
    for t, (e, g) in enumerate(zip(eager, graphed)):
        for k in KEYS:
            assert np.array_equal(_bits(e[k]), _bits(g[k])), (t, k)
        _check_frame(e, t)
        assert e["frame_px"].shape == (2, 21, 3)
        if t:
            assert torch.equal(e["bbox_used"], eager[t - 1]["bbox"])
