"""CPU side of device-resident tracking (keypointfusion_amd/tracking.py, kpf_track_step_f32 and kpf_prep_crop_u16_indexed of include/kpf.h, ABI 21): the
host yardstick `next_bbox` equals the reference loader's box rule bit for bit (fixture tests/golden/track_bbox.npz, and the live reference where it is
present), the new entries are declared, exported and refuse bad arguments before any launch, and the analytic video of tests/track_cases.py is what
tests/test_tracking_gpu.py assumes: tracked on the host, the rule never loses the discs and no integer decision of the preprocessing sits on a rounding edge."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import prep_cases as PC
import track_cases as TC
from conftest import GOLDEN, ROOT
from keypointfusion_amd import lib as L
from keypointfusion_amd.tracking import next_bbox

NEW = ("kpf_track_step_f32", "kpf_prep_crop_u16_indexed")


def _same(got, want, valid):
    if not valid:
        return got is None
    return got is not None and got.dtype == np.float64 and np.array_equal(got.view(np.int64), np.asarray(want, np.float64).view(np.int64))


def test_next_bbox_equals_the_reference_fixture_bit_for_bit():
    z = np.load(os.path.join(GOLDEN, "track_bbox.npz"))
    joints, size, bbox, valid, e = z["joints"], z["size"], z["bbox"], z["valid"], float(z["expansion"])
    assert joints.shape == (512, 21, 2) and joints.dtype == np.float32 and bbox.dtype == np.float64
    assert 0.05 <= 1.0 - valid.mean() <= 0.20 and {tuple(s) for s in size} == {(640, 480), (1920, 1080)}
    bad = [i for i in range(len(joints)) if not _same(next_bbox(joints[i], int(size[i, 0]), int(size[i, 1]), e), bbox[i], valid[i])]
    assert not bad, bad[:10]


def test_next_bbox_equals_the_live_reference():
    import sys
    sys.path.insert(0, GOLDEN)
    import ref_import
    if not ref_import.reference_available():
        pytest.skip("reference tree not present")
    ref_import.load_reference()
    from dataloader.loader import HO3D
    g = np.random.RandomState(7)
    none = 0
    for i in range(2000):
        Wf, Hf = ((640, 480), (1920, 1080))[i % 2]
        c = np.array([g.uniform(-0.3 * Wf, 1.3 * Wf), g.uniform(-0.3 * Hf, 1.3 * Hf)])
        spread = g.uniform(0, 0.2 * Hf, 2) * (g.rand(2) > 0.05)  # now and then a line or a point
        j = (c + g.uniform(-1, 1, (21, 2)) * spread).astype(np.float32)
        want = HO3D.process_bbox(None, HO3D.get_bbox(None, j, 1.5), Wf, Hf, 1.0)
        none += want is None
        assert _same(next_bbox(j, Wf, Hf, 1.5), want if want is not None else np.zeros(4), want is not None), (i, j, want)
    assert 50 < none < 1000


def test_next_bbox_refuses_other_dtypes():
    with pytest.raises(ValueError, match="float32"):
        next_bbox(np.zeros((21, 2), np.float64), 640, 480)
    with pytest.raises(ValueError, match="float32"):
        next_bbox(np.zeros((21,), np.float32), 640, 480)


def test_new_entry_points_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), "%s is not declared in include/kpf.h" % name
        assert name in L.EXPORTS
        assert hasattr(raw, name), "libkpf_hip.so does not export %s" % name
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 21 and L.ABI_VERSION == abi and L.load().kpf_abi_version() == abi


def test_bad_arguments_fail_with_a_message_not_a_launch():
    """Null pointers, J > 64 and bad shapes return KPF_EINVAL before anything reaches a device."""
    l = L.load()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused by its argument checks

    def track(J=21, B=1, W=640, H=480, e=1.5, null=None):
        a = [p] * 6 + [B, J, W, H, e, 1] + [p] * 8 + [None]
        if null is not None:
            a[null] = None
        return l.kpf_track_step_f32(*a)

    def crop(F=2, B=4, idx=p, rgb=p, S=128):
        return l.kpf_prep_crop_u16_indexed(rgb, p, idx, F, p, p, p, B, 480, 640, 0, 0, 480, 640, S, p, p, p, p, p, p, p, p, p, None)

    calls = [(lambda i=i: track(null=i), "null") for i in (0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17, 18, 19)]
    calls += [(lambda: track(J=65), "J = 65"), (lambda: track(J=0), "bad shape"), (lambda: track(B=0), "bad shape"), (lambda: track(W=0), "bad shape"),
              (lambda: track(e=0.0), "expansion"), (lambda: track(e=float("nan")), "expansion"),
              (lambda: crop(idx=None), "null frame index"), (lambda: crop(rgb=None), "null pointer"), (lambda: crop(F=0), "0 stored frames"),
              (lambda: crop(S=129), "S = 129"), (lambda: crop(B=0), "bad shape")]
    for call, word in calls:
        assert l.kpf_inv3x3_f32(None, None, 0, 0, None) == -1  # another message in between
        rc = call()
        msg = l.kpf_last_error().decode()
        assert rc == -1 and word in msg and msg.startswith(NEW), (rc, word, msg)
    # the entry without an index keeps its name in its messages
    assert l.kpf_prep_crop_u16(None, p, p, p, p, 1, 480, 640, 0, 0, 480, 640, 128, p, p, p, p, p, p, p, p, p, None) == -1
    assert l.kpf_last_error().decode().startswith("kpf_prep_crop_u16: null")


def test_frame_index_is_checked_on_the_host():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor, make_frame_index
    fi = make_frame_index([0, 1, 1, 0], 2, "cpu")
    assert fi.dtype == torch.int32 and fi.tolist() == [0, 1, 1, 0]
    for bad in ([0, 2], [-1, 0], [5]):
        with pytest.raises(ValueError, match=r"outside \[0, 2\)"):
            make_frame_index(bad, 2, "cpu")
    for bad in ([], [0.5, 1], "ab", None, torch.zeros(2, dtype=torch.int32), 3):
        with pytest.raises(TypeError, match="host sequence of integers"):
            make_frame_index(bad, 2, "cpu")
    rgb, depth = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(2, 48, 64, dtype=torch.uint16)
    bbox, cam, seed = torch.zeros(4, 4, dtype=torch.float64), torch.ones(4, 4, dtype=torch.float64), torch.zeros(4, dtype=torch.int64)
    assert DevicePreprocessor.check_inputs(rgb, depth, bbox, cam, seed, frame_index=fi) == (4, 48, 64, 0, 0, 48, 64)
    assert DevicePreprocessor.check_inputs(rgb, depth, bbox[:2], cam[:2], seed[:2]) == (2, 48, 64, 0, 0, 48, 64)  # without an index: as before
    with pytest.raises(TypeError, match="frame_index must be torch.int32"):
        DevicePreprocessor.check_inputs(rgb, depth, bbox, cam, seed, frame_index=fi.long())
    with pytest.raises(TypeError, match="frame_index must be a torch tensor"):
        DevicePreprocessor.check_inputs(rgb, depth, bbox, cam, seed, frame_index=[0, 1, 1, 0])
    with pytest.raises(ValueError, match="frame_index has shape"):
        DevicePreprocessor.check_inputs(rgb, depth, bbox, cam, seed, frame_index=fi.view(2, 2))
    with pytest.raises(ValueError, match="bbox has shape"):
        DevicePreprocessor.check_inputs(rgb, depth, bbox[:2], cam, seed, frame_index=fi)  # B is the length of the index
    with pytest.raises(ValueError, match="does not match"):
        DevicePreprocessor.check_inputs(rgb[:1], depth, bbox, cam, seed, frame_index=fi)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DevicePreprocessor().prepare(rgb, depth, bbox, cam, seed, frame_index=fi)


def test_tracked_stream_refuses_bad_arguments_without_a_device():
    from keypointfusion_amd.tracking import TrackedStream
    cam = torch.ones(2, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="float64"):
        TrackedStream(None, None, cam.float(), (480, 640), 1, forward=lambda p, n: None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TrackedStream(None, None, cam, (480, 640), 1, frame_index=[0, 0], forward=lambda p, n: None)


def test_the_analytic_video_is_trackable_on_the_host():
    """The loop of tests/test_tracking_gpu.py on the host path: box -> prepare_rgbd -> analytic joints -> next_bbox, 10 frames, two discs in one frame.  The
    rule never returns None, the centre of mass stays on the disc, and every floor argument of com_to_bounds keeps its distance from an integer."""
    box = [np.array(b, np.float64) for b in TC.FIRST_BOX]
    worst, margin = 0.0, 1.0
    for t in range(TC.FRAMES):
        rgb, depth = TC.frame(t)
        for k in range(2):
            h = PC.host_record(rgb, depth, [float(v) for v in box[k]], TC.CAM)
            worst = max(worst, float(np.abs(h["com"][:2] - TC.centre(k, t)).max()))
            margin = min(margin, PC.floor_margin(h["com"], TC.CAM))
            assert len(h["candidates"]) > 1024
            nb = next_bbox(TC.ring_px(k, t), TC.W, TC.H)
            assert nb is not None and nb[2] == nb[3] and abs(nb[2] - 1.5 * 1.6 * TC.DISCS[k][0][3]) < 2.0, (t, k, nb)
            box[k] = nb
    print("com - disc centre: %.3f px; floor margin %.3g" % (worst, margin))
    assert worst <= 1.5
    assert margin >= 1e-6
