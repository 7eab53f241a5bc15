"""CPU side of the hand detector (keypointfusion_amd/detect.py, kpf_detect_hands_u16 and kpf_detect_assign_f64 of include/kpf.h, ABI 36):
the numpy restatement on miniatures whose labels, counts and ranks are written out here; its labelling against a second, independent one (a sequential
union-find) in shuffled union orders on every scene of tests/detect_cases.py; the assignment rule; the refusals; the interface; the analytic video's two
discs; and csrc/kpf_detect_uf.h -- the kernels' own find, union and key packing -- compiled for the host with the sanitizers and driven over the scenes."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import detect_cases as DC
import track_cases as TC
from keypointfusion_amd import detect as D
from keypointfusion_amd import lib as L
from keypointfusion_amd.tracking import check_detector, next_bbox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kpf_detect_hands_u16", "kpf_detect_assign_f64")


# ---- the rule on miniatures ---------------------------------------------------------------------------------------------------------------------------

MINI = np.array([[10, 11, 0, 20, 20, 0],
                 [0, 12, 0, 0, 23, 0],
                 [5, 0, 50, 0, 22, 0],
                 [5, 6, 0, 51, 21, 0]], np.uint16)
MINI_PARAMS = dict(near=1, far=100, step_mm=2, reach_mm=3, min_pixels=2, min_area_mm2=0.0, max_area_mm2=1e9, slots=2)
UNIT_CAM = np.array([[1.0, 1.0, 0.0, 0.0]], np.float32)  # fx fy = 1: area_mm2 = S2


def test_a_miniature_by_hand():
    """Six components: A {10, 11, 12} label 0; B {20, 20} label 3 (20 | 23 is a step of 3 > 2); C {23, 22, 21} label 10; D {5, 5, 6} label 12; the single
    pixels 50 (label 14) and 51 (label 21) touch only diagonally and are dropped (min_pixels 2).  Ranked by z_min: D (5), A (10), B (20), C (21); two slots."""
    o = D.detect_hands_host(MINI, UNIT_CAM, **MINI_PARAMS)
    assert o["labels"].dtype == np.int32 and o["stats"].dtype == np.int32 and o["valid"].dtype == np.int32 and o["boxes"].dtype == np.float64
    assert o["labels"][0].tolist() == [[0, 0, -1, 3, 3, -1], [-1, 0, -1, -1, 10, -1], [12, -1, -1, -1, 10, -1], [12, 12, -1, -1, 10, -1]]
    assert o["stats"].tolist() == [[13, 6, 4, 4, 2]]
    assert o["valid"].tolist() == [[1, 1]]
    # label, z_min, n, slab, area = S2, centroid u, v, d
    assert o["info"][0, 0].tolist() == [12.0, 5.0, 3.0, 3.0, 25.0 + 25.0 + 36.0, 1.0 / 3.0, 8.0 / 3.0, 16.0 / 3.0]
    assert o["info"][0, 1].tolist() == [0.0, 10.0, 3.0, 3.0, 100.0 + 121.0 + 144.0, 2.0 / 3.0, 1.0 / 3.0, 11.0]
    for k, (lo, hi) in enumerate((((0, 2), (1, 3)), ((0, 0), (1, 1)))):  # the slab's pixel bounds -> the tracker's box rule
        want = next_bbox(np.array([lo, hi], np.float32), 6, 4, 1.25)
        assert want is not None and np.array_equal(o["boxes"][0, k], want)
    all4 = D.detect_hands_host(MINI, UNIT_CAM, **dict(MINI_PARAMS, slots=4))
    assert all4["info"][0, :, 0].tolist() == [12.0, 0.0, 3.0, 10.0] and all4["info"][0, :, 1].tolist() == [5.0, 10.0, 20.0, 21.0]
    assert all4["stats"].tolist() == [[13, 6, 4, 4, 4]]
    gated = D.detect_hands_host(MINI, UNIT_CAM, **dict(MINI_PARAMS, slots=4, min_area_mm2=86.0, max_area_mm2=800.0))  # B's S2 = 800, C's 1454
    assert gated["info"][0, :, 0].tolist() == [12.0, 0.0, 3.0, -1.0] and gated["stats"].tolist() == [[13, 6, 4, 3, 3]]


def test_a_near_slab_is_a_strict_part_of_a_ramp():
    """two rows of 10 12 14 16 18: one component of 10 pixels, z_min 10, reach 3 -> the slab is the four pixels at 10 and 12"""
    ramp = np.array([[10, 12, 14, 16, 18]] * 2, np.uint16)
    o = D.detect_hands_host(ramp, UNIT_CAM, **dict(MINI_PARAMS, slots=1))
    assert o["labels"][0].tolist() == [[0] * 5] * 2 and o["stats"].tolist() == [[10, 1, 1, 1, 1]]
    assert o["info"][0, 0].tolist() == [0.0, 10.0, 10.0, 4.0, 2 * (100.0 + 144.0), 0.5, 0.5, 11.0]
    assert np.array_equal(o["boxes"][0, 0], next_bbox(np.array([[0, 0], [1, 1]], np.float32), 5, 2, 1.25)) and o["valid"].tolist() == [[1]]
    one_row = D.detect_hands_host(ramp[:1], UNIT_CAM, **dict(MINI_PARAMS, slots=1))  # a slab one pixel high: the box rule gives None, the slot is invalid
    assert one_row["valid"].tolist() == [[0]] and not one_row["boxes"].any() and one_row["info"][0, 0, :4].tolist() == [0.0, 10.0, 5.0, 2.0]
    assert one_row["stats"].tolist() == [[5, 1, 1, 1, 1]]


def test_the_scenes_are_what_their_names_say():
    out = {n: D.detect_hands_host(*DC.build(n)[:2], **DC.build(n)[2]) for n in DC.CASES}
    st = {n: o["stats"].tolist() for n, o in out.items()}
    assert st["empty"] == [[0, 0, 0, 0, 0]] and (out["empty"]["labels"] == -1).all()
    for name in ("full", "serpentine", "spiral", "u", "comb", "arm"):  # ONE component, labelled by its first pixel
        depth = DC.build(name)[0]
        n = int((depth > 0).sum())
        assert st[name] == [[n, 1, 1, 1, 1]], (name, st[name])
        assert np.array_equal(out[name]["labels"][0] >= 0, depth[0] > 0) and len(set(out[name]["labels"][0][depth[0] > 0].tolist())) == 1
    assert st["checkerboard"] == [[1750, 1750, 0, 0, 0]] and (out["checkerboard"]["labels"] == -1).all()
    assert st["diagonal"] == [[200, 2, 2, 2, 2]] and out["diagonal"]["info"][0, :2, 0].tolist() == [22.0 * 70 + 22, 32.0 * 70 + 32]
    assert out["four_edges"]["info"][0, :2, :3].tolist() == [[20.0 * 70 + 30, 450.0, 100.0], [0.0, 600.0, 236.0]]
    assert out["step"]["info"][0, :, :3].tolist() == [[5.0 * 70 + 12, 500.0, 400.0], [5.0 * 70 + 32, 541.0, 200.0], [22.0 * 70 + 50, 600.0, 200.0],
                                                      [42.0 * 70 + 50, 641.0, 70.0]]
    assert st["bounds"] == [[128, 2, 2, 2, 2]] and out["bounds"]["info"][0, :2, 1].tolist() == [171.0, 1500.0]
    assert out["equal_zmin"]["info"][0, :3, :2].tolist() == [[36.0 * 70 + 28, 470.0], [3.0 * 70 + 50, 500.0], [20.0 * 70 + 5, 500.0]]
    assert st["many"] == [[600, 6, 6, 5, 4]] and out["many"]["info"][0, :, 1].tolist() == [500.0, 600.0, 700.0, 800.0]
    assert st["area_gate"] == [[960, 4, 4, 2, 2]] and out["area_gate"]["info"][0, :2, 4].tolist() == [2000.0, 40000.0]
    assert out["arm"]["info"][0, 0, 2:4].tolist() == [1080.0, 372.0]
    assert st["random"][0][1] > 500 and st["random"][0][2] > 20 and st["random"][0][3] >= 2
    assert st["thin_row"] == [[187, 2, 2, 2, 2]] and out["thin_row"]["valid"].tolist() == [[0, 0, 0, 0]]
    assert st["ragged_three"] == [st["four_edges"][0], [0, 0, 0, 0, 0], st["step"][0]]


@pytest.mark.parametrize("name", list(DC.CASES))
def test_the_labelling_does_not_depend_on_the_route_or_the_union_order(name):
    depth, cam, params = DC.build(name)
    p = D.check_params(**params)
    want = D.detect_hands_host(depth, cam, **params)
    for order in (None, "reversed", 1, 2, 3):
        for f in range(depth.shape[0]):
            a = D.label_propagate_host(depth[f], p["near"], p["far"], p["step_mm"])
            b = D.label_union_host(depth[f], p["near"], p["far"], p["step_mm"], order)
            assert np.array_equal(a, b), (name, order, f)
        got = D.detect_hands_host(depth, cam, labeller=lambda d, n, fa, s: D.label_union_host(d, n, fa, s, order), **params)
        for k in want:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (name, order, k)


def test_the_discs_of_the_analytic_video_are_the_two_slots():
    """tests/track_cases.py's frame 0 with the defaults: the 600 mm disc first, the 700 mm disc second, each box around its disc"""
    o = D.detect_hands_host(TC.frame(0)[1], np.array(TC.CAM, np.float32))
    assert o["stats"][0, 1:].tolist() == [2, 2, 2, 2] and o["valid"].tolist() == [[1, 1, 0, 0]]
    assert o["info"][0, 0, 1] < o["info"][0, 1, 1]
    for k, ((cx, cy, z, r), _) in enumerate(TC.DISCS):
        x, y, w, h = o["boxes"][0, k]
        assert x <= cx - r + 1 and y <= cy - r + 1 and x + w >= cx + r - 1 and y + h >= cy + r - 1, (k, o["boxes"][0, k])
        assert abs(o["info"][0, k, 5] - cx) < 1.0 and abs(o["info"][0, k, 6] - cy) < 1.0 and abs(o["info"][0, k, 7] - z) < 10.0


# ---- the assignment ---------------------------------------------------------------------------------------------------------------------------------------

def _slots(centres, size=40.0, F=1, K=4):
    """slots of frame 0: a valid slot of `size` pixels around every centre, in rank order"""
    boxes, valid, info = np.zeros((F, K, 4)), np.zeros((F, K), np.int32), np.zeros((F, K, 8))
    info[:, :, 0] = -1
    for k, (u, v) in enumerate(centres):
        boxes[0, k], valid[0, k], info[0, k] = (u - size / 2, v - size / 2, size, size), 1, (k, 500 + k, 100, 100, 5000, u, v, 510)
    return boxes, valid, info


def test_assign_free_and_live_tracks():
    boxes, valid, info = _slots([(100, 100), (300, 200), (500, 300)])
    live_box = [280.0, 180.0, 40.0, 40.0]  # holds slot 1's centroid
    bbox = np.array([[0, 0, 0, 0], live_box, [9, 9, 9, 9], [1, 2, 3, 4]], np.float64)
    # track 0 never seeded; track 1 live on slot 1; track 2 seeded but lost for 3 frames; track 3 seeded, lost 2 < reseed_after: live, on nothing
    nb, lost, seeded, reseeded = D.assign_host(boxes, valid, info, (480, 640), [0, 0, 0, 0], bbox, [0, 0, 3, 2], [0, 1, 1, 1], 3)
    assert nb.tolist() == [boxes[0, 0].tolist(), live_box, boxes[0, 2].tolist(), [1, 2, 3, 4]]
    assert lost.tolist() == [0, 0, 0, 2] and seeded.tolist() == [1, 1, 1, 1] and reseeded.tolist() == [1, 0, 1, 0]
    # the box is half open: a centroid on the right or lower edge is outside
    edge = np.array([[0, 0, 0, 0], [260.0, 160.0, 40.0, 40.0]], np.float64)
    nb, lost, seeded, reseeded = D.assign_host(boxes, valid, info, (480, 640), [0, 0], edge, [0, 0], [0, 1], 3)
    assert nb[0].tolist() == boxes[0, 0].tolist() and reseeded.tolist() == [1, 0]
    edge[1] = [300.0, 200.0, 40.0, 40.0]  # x <= u and y <= v: inside
    two = D.assign_host(boxes[:, 1:2], valid[:, 1:2], info[:, 1:2], (480, 640), [0, 0], edge, [0, 0], [0, 1], 3)
    assert two[0][0].tolist() == [0.0, 0.0, 640.0, 480.0] and two[3].tolist() == [0, 0]


def test_assign_more_free_tracks_than_slots_and_the_whole_frame_box():
    boxes, valid, info = _slots([(100, 100)])
    bbox = np.array([[7, 7, 7, 7]] * 3, np.float64)
    nb, lost, seeded, reseeded = D.assign_host(boxes, valid, info, (480, 640), [0, 0, 0], bbox, [5, 0, 9], [1, 0, 1], 2)
    # track 0 (seeded, lost) takes the slot; track 1 (never seeded) holds the whole frame and stays unseeded; track 2 (seeded, lost) keeps its box and count
    assert nb.tolist() == [boxes[0, 0].tolist(), [0.0, 0.0, 640.0, 480.0], [7.0, 7.0, 7.0, 7.0]]
    assert lost.tolist() == [0, 0, 9] and seeded.tolist() == [1, 0, 1] and reseeded.tolist() == [1, 0, 0]
    assert bbox.tolist() == [[7, 7, 7, 7]] * 3  # (the inputs are not written)


def test_assign_keeps_the_frames_apart_and_skips_invalid_slots():
    boxes, valid, info = _slots([(100, 100), (300, 200)], F=2)
    boxes[1, 0], valid[1, 0], info[1, 0] = (10, 10, 20, 20), 1, (0, 400, 90, 90, 3000, 20, 20, 410)
    valid[0, 0] = 0  # frame 0's first slot has no box: the second is the first to hand out
    bbox = np.zeros((4, 4))
    bbox[3] = [0, 0, 640, 480]  # a live track on frame 0 over everything
    nb, lost, seeded, reseeded = D.assign_host(boxes, valid, info, (480, 640), [1, 0, 1, 0], bbox, [0, 0, 0, 0], [0, 0, 0, 1], 3)
    assert nb.tolist() == [boxes[1, 0].tolist(), [0.0, 0.0, 640.0, 480.0], [0.0, 0.0, 640.0, 480.0], [0.0, 0.0, 640.0, 480.0]]
    assert seeded.tolist() == [1, 0, 0, 1] and reseeded.tolist() == [1, 0, 0, 0]


# ---- refusals and the interface ---------------------------------------------------------------------------------------------------------------------------

def test_the_host_rule_and_the_detector_refuse_bad_arguments():
    import torch
    cam = np.array([600.0, 600.0, 320.0, 240.0], np.float32)
    depth = np.zeros((1, 4, 4), np.uint16)
    bad_params = (dict(slots=0), dict(slots=9), dict(near=200, far=100), dict(near=-1), dict(far=65536), dict(step_mm=-1), dict(reach_mm=70000),
                  dict(min_pixels=0), dict(min_area_mm2=5.0, max_area_mm2=4.0), dict(min_area_mm2=float("nan")), dict(max_area_mm2=float("inf")),
                  dict(expansion=0.0), dict(expansion=-1.0), dict(near=1.5))
    for kw in bad_params:
        with pytest.raises(ValueError):
            D.detect_hands_host(depth, cam, **kw)
        with pytest.raises(ValueError):
            D.HandDetector(cam, (4, 4), torch.device("cuda:0"), **kw)
    with pytest.raises(TypeError):
        D.detect_hands_host(depth, cam, nearest=3)
    for c in ([0.0, 600.0, 1, 1], [600.0, -1.0, 1, 1], [600.0, float("nan"), 1, 1], [600.0, 600.0, float("inf"), 1], [600.0, 600.0, 1], np.ones((33, 4))):
        with pytest.raises(ValueError):
            D.HandDetector(np.asarray(c, np.float32), (4, 4), torch.device("cuda:0"))
    with pytest.raises(ValueError):
        D.detect_hands_host(depth.astype(np.int32), cam)
    with pytest.raises(ValueError):
        D.detect_hands_host(depth, np.stack([cam, cam]))
    with pytest.raises(ValueError):
        D.HandDetector(cam, (4097, 4096), torch.device("cuda:0"))
    with pytest.raises(ValueError):
        D.HandDetector(cam, (0, 4), torch.device("cuda:0"))
    with pytest.raises(RuntimeError):
        D.HandDetector(cam, (4, 4), torch.device("cpu"))
    with pytest.raises(ValueError):
        D.assign_host(*_slots([(1, 1)]), (4, 4), [0], np.zeros((1, 4)), [0], [0], 0)


def test_a_tracked_stream_refuses_a_detector_of_other_frames():
    """TrackedStream's check of detector=, on stand-ins that carry what it reads (the stream itself lives on a GPU: tests/test_detect_gpu.py builds one)"""
    import torch
    dev = torch.device("cuda:0")
    det = types.SimpleNamespace(F=2, H=480, W=640, device=dev)
    check_detector(det, 2, 480, 640, dev, 3)
    for kw in (dict(F=1), dict(H=481), dict(W=320), dict(device=torch.device("cuda:1")), dict(device=torch.device("cpu"))):
        with pytest.raises(ValueError):
            check_detector(types.SimpleNamespace(**dict(vars(det), **kw)), 2, 480, 640, dev, 3)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            check_detector(det, 2, 480, 640, dev, bad)


def test_the_interface_declares_exports_and_binds_the_entries():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    lib = L.load()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 36 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    for name in NEW:
        assert name in L.EXPORTS and re.search(r"\bint %s\(" % name, hdr) and getattr(lib, name)
    assert len(L._SIGS["kpf_detect_hands_u16"]) == 22 and len(L._SIGS["kpf_detect_assign_f64"]) == 15
    assert lib.kpf_detect_ws64_words(1, 480, 640, 4) == 4 * 480 * 640 + 1200 * 4 and lib.kpf_detect_ws64_words(1, 4097, 4096, 4) == -1


_GOOD = dict(depth=True, F=2, H=6, W=8, cam=True, near=171, far=1500, step_mm=20, reach_mm=150, min_pixels=64, min_area=2000.0, max_area=40000.0,
             expansion=1.25, K=4, ws32=True, ws64=True, boxes=True, valid=True, info=True, labels=True, stats=True)
_NAN, _INF = float("nan"), float("inf")
REFUSED = [dict(depth=False), dict(cam=False), dict(ws32=False), dict(ws64=False), dict(boxes=False), dict(valid=False), dict(info=False), dict(labels=False),
           dict(stats=False), dict(F=0), dict(F=33), dict(H=0), dict(W=-1), dict(H=4097, W=4096), dict(K=0), dict(K=9), dict(near=1501), dict(near=-1),
           dict(far=65536), dict(step_mm=-1), dict(reach_mm=65536), dict(min_pixels=0), dict(min_area=_NAN), dict(max_area=_INF), dict(min_area=5e4),
           dict(min_area=-1.0), dict(expansion=0.0), dict(expansion=_NAN), dict(camv=(1, 0, 0.0)), dict(camv=(0, 1, -3.0)), dict(camv=(1, 2, _NAN)),
           dict(camv=(0, 3, _INF)), dict(misaligned="depth"), dict(misaligned="boxes"), dict(misaligned="ws32")]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_a_refusal_comes_before_any_device_call_and_writes_nothing(bad):
    """the refusals need no GPU: the entry returns before its first launch, and host arrays filled with a sentinel stand in for the buffers"""
    kw = dict(_GOOD)
    kw.update({k: v for k, v in bad.items() if k in kw})
    F, H, W, K = 2, 6, 8, 4
    arrays = dict(depth=np.full((F, H, W), 0x5A5A, np.uint16), cam=np.array([[600, 600, 4, 3], [500, 510, 4, 3]], np.float32),
                  ws32=np.full(F * 8 * H * W + 1, 0x1234567, np.int32), ws64=np.full(F * (4 * H * W + K), -5, np.int64), boxes=np.full((F, K, 4) , -7.0),
                  valid=np.full((F, K), -9, np.int32), info=np.full((F, K, 8), -11.0), labels=np.full((F, H, W), -13, np.int32),
                  stats=np.full((F, 5), -77, np.int32))
    if "camv" in bad:
        arrays["cam"][bad["camv"][0], bad["camv"][1]] = bad["camv"][2]
    before = {k: a.copy() for k, a in arrays.items()}
    ptr = {k: (a.ctypes.data if kw[k] else None) for k, a in arrays.items()}
    if "misaligned" in bad:
        ptr[bad["misaligned"]] += 1
    lib = L.load()
    rc = lib.kpf_detect_hands_u16(ptr["depth"], kw["F"], kw["H"], kw["W"], ptr["cam"], kw["near"], kw["far"], kw["step_mm"], kw["reach_mm"], kw["min_pixels"],
                                  kw["min_area"], kw["max_area"], kw["expansion"], kw["K"], ptr["ws32"], ptr["ws64"], ptr["boxes"], ptr["valid"], ptr["info"],
                                  ptr["labels"], ptr["stats"], None)
    assert rc != 0 and b"kpf_detect_hands_u16" in lib.kpf_last_error(), (bad, lib.kpf_last_error())
    for k, a in arrays.items():
        assert np.array_equal(a.view(np.uint8), before[k].view(np.uint8)), k


@pytest.mark.parametrize("bad", [dict(boxes=False), dict(index=False), dict(reseeded=False), dict(F=0), dict(F=33), dict(K=9), dict(B=0), dict(W=0),
                                 dict(reseed_after=0)], ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_the_assignment_refuses_before_any_device_call(bad):
    kw = dict(dict(boxes=True, index=True, reseeded=True, F=1, K=4, B=2, W=640, H=480, reseed_after=3), **bad)
    boxes, valid, info = _slots([(5, 5)])
    index, bbox, lost, seeded, reseeded = np.zeros(2, np.int32), np.full((2, 4), -3.0), np.full(2, 5, np.int32), np.ones(2, np.int32), np.full(2, -1, np.int32)
    lib = L.load()
    rc = lib.kpf_detect_assign_f64(boxes.ctypes.data if kw["boxes"] else None, valid.ctypes.data, info.ctypes.data, kw["F"], kw["K"], kw["W"], kw["H"],
                                   index.ctypes.data if kw["index"] else None, kw["B"], kw["reseed_after"], bbox.ctypes.data, lost.ctypes.data,
                                   seeded.ctypes.data, reseeded.ctypes.data if kw["reseeded"] else None, None)
    assert rc != 0 and b"kpf_detect_assign_f64" in lib.kpf_last_error(), (bad, lib.kpf_last_error())
    assert (bbox == -3.0).all() and lost.tolist() == [5, 5] and reseeded.tolist() == [-1, -1]


def test_the_bench_tool_parses_and_names_its_record():
    """tools/detect_bench.py needs the GPU to run; here it must at least be valid Python that writes where DESIGN.md 4.21 says"""
    import ast
    src = open(os.path.join(ROOT, "tools", "detect_bench.py")).read()
    ast.parse(src)
    assert '"profiles", "detect_bench.json"' in src and "HandDetector" in src and "TrackedStream" in src


# ---- the kernels' own union-find on the host ----------------------------------------------------------------------------------------------------------------

def test_the_kernels_union_find_header_on_the_host_under_the_sanitizers(tmp_path):
    """csrc/kpf_detect_uf.h is __host__ __device__: tools/detect_uf_check.cpp, a stand-alone program built with the address and undefined-behaviour
    sanitizers, drives its find and union sequentially -- tiles, seams, flatten as the kernels do, and all unions at once -- in row-major, reversed and six
    shuffled orders over every scene, and compares the labels with the restatement's."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "detect_uf_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keypointfusion_amd", "csrc"),
            os.path.join(ROOT, "tools", "detect_uf_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked INTO the program (gcc's spelling, then clang's, then the compiler's default): it stands alone
    built = [subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], [])
             if not os.path.exists(exe)]
    assert os.path.exists(exe), b"\n".join(b.stdout for b in built).decode(errors="replace")[-3000:]
    files = []
    for name in DC.CASES:
        depth, _, params = DC.build(name)
        p = D.check_params(**params)
        for f in range(depth.shape[0]):
            lab = D.label_propagate_host(depth[f], p["near"], p["far"], p["step_mm"]).astype(np.int32)
            path = str(tmp_path / ("%s_%d.bin" % (name, f)))
            with open(path, "wb") as fh:
                fh.write(np.array([depth.shape[1], depth.shape[2], p["near"], p["far"], p["step_mm"]], np.int32).tobytes())
                fh.write(np.ascontiguousarray(depth[f]).tobytes())
                fh.write(np.ascontiguousarray(lab).tobytes())
            files.append(path)
    run = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert run.returncode == 0 and b"ok" in run.stdout, run.stdout.decode(errors="replace")[-2000:]
    wrong = str(tmp_path / "wrong.bin")  # the program does compare: one label off is reported
    raw = bytearray(open(files[list(DC.CASES).index("diagonal")], "rb").read())
    raw[20 + 2 * 50 * 70 + 4 * (22 * 70 + 23)] ^= 1
    open(wrong, "wb").write(bytes(raw))
    assert subprocess.run([exe, wrong], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60).returncode == 1
