"""CPU side of preprocessing by the dataset protocol (keypointfusion_amd/preprocess.py::prepare_annotated, the yardstick of kpf_prep_annot_u16, ABI 23):
bit-equal to the reference's dataset items — the committed fixture tests/golden/dataset_item.npz (gen_golden_dataset_item.py) and, where the reference tree
is present, the live DexYCBDataset / HO3D items on 200 random hands — the mirror identity, every refusal of the argument checks without a device, and the
interface declared, exported and bound."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import annot_cases as AC
from conftest import GOLDEN, ROOT
from keypointfusion_amd import lib as L
from keypointfusion_amd import preprocess as P

NEW = ("kpf_prep_annot_u16", "kpf_prep_uncrop_mirror_f32")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_prepare_annotated_equals_the_reference_fixture_bit_for_bit():
    z = np.load(os.path.join(GOLDEN, "dataset_item.npz"))
    names = [str(n) for n in z["names"]]
    assert names == list(AC.CASES) and tuple(z["in_cube"]) == AC.CUBE
    counts, sz = {}, {}
    for i, name in enumerate(names):
        rgb, depth, joints_mm, cam, mirror, center = AC.synth(name, int(z["in_frame_seed"][i]))
        # the annotations of the fixture are the ones the frames are regenerated with
        assert _bits(joints_mm, z["in_joints_mm"][i]) and _bits(cam, z["in_cam"][i]) and mirror == bool(z["in_mirror"][i]), name
        assert (center is not None) == bool(z["in_has_center"][i]) and (center is None or _bits(center, z["in_center_xyz"][i])), name
        h = AC.host_record(rgb, depth, z["in_joints_mm"][i], z["in_cam"][i], mirror, z["in_center_xyz"][i] if center is not None else None)
        for k in ("img", "joint", "joint_img", "center", "M", "cube", "cam_para"):
            assert _bits(h[k], z["ref_" + k][i]), (name, k)
        assert _bits(h["img_rgb"], z["ref_img_rgb"][i].astype(np.float32) / np.float32(255)), name
        assert np.array_equal(h["bounds"], z["ref_bounds"][i]) and len(h["candidates"]) == int(z["ref_count"][i]), name
        assert h["mirror"] == mirror and h["frame_w"] == rgb.shape[1]
        N = counts[name] = len(h["candidates"])
        sz[name] = tuple(int(v) for v in h["sz"])
        if N == 0:
            assert not h["pcl"].any()
        else:  # every sampled row is a candidate's row
            rows = {r.tobytes() for r in h["candidates"]}
            assert h["pcl"].shape == (1024, 3) and all(r.tobytes() in rows for r in h["pcl"]), name
    # the cases reach the branches they are named for
    b = dict(zip(names, z["ref_bounds"]))
    assert counts["wall"] == 0 and counts["empty"] == 0 and 0 < counts["far"] < 1024 and 0 < counts["corner"] < 1024 and counts["right"] > 1024
    assert b["right"][0] > 0 and b["right"][1] < 640 and b["corner"][0] < 0 and b["corner"][2] < 0 and b["left_edge"][0] < 0
    assert b["near"][0] < 0 and b["near"][1] > 640 and b["near"][2] < 0 and b["near"][3] > 480
    assert b["far"][1] - b["far"][0] < 128 and sz["fx_ne_fy"] == (128, 120)  # scaled up; letterboxed
    assert not _bits(z["ref_bounds"][names.index("given")], z["ref_bounds"][names.index("right")])


def test_prepare_annotated_equals_the_live_reference_on_random_hands():
    sys.path.insert(0, GOLDEN)
    import ref_import
    if not ref_import.reference_available():
        pytest.skip("reference tree not present")
    import gen_golden_dataset_item as G
    Lm = G.load_loader_module()
    g = np.random.RandomState(11)
    kinds = {"left": 0, "given": 0, "empty": 0, "tiled": 0}
    for i in range(200):
        ins = AC.random_hand(g)
        rgb, depth, jm, cam, mirror, center = ins
        ref = G.reference_item(Lm, "random%d" % i, 5000 + i, ins)
        G.FRAMES.clear()
        got = P.prepare_annotated(rgb, depth, jm * 1000, cam, mirror, center, AC.CUBE, 128, 1024, np.random.RandomState(5000 + i))
        G.assert_equal(ref, got, i)
        kinds["left"] += mirror
        kinds["given"] += center is not None
        kinds["empty"] += int(ref["count"]) == 0
        kinds["tiled"] += 0 < int(ref["count"]) < 1024
    print(kinds)
    assert min(kinds.values()) >= 10, kinds


@pytest.mark.parametrize("name", ["left", "left_edge", "hd_left"])
def test_mirror_equals_the_flipped_frame_with_flipped_annotations(name):
    """mirror=True on frame X against mirror=False on X[:, ::-1] with the annotations moved by u -> W - 1 - u: every array bit for bit."""
    rgb, depth, joints_mm, cam, mirror, _ = AC.synth(name)
    assert mirror
    a = AC.host_record(rgb, depth, joints_mm, cam, True, None)
    frgb, fdepth, fj, fc = AC.flipped(rgb, depth, joints_mm, cam)
    b = AC.host_record(frgb, fdepth, fj, cam, False, fc)
    for k in ("img", "img_rgb", "pcl", "center", "M", "cube", "cam_para", "com", "joint", "joint_img", "bounds", "sz", "M64", "candidates"):
        assert _bits(a[k], b[k]), (name, k)
    # and the un-crop takes the mirrored sample's pixels back to X's own columns
    px = P.project_to_crop(a["joint"], a["center"], a["M"], a["cube"], a["cam_para"])
    back, flipped = P.uncrop_points_mirrored(px, a["M"], True, a["frame_w"]), P.uncrop_points(px, a["M"])
    assert np.array_equal(back[:, 0], (a["frame_w"] - 1) - flipped[:, 0]) and np.array_equal(back[:, 1:], flipped[:, 1:])
    want = P._project_f32(joints_mm, cam)  # the annotation in X's own frame
    assert np.abs(back[:, :2] - want[:, :2]).max() < 1e-2
    assert np.array_equal(P.uncrop_points_mirrored(px, a["M"], False, a["frame_w"]), flipped)


def test_labels_without_joints_are_zeros_and_the_crop_is_the_same():
    rgb, depth, joints_mm, cam, mirror, center = AC.synth("given")
    a, b = P.prepare_annotated(rgb, depth, joints_mm, cam, mirror, center), P.prepare_annotated(rgb, depth, None, cam, mirror, center)
    for k in ("img", "img_rgb", "pcl", "center", "M", "com"):
        assert _bits(a[k], b[k]), k
    assert b["joint"].shape == (21, 3) and not b["joint"].any() and not b["joint_img"].any() and a["joint"].any()
    with pytest.raises(ValueError, match="neither"):
        P.prepare_annotated(rgb, depth, None, cam)
    with pytest.raises(ValueError, match=r"\[J\]\[3\]"):
        P.prepare_annotated(rgb, depth, joints_mm[:, :2], cam)
    with pytest.raises(ValueError, match=r"center_xyz"):
        P.prepare_annotated(rgb, depth, joints_mm, cam, center_xyz=np.zeros(2, np.float32))


def test_header_library_and_binding_agree_on_abi_23_with_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), "%s is not declared in include/kpf.h" % name
        assert name in L.EXPORTS
        assert hasattr(raw, name), "libkpf_hip.so does not export %s" % name
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 23 and L.ABI_VERSION == abi and L.load().kpf_abi_version() == abi


def test_bad_arguments_fail_with_a_message_not_a_launch():
    l = L.load()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused by its argument checks

    def annot(rgb=p, joints=p, centre=p, J=21, S=128, F=1, idx=None, win=(480, 640, 0, 0, 480, 640)):
        return l.kpf_prep_annot_u16(rgb, p, idx, F, joints, p, centre, p, p, 1, J, *win, S, p, p, p, p, p, p, p, p, p, p, p, p, None)

    unc = lambda mirror=p, w=640, B=1: l.kpf_prep_uncrop_mirror_f32(p, p, p, p, p, mirror, w, B, 21, p, p, None)
    calls = ((lambda: annot(rgb=None), "null"), (lambda: annot(joints=None, centre=None), "neither"), (lambda: annot(J=65), "J = 65"),
             (lambda: annot(J=0), "J = 0"), (lambda: annot(S=129), "S = 129"), (lambda: annot(F=0), "stored frames"),
             (lambda: annot(win=(460, 500, 1500, 300, 1080, 1920)), "leaves"), (lambda: unc(mirror=None), "null"), (lambda: unc(w=0), "frame width"),
             (lambda: unc(B=0), "bad shape"))
    for call, word in calls:
        rc = call()
        assert rc == -1 and word in l.kpf_last_error().decode(), (rc, word, l.kpf_last_error())


def test_device_preprocessor_refuses_bad_annotated_inputs_without_a_device():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    from keypointfusion_amd.serving import PipelinedEval
    pre = DevicePreprocessor()
    rgb, depth = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(2, 48, 64, dtype=torch.uint16)
    joints, cam, seed = torch.ones(2, 21, 3), torch.ones(2, 4), torch.zeros(2, dtype=torch.int64)
    mirror, centre = torch.zeros(2, dtype=torch.uint8), torch.ones(2, 3)
    ok = dict(rgb=rgb, depth=depth, joints_mm=joints, cam=cam, seed=seed, mirror=mirror, center_xyz=centre)
    bad = (("neither", ValueError, dict(joints_mm=None, center_xyz=None)), ("at most 64", ValueError, dict(joints_mm=torch.ones(2, 65, 3))),
           ("uint16", TypeError, dict(depth=depth.float())), ("rgb must be", TypeError, dict(rgb=rgb.float())),
           ("does not match", ValueError, dict(rgb=rgb[:, :40])), ("joints_mm has shape", ValueError, dict(joints_mm=joints[:1])),
           ("joints_mm has shape", ValueError, dict(joints_mm=torch.ones(2, 21, 2))), ("joints_mm must be", TypeError, dict(joints_mm=joints.double())),
           ("cam must be", TypeError, dict(cam=cam.double())), ("cam has shape", ValueError, dict(cam=cam[:, :3])),
           ("seed has shape", ValueError, dict(seed=seed[:1])), ("seed must be", TypeError, dict(seed=seed.int())),
           ("mirror must be", TypeError, dict(mirror=mirror.bool())), ("mirror has shape", ValueError, dict(mirror=mirror[:1])),
           ("center_xyz has shape", ValueError, dict(center_xyz=centre[:, :2])), ("center_xyz must be", TypeError, dict(center_xyz=centre.double())),
           ("torch tensor", TypeError, dict(joints_mm=joints.numpy())), ("torch tensor", TypeError, dict(mirror=[0, 1])),
           ("leaves", ValueError, dict(origin=(1900, 0), frame_size=(1080, 1920))), ("go together", ValueError, dict(origin=(0, 0))),
           ("frame_index must be", TypeError, dict(frame_index=torch.zeros(2, dtype=torch.int64))),
           ("no CPU fallback", RuntimeError, dict()))  # well-formed, but host tensors: preprocess.prepare_annotated is the host path
    for word, exc, change in bad:
        with pytest.raises(exc, match=word):
            pre.prepare_annotated(**{**ok, **change})
    assert DevicePreprocessor.check_annotated(rgb, depth, None, cam, seed, None, centre) == (2, 21, 48, 64, 0, 0, 48, 64)
    assert DevicePreprocessor.check_annotated(rgb, depth, joints[:, :5].contiguous(), cam, seed) == (2, 5, 48, 64, 0, 0, 48, 64)
    with pytest.raises(ValueError, match="neither"):  # refused before the model or a device is looked at
        PipelinedEval(None).submit_annotated(pre, rgb, depth, None, cam, seed)
