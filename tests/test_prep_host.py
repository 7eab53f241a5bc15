"""CPU side of the device preprocessing path (keypointfusion_amd/preprocess_gpu.py, kpf_prep_* of include/kpf.h): the interface is declared, exported and
bound (since ABI 18), bad arguments are refused with a message instead of a launch, and the inputs of tests/test_preprocess_gpu.py are what that file's
assertions assume (the host path's results for them, and their distance from a rounding decision)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import prep_cases as PC
from conftest import ROOT
from keypointfusion_amd import lib as L

PREP = ("kpf_prep_crop_u16", "kpf_prep_pcl_sample", "kpf_prep_uncrop_f32")


def test_prep_entry_points_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in PREP:
        assert re.search(r"\bint %s\s*\(" % name, hdr), "%s is not declared in include/kpf.h" % name
        assert name in L.EXPORTS
        assert hasattr(raw, name), "libkpf_hip.so does not export %s" % name


def test_header_library_and_binding_agree_on_an_abi_with_the_prep_interface():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 18  # (the kpf_prep_* entry points came with ABI 18)
    assert L.ABI_VERSION == abi and L.load().kpf_abi_version() == abi


def test_bad_arguments_fail_with_a_message_not_a_launch():
    """Null pointers, a crop size beyond the LDS plan and more samples than pixels return KPF_EINVAL before anything reaches a device."""
    l = L.load()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused by its argument checks
    crop = lambda S, rgb=p: l.kpf_prep_crop_u16(rgb, p, p, p, p, 1, 480, 640, 0, 0, 480, 640, S, p, p, p, p, p, p, p, p, p, None)
    pcl = lambda S, n, seed=p: l.kpf_prep_pcl_sample(p, p, p, p, p, seed, 1, S, n, p, p, p, None, None)
    calls = ((lambda: crop(128, None), "null"), (lambda: crop(129), "S = 129"), (lambda: crop(0), "S = 0"), (lambda: pcl(128, 1024, None), "null"),
             (lambda: pcl(256, 1024), "S = 256"), (lambda: pcl(64, 64 * 64 + 1), "n = 4097"), (lambda: pcl(128, 8192), "LDS"),
             (lambda: l.kpf_prep_uncrop_f32(p, p, p, p, None, 1, 21, p, p, None), "null"),
             (lambda: l.kpf_prep_uncrop_f32(p, p, p, p, p, 0, 21, p, p, None), "bad shape"),
             (lambda: l.kpf_prep_crop_u16(p, p, p, p, p, 1, 460, 500, 1500, 300, 1080, 1920, 128, p, p, p, p, p, p, p, p, p, None), "leaves"))
    for call, word in calls:
        rc = call()
        assert rc == -1 and word in l.kpf_last_error().decode(), (rc, word, l.kpf_last_error())


def test_device_preprocessor_refuses_bad_inputs_without_a_device():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    pre = DevicePreprocessor()
    rgb, depth = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(2, 48, 64, dtype=torch.uint16)
    bbox, cam, seed = torch.zeros(2, 4, dtype=torch.float64), torch.ones(2, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="uint16"):
        pre.prepare(rgb, depth.float(), bbox, cam, seed)
    with pytest.raises(TypeError, match="uint16"):
        pre.prepare(rgb, depth.to(torch.int32), bbox, cam, seed)
    with pytest.raises(ValueError, match="does not match"):
        pre.prepare(rgb[:, :40], depth, bbox, cam, seed)
    with pytest.raises(ValueError, match="bbox has shape"):
        pre.prepare(rgb, depth, bbox[:1], cam, seed)
    with pytest.raises(TypeError, match="cam must be"):
        pre.prepare(rgb, depth, bbox, cam.float(), seed)
    with pytest.raises(ValueError, match="seed has shape"):
        pre.prepare(rgb, depth, bbox, cam, seed[:1])
    with pytest.raises(ValueError, match="leaves"):
        pre.prepare(rgb, depth, bbox, cam, seed, origin=(1900, 0), frame_size=(1080, 1920))
    with pytest.raises(ValueError, match="go together"):
        pre.prepare(rgb, depth, bbox, cam, seed, origin=(0, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pre.prepare(rgb, depth, bbox, cam, seed)  # well-formed, but host tensors: preprocess.prepare_rgbd is the host path
    with pytest.raises(ValueError, match="img_size"):
        DevicePreprocessor(img_size=256)
    with pytest.raises(ValueError, match="sample_num"):
        DevicePreprocessor(img_size=32, sample_num=2048)


def test_cases_reach_the_branches_they_are_named_for():
    """The host path on the synthetic frames: counts, bounds and crop sizes the GPU tests' case table relies on, and every com_to_bounds floor argument
    far enough from an integer that the device's summation order (a few 1e-13 relative on the centre of mass) cannot flip a bound."""
    rec = {}
    for name in PC.CASES:
        rgb, depth, bbox, cam = PC.synth_frame(name)
        rec[name] = h = PC.host_record(rgb, depth, bbox, cam)
        assert PC.floor_margin(h["com"], cam) >= 1e-6, name
    n = {k: len(v["candidates"]) for k, v in rec.items()}
    assert n["centre"] == 2969 and n["corner"] == 733 and n["far_small"] == 357 and n["background_wall"] == 0 and n["empty"] == 0
    assert 1024 // n["far_small"] == 2 and 1024 % n["far_small"] == 310
    assert n["full_wall"] > 8192  # more than half the pixels: the sort runs over all 16384 LDS elements
    assert tuple(rec["corner"]["bounds"]) == (-117, 181, -119, 178)
    b = rec["near_big"]["bounds"]
    assert b[0] < 0 and b[1] > 640 and b[2] < 0 and b[3] > 480
    assert list(rec["empty"]["com"]) == [250.0, 170.0, 300.0]
    b = rec["fx_ne_fy"]["bounds"]
    assert (b[1] - b[0], b[3] - b[2]) == (219, 207) and tuple(rec["fx_ne_fy"]["sz"]) == (128, 120)
    rw, dw, bbox, cam, org, fs = PC.demo_window()
    assert PC.floor_margin(PC.host_record(*PC.embed(rw, dw, org, fs), bbox, cam)["com"], cam) >= 1e-6
