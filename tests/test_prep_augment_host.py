"""CPU side of the training augmentation by the dataset protocol (keypointfusion_amd/preprocess.py::prepare_augmented and draw_augment, the yardsticks of
kpf_prep_augment_u16 and kpf_prep_aug_draw, ABI 25): bit-equal to the reference's TRAINING items — the committed fixture tests/golden/augment_item.npz
(gen_golden_augment.py) and, where the reference tree is present, the live DexYCBDataset / HO3D items on 200 random hands with random draws — the
properties of the draw, the rotation identities of the warp rule against itself, every refusal of the argument checks without a device, and the interface
declared, exported and bound.  The two warps are the project's own rule, restated from OpenCV's algorithm and UNPINNED against a real OpenCV: the fixture
pins the logic around them."""
import ctypes
import hashlib
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

NEW = ("kpf_prep_augment_u16", "kpf_prep_aug_draw")
GEOMETRY = ("joint", "joint_img", "center", "M", "cube", "cam_para", "com")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def fixture_items():
    """(tag -> (inputs, aug, prepare_augmented's result, index)) of every fixture item, computed once."""
    z = np.load(os.path.join(GOLDEN, "augment_item.npz"))
    assert tuple(z["in_cube"]) == AC.CUBE
    items = {}
    for i, (name, tag) in enumerate(zip(z["names"], z["tags"])):
        ins = AC.synth(str(name))
        aug = dict(mode=int(z["mode"][i]), off=z["off"][i], rot=float(z["rot"][i]), sc=float(z["sc"][i]), rot_cs=tuple(z["rot_cs"][i]),
                   color=z["color"][i] if z["has_color"][i] else None)
        rgb, depth, joints_mm, cam, mirror, center = ins
        got = P.prepare_augmented(rgb, depth, joints_mm, cam, aug, mirror, center, AC.CUBE, 128, 1024, np.random.RandomState(int(z["pcl_seed"][i])))
        items[(str(name), str(tag))] = (ins, aug, got, i)
    return z, items


def test_prepare_augmented_equals_the_reference_fixture_bit_for_bit(fixture_items):
    z, items = fixture_items
    frames = {n for n, _ in items}
    assert {"right", "left", "corner", "fx_ne_fy", "wall", "given", "empty"} <= frames
    assert all((n, m) in items for n in frames for m in P.AUG_MODES)
    assert {t for _, t in items} >= {"com_off0", "rot_0", "rot_360", "sc_1"}
    for (name, tag), (ins, aug, got, i) in items.items():
        for k in GEOMETRY:
            assert _bits(got[k], z["ref_" + k][i]), (name, tag, k)
        assert _sha(got["img"]) == str(z["sha_img"][i]), (name, tag, "img")
        assert _sha(got["img_rgb"]) == str(z["sha_img_rgb"][i]), (name, tag, "img_rgb")
        assert got["aug_status"] == int(z["status"][i])
        cand = P.depth_to_pcl(got["img"][0], got["center"], got["cube64"], got["M64"], tuple(float(c) for c in ins[3]))
        assert len(cand) == int(z["count"][i]), (name, tag)
        # without the pair the host computes it with NumPy: the same bits
        rgb, depth, joints_mm, cam, mirror, center = ins
        again = P.prepare_augmented(rgb, depth, joints_mm, cam, {k: v for k, v in aug.items() if k != "rot_cs"}, mirror, center, AC.CUBE)
        assert all(_bits(again[k], got[k]) for k in GEOMETRY + ("img", "img_rgb")), (name, tag)
    for tag in P.AUG_MODES:  # one case per mode in full
        got = items[("right", tag)][2]
        assert _bits(got["img"], z["full_img_" + tag]) and _bits(got["img_rgb"], z["full_img_rgb_" + tag].astype(np.float32) / np.float32(255)), tag


def test_mode_none_is_not_the_test_item(fixture_items):
    """Fact 1: the training branch divides the labels by a float64 scalar, so they stay float64 into joint_img: on `corner` it differs from the test
    item's, while joint has the test item's bits."""
    ins, _, got, _ = fixture_items[1][("corner", "none")]
    test_item = P.prepare_annotated(*ins, AC.CUBE)
    assert _bits(got["joint"], test_item["joint"]) and not _bits(got["joint_img"], test_item["joint_img"])
    assert all(_bits(got[k], test_item[k]) for k in ("img", "img_rgb", "center", "M", "cube", "com"))


def test_an_all_zero_depth_crop_warps_rgb_only(fixture_items):
    """Fact 2: np.max(img) == 0 leaves depth, labels, com, M and cube unaugmented; augmentCrop_RGB has no such test."""
    none = fixture_items[1][("empty", "none")][2]
    for tag in ("rot", "com", "sc"):
        got = fixture_items[1][("empty", tag)][2]
        assert all(_bits(got[k], none[k]) for k in GEOMETRY + ("img",)), tag
        assert not _bits(got["img_rgb"], none["img_rgb"]) and got["aug_status"] == 0, tag


def test_mode_sc_returns_the_scaled_cube_and_a_new_M(fixture_items):
    """Fact 3: cube is sc times the cube in all three components, M is new; with sc = 0.8377 the background of `right` is not exactly 1.0 after the
    normalisation, and getpcl's isclose still removes it: 4188 candidates."""
    z, items = fixture_items
    ins, aug, got, i = items[("right", "sc")]
    none = items[("right", "none")][2]
    assert aug["sc"] == 0.8377 and _bits(got["cube"], (np.asarray(AC.CUBE, np.float64) * 0.8377).astype(np.float32))
    assert not _bits(got["M"], none["M"]) and _bits(got["center"], none["center"])
    bg = got["img"].max()
    assert bg != 1.0 and abs(bg - 1.0) < 1e-6 and int(z["count"][i]) == 4188


def test_mode_rot_returns_the_old_M_and_rotates_the_labels_about_the_centre(fixture_items):
    """Fact 4: M unchanged; the labels rotate in the image plane around com[0:2], so every joint keeps its pixel distance from the centre and its depth."""
    _, items = fixture_items
    ins, aug, got, _ = items[("right", "rot")]
    none = items[("right", "none")][2]
    assert all(_bits(got[k], none[k]) for k in ("M", "center", "cube", "com")) and not _bits(got["joint"], none["joint"])
    r_rot, r_none = np.hypot(got["joint_img"][:, 0], got["joint_img"][:, 1]), np.hypot(none["joint_img"][:, 0], none["joint_img"][:, 1])
    # (the crop is centred on com: normalised crop coordinates are pixel offsets from it, up to the half-pixel of the integer bounds)
    assert np.abs(r_rot - r_none).max() < 2e-2 and np.abs(got["joint_img"][:, 2] - none["joint_img"][:, 2]).max() < 1e-6
    # and the depth after a com warp is no longer integer-valued: the near-plane clamp stores a float zstart
    com = items[("wall", "com")][2]
    d = com["img"][0].astype(np.float64) * 125.0 + float(com["center"][2])
    assert np.abs(d - np.rint(d)).max() > 1e-3


def test_prepare_augmented_equals_the_live_reference_on_random_hands():
    sys.path.insert(0, GOLDEN)
    import ref_import
    if not ref_import.reference_available():
        pytest.skip("reference tree not present")
    import gen_golden_augment as GA
    import gen_golden_dataset_item as G
    Lm = GA.load_loader_module()
    g = np.random.RandomState(12)
    kinds = {"left": 0, "given": 0, "empty": 0, "rot": 0, "com": 0, "sc": 0, "none": 0}
    for i in range(200):
        ins = AC.random_hand(g)
        rgb, depth, jm, cam, mirror, center = ins
        mode, off, rot, sc = int(g.randint(4)), g.uniform(-1, 1, 3) * 10.0, float(g.uniform(-180, 180)), float(abs(1.0 + g.uniform(-1, 1) * 0.2))
        ref, color = GA.reference_train_item(Lm, "random%d" % i, 7000 + i, mode, off, rot, sc, ins)
        G.FRAMES.clear()
        got = P.prepare_augmented(rgb, depth, jm * 1000, cam, dict(mode=mode, off=off, rot=rot, sc=sc, color=color), mirror, center, AC.CUBE, 128, 1024,
                                  np.random.RandomState(7000 + i))
        GA.assert_equal(ref, got, i)
        kinds["left"] += mirror
        kinds["given"] += center is not None
        kinds["empty"] += int(ref["count"]) == 0
        kinds[P.AUG_MODES[mode]] += 1
    print(kinds)
    assert min(kinds.values()) >= 10, kinds


def test_draw_augment_has_the_reference_ranges_and_is_a_function_of_the_seed():
    seeds = np.arange(4096, dtype=np.int64) + 123456789
    d = P.draw_augment(seeds, 10.0, 0.2, 180.0, 0.2)
    counts = np.bincount(d["mode"], minlength=4)
    print("modes", counts.tolist())
    assert len(counts) == 4 and (np.abs(counts - 1024) <= 139).all()  # 5 sigma of a binomial with n = 4096, p = 1/4
    assert (d["off"] >= -10.0).all() and (d["off"] < 10.0).all() and (d["rot"] >= -180.0).all() and (d["rot"] < 180.0).all() and (d["sc"] > 0).all()
    assert (np.abs(d["sc"] - 1.0) <= 0.2).all() and (d["color"] >= 0.8).all() and (d["color"] <= 1.2).all()
    assert abs(d["off"].mean()) < 0.5 and abs(d["rot"].mean()) < 10 and d["off"].std() > 5 and d["rot"].std() > 90  # spread over the range, not a constant
    for k in ("off", "rot", "sc", "color"):
        assert len(np.unique(d[k].reshape(4096, -1)[:, 0])) == 4096, k  # two different seeds differ
    again = P.draw_augment(seeds, 10.0, 0.2, 180.0, 0.2)
    assert all(_bits(d[k], again[k]) for k in d)  # the same seed repeats
    one = P.draw_augment(seeds[7:8], 10.0, 0.2, 180.0, 0.2)
    assert all(_bits(one[k][0], d[k][7]) for k in d)  # and does not depend on the batch
    assert _bits(d["rot_cs"], np.stack([np.cos(np.mod(d["rot"], 360) * np.pi / 180.0), np.sin(np.mod(d["rot"], 360) * np.pi / 180.0)], 1))
    assert (P.draw_augment(seeds, 10.0, 0.2, 180.0, 0.0)["color"] == 1.0).all()


def test_rotation_identities_of_the_warp_rule():
    S = 128
    g = np.random.RandomState(4)
    crop = g.randint(1, 60000, (S, S)).astype(np.float32)
    rot = lambda img, deg: P.warp_affine_nearest(img, P.rotation_matrix_2d(S // 2, S // 2, *P._rot_cs(deg)))
    assert _bits(rot(crop, 0.0), crop) and _bits(rot(crop, 360.0), crop)
    twice = rot(rot(crop, 180.0), 180.0)
    inside = np.zeros((S, S), bool)
    inside[1:, 1:] = True  # a half turn about (64, 64) maps index i to 128 - i: row and column 0 leave the crop
    assert _bits(twice[inside], crop[inside]) and not twice[~inside].any()
    quarter = rot(crop, 90.0)
    assert quarter[S // 2, S // 2] == crop[S // 2, S // 2] and not _bits(quarter, crop)
    # a quarter turn four times is the identity where nothing left the crop
    four = rot(rot(rot(quarter, 90.0), 90.0), 90.0)
    assert _bits(four[inside], crop[inside])
    # the perspective rule with the identity and with an integer shift
    assert _bits(P.warp_perspective_nearest(crop, np.eye(3)), crop)
    shift = np.array([[1.0, 0, 3], [0, 1.0, -2], [0, 0, 1]])
    moved = P.warp_perspective_nearest(crop, shift)
    assert _bits(moved[:-2, 3:], crop[2:, :-3]) and not moved[:, :3].any() and not moved[-2:].any()


def test_prepare_augmented_refuses_bad_arguments_and_bad_parameters():
    rgb, depth, joints_mm, cam, mirror, center = AC.synth("right")
    ok = dict(mode=3, off=np.zeros(3), rot=0.0, sc=1.0)
    for word, change in (("0..3", dict(mode=4)), ("0..3", dict(off=np.zeros(2))), ("three factors", dict(color=np.ones(2)))):
        with pytest.raises(ValueError, match=word):
            P.prepare_augmented(rgb, depth, joints_mm, cam, {**ok, **change})
    with pytest.raises(ValueError, match="required"):
        P.prepare_augmented(rgb, depth, None, cam, ok, center_xyz=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match=r"\[J\]\[3\]"):
        P.prepare_augmented(rgb, depth, joints_mm[:, :2], cam, ok)
    none = P.prepare_augmented(rgb, depth, joints_mm, cam, ok)
    nan = float("nan")
    for change in (dict(mode=0, rot=nan), dict(mode=2, sc=0.0), dict(mode=1, off=np.array([nan, 0.0, 0.0])), dict(mode=0, rot=30.0, rot_cs=(nan, 0.5)),
                   dict(mode=3, color=np.array([1.0, nan, 1.0])), dict(mode=2, sc=float("inf"))):
        got = P.prepare_augmented(rgb, depth, joints_mm, cam, {**ok, **change})
        assert got["aug_status"] == 2 and all(_bits(got[k], none[k]) for k in GEOMETRY + ("img", "img_rgb")), change


def test_header_library_and_binding_agree_on_abi_25_with_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), "%s is not declared in include/kpf.h" % name
        assert name in L.EXPORTS
        assert hasattr(raw, name), "libkpf_hip.so does not export %s" % name
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 25 and L.ABI_VERSION == abi and L.load().kpf_abi_version() == abi


def test_bad_arguments_fail_with_a_message_not_a_launch():
    l = L.load()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused by its argument checks

    def augment(rgb=p, joints=p, mode=p, rot_cs=p, status=p, J=21, S=128, F=1, win=(480, 640, 0, 0, 480, 640)):
        return l.kpf_prep_augment_u16(rgb, p, None, F, joints, p, None, p, p, mode, p, p, p, rot_cs, None, 1, J, *win, S, p, p, p, p, p, p, p, p, p, p, p, p, p,
                                      status, None)

    draw = lambda seed=p, B=1, sigma=10.0, cf=0.0: l.kpf_prep_aug_draw(seed, B, sigma, 0.2, 180.0, cf, 1, p, p, p, p, p, p, None)
    calls = ((lambda: augment(rgb=None), "null"), (lambda: augment(status=None), "null"), (lambda: augment(joints=None), "null joints"),
             (lambda: augment(mode=None), "augmentation parameter"), (lambda: augment(rot_cs=None), "augmentation parameter"), (lambda: augment(J=65), "J = 65"),
             (lambda: augment(S=129), "S = 129"), (lambda: augment(F=0), "stored frames"), (lambda: augment(win=(460, 500, 1500, 300, 1080, 1920)), "leaves"),
             (lambda: draw(seed=None), "null"), (lambda: draw(B=0), "B = 0"), (lambda: draw(sigma=-1.0), "finite and not negative"),
             (lambda: draw(cf=float("nan")), "finite and not negative"))
    for call, word in calls:
        rc = call()
        assert rc == -1 and word in l.kpf_last_error().decode(), (rc, word, l.kpf_last_error())


def test_device_preprocessor_refuses_bad_augmented_inputs_without_a_device():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor, train_batch
    pre = DevicePreprocessor()
    rgb, depth = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(2, 48, 64, dtype=torch.uint16)
    joints, cam, seed = torch.ones(2, 21, 3), torch.ones(2, 4), torch.zeros(2, dtype=torch.int64)
    f64 = torch.float64
    aug = dict(mode=torch.zeros(2, dtype=torch.int32), off=torch.zeros(2, 3, dtype=f64), sc=torch.ones(2, dtype=f64), rot=torch.zeros(2, dtype=f64),
               rot_cs=torch.zeros(2, 2, dtype=f64))
    ok = dict(rgb=rgb, depth=depth, joints_mm=joints, cam=cam, seed=seed, aug=aug)
    bad = (("required", ValueError, dict(joints_mm=None, center_xyz=torch.ones(2, 3))), ("uint16", TypeError, dict(depth=depth.float())),
           ("joints_mm has shape", ValueError, dict(joints_mm=joints[:1])), ("seed must be", TypeError, dict(seed=seed.int())),
           ("aug must be a dict", TypeError, dict(aug=[1])), (r"aug\['mode'\] must be torch.int32", TypeError, dict(aug=dict(aug, mode=aug["mode"].long()))),
           (r"aug\['off'\] has shape", ValueError, dict(aug=dict(aug, off=aug["off"][:, :2]))), (r"aug\['sc'\] must be", TypeError, dict(aug=dict(aug, sc=aug["sc"].float()))),
           (r"aug\['rot'\] has shape", ValueError, dict(aug=dict(aug, rot=aug["rot"][:1]))), (r"aug\['rot_cs'\] must be a torch tensor", TypeError, dict(aug={k: v for k, v in aug.items() if k != "rot_cs"})),
           (r"aug\['color'\] has shape", ValueError, dict(aug=dict(aug, color=torch.ones(2, 2, dtype=f64)))), ("sigma_com", ValueError, dict(sigma_com=-1)),
           ("rot_range", ValueError, dict(rot_range=float("nan"))), ("color_factor", ValueError, dict(color_factor="x")),
           ("no CPU fallback", RuntimeError, dict()))  # well-formed, but host tensors: preprocess.prepare_augmented is the host path
    for word, exc, change in bad:
        with pytest.raises(exc, match=word):
            pre.prepare_augmented(**{**ok, **change})
    assert DevicePreprocessor.check_augmented(rgb, depth, joints, cam, seed, aug) == (2, 21, 48, 64, 0, 0, 48, 64)
    assert DevicePreprocessor.check_augmented(rgb, depth, joints, cam, seed) == (2, 21, 48, 64, 0, 0, 48, 64)
    # uncrop on an augmented result is refused before anything else is looked at; train_batch wants the labels
    with pytest.raises(ValueError, match="augmented crop is refused"):
        pre.uncrop(torch.zeros(2, 21, 3), dict(augmented=True))
    with pytest.raises(ValueError, match="joint_img"):
        train_batch({k: torch.zeros(1) for k in ("img_rgb", "img", "pcl", "center", "M", "cube", "cam_para")})
    prep = {k: torch.zeros(1) for k in ("img_rgb", "img", "pcl", "center", "M", "cube", "cam_para", "joint", "joint_img")}
    b = train_batch(prep, epoch=torch.tensor(3))
    assert b["uvd_gt"] is prep["joint_img"] and b["xyz_gt"] is prep["joint"] and int(b["epoch"]) == 3 and len(b) == 10
