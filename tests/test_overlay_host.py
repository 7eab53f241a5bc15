"""overlay.draw_host, the numpy-float32 statement of the overlay's drawing rule, against pixel sets worked out by hand, and the
interface's bookkeeping.  No GPU: test_overlay_gpu.py holds the kernels to draw_host's bits."""
import os
import re

import numpy as np
import pytest

import overlay_cases as C
from conftest import ROOT
from keypointfusion_amd import lib as L
from keypointfusion_amd import overlay as O

PARKED = (0.0, 0.0, -1000.0)  # z <= 0: not ok, so the vertex is in no drawn face
UNIT = np.asarray([[1.0, 1.0, 0.0, 0.0]], np.float32)  # with sample_offset 0 a vertex (4 c, 4 r, 4) lies exactly on pixel (c, r), 4 mm away


def _triangle():
    """one fronto-parallel triangle with its right angle at pixel (2, 2) and legs of 8 pixels: its area function is 64, every weight is an integer over
    64, so the weights sum to exactly 1 and the depth is exactly 4 everywhere"""
    v = np.tile(np.asarray(PARKED, np.float32), (1, 778, 1))
    v[0, 0], v[0, 1], v[0, 2] = (8.0, 8.0, 4.0), (40.0, 8.0, 4.0), (8.0, 40.0, 4.0)
    want = np.zeros((16, 16), bool)
    for r in range(16):
        for c in range(16):
            want[r, c] = c >= 2 and r >= 2 and (c - 2) + (r - 2) <= 8
    return v, np.asarray([[0, 1, 2]], np.int32), want


def _rgb(F=1, Hh=16, Ww=16, seed=3):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (F, Hh, Ww, 3), dtype=np.uint8)


def test_one_triangle_covers_the_hand_computed_pixels_at_constant_depth():
    v, f, want = _triangle()
    rgb = _rgb()
    out = O.draw_host(rgb, f, v, UNIT)
    assert want.sum() == 45 and np.array_equal(out["label"][0] == O.LABEL_MESH, want) and set(np.unique(out["label"])) == {0, 1}
    assert np.array_equal(out["depth"][0], np.where(want, np.float32(4), np.float32(0)))
    assert np.array_equal(out["owner"][0], np.where(want, 0, -1)) and np.array_equal(out["prim"][0], np.where(want, 0, -1))
    assert out["project"]["rect"].tolist() == [[2, 2, 10, 10]] and out["project"]["ok"].sum() == 3
    # the other winding covers the same pixels (two-sided)
    assert np.array_equal(O.draw_host(rgb, f[:, ::-1], v, UNIT)["label"], out["label"])


def test_alpha_zero_keeps_the_frame_and_alpha_one_paints_the_mesh_colour():
    v, f, want = _triangle()
    rgb = _rgb()
    assert np.array_equal(O.draw_host(rgb, f, v, UNIT, alpha=0.0)["image"], rgb)
    out = O.draw_host(rgb, f, v, UNIT, alpha=1.0, ambient=1.0, mesh_color=(12.0, 200.0, 255.0))
    assert np.array_equal(out["image"][0][want], np.tile(np.asarray([12, 200, 255], np.uint8), (45, 1)))
    assert np.array_equal(out["image"][0][~want], rgb[0][~want])
    # ambient = 1 is the same with normals: shade = 1 + 0 |n.z|
    n = np.zeros((1, 778, 3), np.float32)
    n[0, :3] = (0.6, 0.0, -0.8)
    assert np.array_equal(O.draw_host(rgb, f, v, UNIT, normals=n, alpha=1.0, ambient=1.0, mesh_color=(12.0, 200.0, 255.0))["image"], out["image"])
    # a headlight: ambient 0.25, |n.z| = 0.5 -> shade 0.625 exactly; 200 * 0.625 = 125
    n[0, :3] = (0.0, 0.0, -0.5)
    lit = O.draw_host(rgb, f, v, UNIT, normals=n, alpha=1.0, ambient=0.25, mesh_color=(200.0, 8.0, 0.0))
    assert np.array_equal(lit["image"][0][want], np.tile(np.asarray([125, 5, 0], np.uint8), (45, 1)))


def test_a_radius_two_joint_covers_the_thirteen_pixels_of_its_disc():
    rgb = _rgb()
    jp = np.asarray([[[7.0, 6.0, 500.0]]], np.float32)
    out = O.draw_host(rgb, joints_px=jp, bones=(), bone_color=(), joint_color=((9, 8, 7),), joint_radius=2.0)
    want = np.zeros((16, 16), bool)
    for r in range(16):
        for c in range(16):
            want[r, c] = (c - 7) ** 2 + (r - 6) ** 2 <= 4
    assert want.sum() == 13 and np.array_equal(out["label"][0] == O.LABEL_JOINT, want)
    assert np.array_equal(out["image"][0][want], np.tile(np.asarray([9, 8, 7], np.uint8), (13, 1))) and not out["depth"].any()
    assert np.array_equal(out["owner"][0], np.where(want, 0, -1)) and np.array_equal(out["prim"][0], np.where(want, 0, -1))


def test_a_horizontal_bone_covers_one_row_between_its_ends():
    rgb = _rgb()
    jp = np.asarray([[[3.0, 5.0, 500.0], [9.0, 5.0, 500.0]]], np.float32)
    kw = dict(bones=((0, 1),), bone_color=((1, 2, 3),), joint_color=((9, 8, 7), (6, 5, 4)), joint_radius=0.0, bone_half_width=0.75)
    out = O.draw_host(rgb, joints_px=jp, **kw)
    want = np.zeros((16, 16), bool)
    want[5, 3:10] = True
    assert np.array_equal(out["label"][0] == O.LABEL_BONE, want) and set(np.unique(out["label"])) == {0, 2}  # the bone lies over its joints' pixels
    assert np.array_equal(out["image"][0][want], np.tile(np.asarray([1, 2, 3], np.uint8), (7, 1)))
    # without the bone the radius-0 joints cover their own pixel; a NaN end drops the joint and the bone
    dots = O.draw_host(rgb, joints_px=jp, **dict(kw, bones=(), bone_color=()))
    assert np.argwhere(dots["label"][0] == O.LABEL_JOINT).tolist() == [[5, 3], [5, 9]] and dots["prim"][0][5, 9] == 1
    jp[0, 1, 0] = np.nan
    gone = O.draw_host(rgb, joints_px=jp, **kw)
    assert np.argwhere(gone["label"][0] != 0).tolist() == [[5, 3]]


def test_pixels_that_nothing_covers_are_the_frames():
    out, c = C.full_host(), C.full_case()
    none = out["label"] == O.LABEL_NONE
    assert none.any() and np.array_equal(out["image"][none], c["rgb"][none])
    assert bool((out["owner"][none] == -1).all()) and bool((out["prim"][none] == -1).all()) and not out["depth"][none].any()
    # the case is what the GPU tests need: every label but 4 is present, the mesh crosses both seams, hand 0 leaves the grid, both hands of frame 0 own pixels
    assert {int(x) for x in np.unique(out["label"])} == {0, 1, 2, 3}
    mesh = out["depth"] > 0
    assert mesh[0][:, 63].any() and mesh[0][:, 64].any() and mesh[0][63].any() and mesh[0][64].any() and mesh[0][C.H - 1].any()
    own = out["owner"][0][mesh[0]]
    assert (own == 0).sum() > 100 and (own == 1).sum() > 100 and not (out["owner"][1] == 0).any() and (out["owner"][1] == 2).sum() > 100


def test_the_scene_hides_what_lies_behind_it():
    v, f, want = _triangle()
    rgb = _rgb()
    seen = np.zeros((1, 16, 16), np.uint16)
    seen[0, 4:6, 3:8] = 2  # 2 mm in front of the triangle at 4 mm
    out = O.draw_host(rgb, f, v, UNIT, depth_frame=seen, occl_margin=1.0)
    hid = want & (seen[0] != 0)
    assert hid.sum() == 10 and np.array_equal(out["label"][0] == O.LABEL_HIDDEN, hid) and np.array_equal(out["image"][0][hid], rgb[0][hid])
    assert np.array_equal(out["depth"][0], np.where(want, np.float32(4), np.float32(0))) and np.array_equal(out["owner"][0], np.where(want, 0, -1))
    # not more than the margin in front: nothing is hidden
    assert not (O.draw_host(rgb, f, v, UNIT, depth_frame=seen, occl_margin=2.0)["label"] == O.LABEL_HIDDEN).any()


def test_the_skeleton_tables_follow_the_models_joint_order():
    assert len(O.MANO21_BONES) == 20 and len(O.MANO21_BONE_COLOR) == 20 and len(O.MANO21_JOINT_COLOR) == 21
    assert sorted(b for _, b in O.MANO21_BONES) == list(range(1, 21)) and [a for a, _ in O.MANO21_BONES].count(0) == 5  # a tree from the wrist
    assert O.MANO21_BONES[:4] == ((0, 13), (13, 14), (14, 15), (15, 20)) and O.MANO21_JOINT_COLOR[20] == O.FINGER_COLOR["thumb"]
    assert O.MANO21_JOINT_COLOR[0] == O.WRIST_COLOR and O.MANO21_JOINT_COLOR[18] == O.FINGER_COLOR["little"] == O.MANO21_BONE_COLOR[-1]


def test_the_interface_declares_exports_and_binds_the_overlay():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    lib = L.load()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 34 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    for name in ("kpf_overlay_project_f32", "kpf_overlay_draw_u8"):
        assert name in L.EXPORTS and re.search(r"\bint %s\(" % name, hdr) and getattr(lib, name), name
    fields = re.search(r"typedef struct \{([^}]*)\} kpf_overlay_draw_desc;", hdr).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [n for n, _ in L.OverlayDrawDesc._fields_]


@pytest.mark.parametrize("bad", [dict(ambient=1.5), dict(B=0), dict(B=1 << 20), dict(H=0), dict(sample_offset=float("nan")), dict(verts=None)])
def test_the_projection_refuses_before_any_device_call(bad):
    """the refusals need no GPU: the entry returns before its launch"""
    kw = dict(verts=1, ambient=0.3, B=1, H=8, sample_offset=0.0)
    kw.update(bad)
    rc = L.load().kpf_overlay_project_f32(kw["verts"], None, 1, None, kw["sample_offset"], kw["ambient"], kw["H"], 8, 1, 1, 1, 1, 1, 1, kw["B"], None)
    assert rc != 0 and b"kpf_overlay_project_f32" in L.load().kpf_last_error()


def test_the_bench_tool_parses_and_names_its_record():
    """tools/overlay_bench.py needs the GPU to run; here it must at least be valid Python that writes where DESIGN.md 4.19 says"""
    import ast
    src = open(os.path.join(ROOT, "tools", "overlay_bench.py")).read()
    ast.parse(src)
    assert '"profiles", "overlay_bench.json"' in src and "FrameOverlay" in src and "TrackedStream" in src
