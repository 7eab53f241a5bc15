"""sensor.align_depth_host, the numpy statement of the depth-to-colour registration rule, against results worked out by hand, its float32
form against its float64 form, and the interface's bookkeeping and refusals.  No GPU: test_align_gpu.py holds the kernels to align_depth_host's bits."""
import ctypes
import os
import re

import numpy as np
import pytest

import align_cases as AC
import prep_cases as PC
from conftest import ROOT
from keypointfusion_amd import lib as L
from keypointfusion_amd import sensor as S

K = (600.0, 600.0, 320.0, 240.0)


def _one(raw, cal, out_size=None, **kw):
    out = S.align_depth_host(raw, cal[None] if cal.ndim == 1 else cal, out_size or raw.shape[-2:], **kw)
    return out["depth"][0], out["stats"][0]


def test_an_identity_calibration_returns_the_frame():
    dw = PC.demo_window()[1]
    cam = PC.demo_window()[3]
    assert dw.dtype == np.uint16 and (dw > 0).sum() > 1000
    d, st = _one(dw, S.make_calib(cam, cam), fill=0)
    assert np.array_equal(d, dw)
    assert st.tolist() == [(dw > 0).sum(), 0, 0, (dw > 0).sum(), 0]
    f, stf = _one(dw, S.make_calib(cam, cam), fill=1)  # the fill touches only what was not measured
    assert np.array_equal(f[dw > 0], dw[dw > 0]) and stf[:4].tolist() == st[:4].tolist() and stf[4] == ((f > 0) & (dw == 0)).sum()
    # a unit of 0.25 mm: d = rint(q / 4), half to even
    raw = np.arange(1, 401, dtype=np.uint16).reshape(20, 20)
    d, _ = _one(raw, S.make_calib(K, K, unit_mm=0.25), fill=0)
    assert np.array_equal(d, np.rint(raw * 0.25).astype(np.uint16)) and d[0, 1] == 0 and d[0, 5] == 2 and d[0, 9] == 2  # 0.5 -> 0 (skipped), 1.5 -> 2, 2.5 -> 2


def test_twice_the_resolution_repeats_every_pixel():
    raw = AC.scene("block", (30, 40))
    Kd = (55.0, 57.0, 19.3, 14.6)
    d, st = _one(raw, S.make_calib(Kd, (110.0, 114.0, 2 * 19.3 + 0.5, 2 * 14.6 + 0.5)), (60, 80), fill=0)
    assert np.array_equal(d, np.repeat(np.repeat(raw, 2, 0), 2, 1))
    assert st.tolist() == [(raw > 0).sum(), 0, 0, 4 * (raw > 0).sum(), 0]
    assert np.array_equal(S.make_calib(Kd, AC.scaled(Kd, 2))[4:8], np.asarray([110.0, 114.0, 39.1, 29.7], np.float32))


def test_a_frontal_plane_and_a_baseline_along_x_shift_the_columns():
    raw = np.full((24, 32), 600, np.uint16)
    raw[5:9, 3:30] = 0
    # tx fx / z = 5.25: the footprint [c + 4.75, c + 5.75) holds the one centre c + 5
    d, st = _one(raw, S.make_calib(K, K, t=(5.25, 0.0, 0.0)), fill=0)
    assert np.array_equal(d[:, 5:], raw[:, :-5]) and not d[:, :5].any()
    assert st.tolist() == [(raw > 0).sum(), 0, 0, (raw[:, :-5] > 0).sum(), 0]
    d, _ = _one(raw, S.make_calib(K, K, t=(-3.75, 0.0, 0.0)), fill=0)  # -3.75: [c - 4.25, c - 3.25) holds c - 4
    assert np.array_equal(d[:, :-4], raw[:, 4:]) and not d[:, -4:].any()


def _occlusion():
    """a far plane at 1200 with a near block at 400 in front; fx = 600 and tx = 20.5: the plane moves 10.25 -> 10 columns, the block 30.75 -> 31"""
    raw = np.full((40, 96), 1200, np.uint16)
    raw[10:30, 20:44] = 400
    want = np.zeros_like(raw)
    want[:, 10:] = np.where(raw[:, :-10] == 1200, 1200, 0)
    contested = np.zeros(raw.shape, bool)
    contested[10:30, 51:75] = want[10:30, 51:75] == 1200
    want[10:30, 51:75] = 400
    return raw, S.make_calib(K, K, t=(20.5, 0.0, 0.0)), want, contested


def test_the_near_surface_keeps_a_contested_pixel_whatever_the_order():
    raw, cal, want, contested = _occlusion()
    assert contested.sum() == 20 * 21  # the moved block's columns 54..74 lie over plane pixels, its first three over the plane's own shadow
    d, st = _one(raw, cal, fill=0)
    assert np.array_equal(d, want) and (d[contested] == 400).all()
    assert not d[10:30, 30:51].any()  # the occlusion shadow: the plane behind the block was never measured
    for order in ("reversed", 1, 2):
        d2, st2 = _one(raw, cal, fill=0, _order=order)
        assert np.array_equal(d2, d) and np.array_equal(st2, st)
    # the fill closes no shadow: it is 21 columns wide, and only its rim has two measured neighbours
    f, stf = _one(raw, cal, fill=1)
    assert np.array_equal(f[11:29, 31:50], np.zeros((18, 19), np.uint16)) and np.array_equal(f[d > 0], d[d > 0])


FP_SCENE = {}


def _fp_scene():
    if not FP_SCENE:
        raw_size = (120, 160)
        FP_SCENE["raw"] = AC.scene("block", raw_size, seed=5)
        FP_SCENE["Kd"] = AC.intrinsics(raw_size)
    return FP_SCENE["raw"], FP_SCENE["Kd"]


GRIDS = [(3.0, (360, 480)), (0.5, (60, 80)), (1.25, (150, 200))]


def test_float32_parts_from_float64_only_on_a_decision_boundary():
    """The float32 rule against the same rule in float64 on a 120 x 160 tilted plane with a near block and holes, rotated by 0.01 rad about y and 0.005
    about x and moved by (15, -0.3, 1.2) mm, registered to a 3 x, a 0.5 x and a 1.25 x colour grid, without and with the fill.

    On every grid the outputs may differ only at pixels that a raw pixel reaches through a float64 decision within 1e-4 of its boundary (a rectangle edge
    within 1e-4 of an integer, the centre's Zc within 1e-4 of a rounding boundary of d; with the fill also the empty pixels beside such a pixel), and the
    pixels that need this excuse are at most 0.1 % of the grid.  The excusable set itself is held to 0.1 % of the pixels compared, over the three grids
    together: on the 0.5 x grid alone its expected size IS the cap -- each of its 4800 pixels is written by the one raw pixel whose half-pixel footprint
    holds its centre, so an edge lies within 1e-4 of the centre with probability 2 * 2e-4 / 0.5 and Zc within 1e-4 of a half-integer with 2e-4, 1e-3 in
    all, 4.8 pixels -- so there its size says nothing about the rule.  Measured here: 81 / 5 / 22 excusable pixels without the fill (88 / 8 / 29 with it)
    of 172800 / 4800 / 30000, of which 18 / 0 / 2 differ."""
    raw, Kd = _fp_scene()
    for fill in (0, 1):
        excusable = compared = 0
        for k, out_size in GRIDS:
            cal = S.make_calib(Kd, AC.scaled(Kd, k), AC.rot(0.01, 0.005), AC.T_MM)
            a, sa = _one(raw, cal, out_size, fill=fill, dtype=np.float32)
            b, sb = _one(raw, cal, out_size, fill=fill, dtype=np.float64)
            out = AC.may_differ(raw, cal, out_size, 8, fill)
            differ = a != b
            print("x%g fill %d: %d of %d pixels differ, %d excusable; stats %s / %s" % (k, fill, differ.sum(), differ.size, out.sum(), sa.tolist(), sb.tolist()))
            assert not (differ & ~out).any(), (k, fill, np.argwhere(differ & ~out)[:8])
            assert differ.mean() <= 1e-3, (k, fill, differ.sum(), differ.size)
            assert (a > 0).mean() > 0.8 and sa[0] == sb[0] == (raw > 0).sum() and sa[1] == sa[2] == 0
            excusable, compared = excusable + int(out.sum()), compared + out.size
            if fill:  # many raw pixels contest one output pixel at the block's edge and on the coarse grid: the order is immaterial there too
                for order in ("reversed", 7):
                    c, sc = _one(raw, cal, out_size, fill=1, _order=order)
                    assert np.array_equal(c, a) and np.array_equal(sc, sa)
        assert excusable <= 1e-3 * compared, (fill, excusable, compared)


def test_the_fill_takes_the_least_of_two_measured_neighbours_of_the_unfilled_map():
    u = np.asarray([[0, 7, 0, 0, 0],
                    [5, 0, 9, 0, 0],
                    [0, 0, 0, 0, 3],
                    [0, 0, 4, 0, 0],
                    [6, 0, 0, 2, 0]], np.uint16)
    got, n = S.fill_host(u)
    # worked by hand, pixel by pixel: (row, col) -> non-zero 4-neighbours in the UNFILLED map
    hand = {(0, 0): (7, 5), (0, 2): (7, 9), (1, 1): (7, 5, 9), (2, 2): (9, 4), (3, 3): (4, 2), (4, 2): (4, 2), (4, 4): (2,), (1, 3): (9,), (2, 3): (3,),
            (3, 1): (4,), (2, 0): (5,), (3, 4): (3,), (4, 1): (6,), (0, 3): (), (0, 4): (), (1, 4): (3,), (2, 1): (), (3, 0): (6,)}
    exp = u.copy()
    for (r, c), nb in hand.items():
        assert u[r, c] == 0
        if len(nb) >= 2:
            exp[r, c] = min(nb)
    assert len(hand) == (u == 0).sum() and np.array_equal(got, exp) and n == 6
    assert got[0, 3] == 0 and got[2, 1] == 0  # not from FILLED values: (0,3) lies beside the filled (0,2), (2,1) between the filled (1,1) and (2,2)
    assert got[0, 0] == 5 and got[4, 2] == 2 and got[4, 4] == 0  # a corner and an edge pixel: outside the grid counts as not measured
    # the same through the whole rule, an identity calibration
    d, st = _one(u, S.make_calib(K, K), fill=1)
    assert np.array_equal(d, exp) and st.tolist() == [7, 0, 0, 7, 6]


def test_a_pixel_close_to_the_colour_cameras_plane_is_too_large_and_writes_nothing():
    raw = np.zeros((16, 16), np.uint16)
    raw[8, 8] = 500
    d, st = _one(raw, S.make_calib(K, K, t=(0.0, 0.0, -499.0)), fill=1)  # Zc = 1 mm: the footprint is 500 pixels wide
    assert not d.any() and st.tolist() == [1, 0, 1, 0, 0]
    # the span that decides: twice the resolution covers 2 x 2, which max_span = 1 refuses and 2 takes
    cal = S.make_calib(K, AC.scaled(K, 2))
    d, st = _one(raw, cal, (32, 32), max_span=1, fill=0)
    assert not d.any() and st.tolist() == [1, 0, 1, 0, 0]
    d, st = _one(raw, cal, (32, 32), max_span=2, fill=0)
    assert st.tolist() == [1, 0, 0, 4, 0] and (d[16:18, 16:18] == 500).all()


def test_points_behind_the_colour_camera_and_depths_beyond_16_bits_are_skipped():
    raw = np.zeros((16, 16), np.uint16)
    raw[8, 8], raw[3, 4] = 500, 700
    d, st = _one(raw, S.make_calib(K, K, t=(0.0, 0.0, -600.0)), fill=0)  # Zc = -100 and 100
    assert st.tolist() == [2, 1, 0, 0, 0] and not d.any()  # (the other point, 7 times nearer, lands off the grid)
    d, st = _one(raw, S.make_calib(K, K, t=(0.0, 0.0, -500.0)), fill=0)  # Zc = 0: u is not finite
    assert st[1] == 1 and d[8, 8] == 0
    raw[8, 8] = 40000
    d, st = _one(raw, S.make_calib(K, K, unit_mm=2.0), fill=0)  # 80000 mm and 1400 mm
    assert st.tolist() == [2, 1, 0, 1, 0] and d[8, 8] == 0 and d[3, 4] == 1400
    d, st = _one(raw, S.make_calib(K, K, unit_mm=0.00001), fill=0)  # d = rint(0.4) = 0 and rint(0.007) = 0
    assert st.tolist() == [2, 2, 0, 0, 0] and not d.any()


def test_the_kernel_cases_reach_every_branch():
    """what the scenes of tests/test_align_gpu.py are for, on the host's own counters: nothing measured; everything measured; contested pixels; footprints cut by every side of the
    grid; points behind the colour camera and close to its plane; cracks that the fill closes"""
    st = lambda n, sp=8, fl=1: S.align_depth_host(*AC.build(n), max_span=sp, fill=fl)["stats"]  # noqa: E731
    assert st("ragged_zero").tolist() == [[0, 0, 0, 0, 0]] and not S.align_depth_host(*AC.build("ragged_zero"))["depth"].any()
    assert st("ragged_plane")[0, 0] == 37 * 53 and st("ragged_plane")[0, 1] == 0
    for name in ("ragged_block", "up_block", "down_block"):  # the near block lands on the far plane's pixels: a twelfth of the writes is contested
        raw, cal, out_size = AC.build(name)
        t = S.scatter_terms_host(raw[0], cal[0], out_size)
        live = t["keep"] & (t["X0"] <= t["X1"]) & (t["Y0"] <= t["Y1"])
        writes = ((t["X1"] - t["X0"] + 1) * (t["Y1"] - t["Y0"] + 1))[live].sum()
        assert writes > 1.08 * st(name)[0, 3], (name, writes, st(name)[0, 3])
    raw, cal, out_size = AC.build("ragged_leaving")
    t = S.scatter_terms_host(raw[0], cal[0], out_size)
    k = t["keep"]
    assert ((t["x0"] < 0) & (t["x1"] >= 0) & k).any() and ((t["x1"] > out_size[1] - 1) & (t["x0"] <= out_size[1] - 1) & k).any()
    assert ((t["y0"] < 0) & (t["y1"] >= 0) & k).any() and ((t["y1"] > out_size[0] - 1) & (t["y0"] <= out_size[0] - 1) & k).any()
    for name in ("ragged_behind", "ragged_three", "up_three", "down_three"):
        s = st(name)[-1]
        assert s[1] > 0 and s[2] > 0 and s[3] > 0, (name, s)  # skipped behind the camera, too large close to its plane, and some of it seen
    assert st("up_block")[0, 4] > 0 and (st("up_three")[:, 3] > 0).all()
    assert st("ragged_plane", 1)[0, 2] > 0  # max_span = 1 refuses the footprints that span two pixels


def test_make_calib_and_the_host_checks():
    Km = np.asarray([[500.0, 0, 300.5], [0, 510.0, 200.25], [0, 0, 1]])
    c = S.make_calib(Km, K, AC.rot(0.1, 0.0), (1, 2, 3), 0.5)
    assert c.dtype == np.float32 and c.shape == (21,) and c[:8].tolist() == [500.0, 510.0, 300.5, 200.25, 600.0, 600.0, 320.0, 240.0]
    assert np.array_equal(c[8:17].reshape(3, 3), AC.rot(0.1, 0.0).astype(np.float32)) and c[17:].tolist() == [1.0, 2.0, 3.0, 0.5]
    raw = np.ones((1, 4, 4), np.uint16)
    for bad in (dict(max_span=0), dict(max_span=17), dict(fill=2)):
        with pytest.raises(ValueError):
            S.align_depth_host(raw, c[None], (4, 4), **bad)
    for i, v in ((0, 0.0), (5, -1.0), (20, 0.0), (9, np.nan), (18, np.inf)):
        b = c.copy()
        b[i] = v
        with pytest.raises(ValueError):
            S.align_depth_host(raw, b[None], (4, 4))
    with pytest.raises(ValueError):
        S.align_depth_host(raw.astype(np.int32), c[None], (4, 4))
    with pytest.raises(ValueError):
        S.align_depth_host(raw, np.stack([c, c]), (4, 4))


def test_the_interface_declares_exports_and_binds_the_entry():
    hdr = open(os.path.join(ROOT, "include", "kpf.h")).read()
    lib = L.load()
    abi = int(re.search(r"#define KPF_ABI_VERSION (\d+)", hdr).group(1))
    assert abi >= 35 and L.ABI_VERSION == abi and lib.kpf_abi_version() == abi
    assert "kpf_align_depth_u16" in L.EXPORTS and re.search(r"\bint kpf_align_depth_u16\(", hdr) and lib.kpf_align_depth_u16
    assert len(L._SIGS["kpf_align_depth_u16"]) == 13


_GOOD = dict(raw=True, Hd=6, Wd=8, calib=True, F=2, Hc=5, Wc=7, max_span=8, fill=1, zbuf=True, out=True, stats=True)
_NAN, _INF = float("nan"), float("inf")
REFUSED = [dict(raw=False), dict(calib=False), dict(zbuf=False), dict(out=False), dict(stats=False), dict(F=0), dict(F=33), dict(Hd=0), dict(Wd=-1), dict(Hc=0),
           dict(Wc=0), dict(Hd=4097, Wd=4096), dict(Hc=1 << 13, Wc=(1 << 11) + 1), dict(max_span=0), dict(max_span=17), dict(fill=2), dict(fill=-1),
           dict(cal=(1, 9, _NAN)), dict(cal=(0, 19, _INF)), dict(cal=(1, 0, 0.0)), dict(cal=(0, 1, -2.0)), dict(cal=(1, 4, 0.0)), dict(cal=(0, 5, -1.0)),
           dict(cal=(1, 20, 0.0)), dict(overlap=True)]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_a_refusal_comes_before_any_device_call_and_writes_nothing(bad):
    """the refusals need no GPU: the entry returns before its first launch, and host arrays filled with a sentinel stand in for the outputs.  The sizes
    of the two 2^24 cases are only named: a refusal reads none of the buffers but the calibration."""
    kw = dict(_GOOD)
    kw.update({k: v for k, v in bad.items() if k in kw})
    raw = np.full((2, 6, 8), 0x5A5A, np.uint16)
    cal = np.stack([S.make_calib(K, K), S.make_calib(K, K, unit_mm=0.5)])
    if "cal" in bad:
        cal[bad["cal"][0], bad["cal"][1]] = bad["cal"][2]
    zbuf, out, stats = np.full((2, 5, 7), 0x1234567, np.uint32), np.full((2, 5, 7), 0xBEEF, np.uint16), np.full((2, 5), -77, np.int32)
    before = [a.copy() for a in (raw, cal, zbuf, out, stats)]
    ptr = lambda a, on: a.ctypes.data if on else None  # noqa: E731
    out_ptr = raw.ctypes.data + 16 if bad.get("overlap") else ptr(out, kw["out"])
    lib = L.load()
    rc = lib.kpf_align_depth_u16(ptr(raw, kw["raw"]), kw["Hd"], kw["Wd"], ptr(cal, kw["calib"]), kw["F"], kw["Hc"], kw["Wc"], kw["max_span"], kw["fill"],
                                 ptr(zbuf, kw["zbuf"]), out_ptr, ptr(stats, kw["stats"]), None)
    assert rc != 0 and b"kpf_align_depth_u16" in lib.kpf_last_error(), (bad, lib.kpf_last_error())
    for a, b in zip((raw, cal, zbuf, out, stats), before):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert ctypes.sizeof(ctypes.c_float) * S.CALIB_FLOATS * S.MAX_FRAMES == 2688  # what travels with the scatter launch


def test_the_aligner_validates_on_the_host():
    import torch
    c = S.make_calib(K, K)
    with pytest.raises(RuntimeError):
        S.DepthAligner(c, (4, 4), (4, 4), torch.device("cpu"))
    for kw in (dict(max_span=0), dict(fill=3)):
        with pytest.raises(ValueError):
            S.DepthAligner(c, (4, 4), (4, 4), torch.device("cuda:0"), **kw)
    with pytest.raises(ValueError):
        S.DepthAligner(np.zeros((33, 21), np.float32) + 1, (4, 4), (4, 4), torch.device("cuda:0"))
    with pytest.raises(ValueError):
        S.DepthAligner(c, (4097, 4096), (4, 4), torch.device("cuda:0"))


def test_the_bench_tool_parses_and_names_its_record():
    """tools/align_bench.py needs the GPU to run; here it must at least be valid Python that writes where DESIGN.md 4.20 says"""
    import ast
    src = open(os.path.join(ROOT, "tools", "align_bench.py")).read()
    ast.parse(src)
    assert '"profiles", "align_bench.json"' in src and "DepthAligner" in src and "TrackedStream" in src
