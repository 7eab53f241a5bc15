"""Scenes and calibrations shared by tests/test_align_host.py and tests/test_align_gpu.py (keypointfusion_amd/sensor.py): raw depth frames
of a depth sensor, calibrations that carry them to a colour camera, and the margin bookkeeping of the float32-against-float64 comparison."""
import numpy as np

from keypointfusion_amd import sensor as S

T_MM = (15.0, -0.3, 1.2)  # a baseline of 15 mm with a little of the other two axes


def rot(about_y=0.0, about_x=0.0):
    cy, sy, cx, sx = np.cos(about_y), np.sin(about_y), np.cos(about_x), np.sin(about_x)
    return np.asarray([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.asarray([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def intrinsics(size, zoom=1.0):
    """(fx, fy, u0, v0) of a camera of `size` = (H, W) that sees about 58 degrees across; zoom > 1 narrows it"""
    H, W = size
    return (0.9 * W * zoom, 0.92 * W * zoom, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2)


def scaled(K, k):
    """the intrinsics of the same camera on a grid k times as fine (pixel centres at integers)"""
    fx, fy, u0, v0 = K
    return (k * fx, k * fy, k * u0 + (k - 1) / 2.0, k * v0 + (k - 1) / 2.0)


def calib(kind, raw_size, out_size, unit_mm=1.0):
    """general: a small rotation and a baseline of 15 mm; baseline: one of 150 mm, which carries a near surface well over the far one's pixels; leaving:
    the colour camera zoomed in, so that the footprints leave its grid on every side; behind: a wide colour camera standing INSIDE the scene, 850 mm in
    front of the depth camera and turned, so that part of the frame lies behind it, part close to its plane and part in view; identity: the same camera"""
    Kd = intrinsics(raw_size)
    if kind == "identity":
        return S.make_calib(Kd, Kd, unit_mm=unit_mm)
    if kind == "general":
        return S.make_calib(Kd, intrinsics(out_size), rot(0.01, 0.005), T_MM, unit_mm)
    if kind == "baseline":
        return S.make_calib(Kd, intrinsics(out_size), rot(0.01, 0.005), (150.0, -3.0, 12.0), unit_mm)
    if kind == "leaving":
        return S.make_calib(Kd, intrinsics(out_size, 1.7), rot(-0.02, 0.01), (-8.0, 5.0, -20.0), unit_mm)
    if kind == "behind":
        return S.make_calib(Kd, intrinsics(out_size, 0.5), rot(0.3, 0.05), (-250.0, 0.0, -850.0), unit_mm)
    raise KeyError(kind)


def scene(kind, raw_size, unit_mm=1.0, seed=0):
    """raw counts [Hd][Wd] uint16 of a scene in mm / unit_mm.  zero: nothing measured; plane: a tilted plane, every pixel valid; block: the plane with a
    near block in front of it (its pixels land on the plane's after the baseline) and holes"""
    H, W = raw_size
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "zero":
        return np.zeros((H, W), np.uint16)
    mm = 900.0 + 1.1 * xx * (160.0 / W) + 0.7 * yy * (120.0 / H)
    if kind == "block":
        g = np.random.Generator(np.random.PCG64(seed))
        mm[H // 4:(3 * H) // 5, W // 3:(2 * W) // 3] = 420.0 + 0.5 * yy[H // 4:(3 * H) // 5, W // 3:(2 * W) // 3]
        mm[g.random((H, W)) < 0.03] = 0.0
        mm[H // 8:H // 8 + 3, W // 8:W // 2] = 0.0
    elif kind != "plane":
        raise KeyError(kind)
    return np.rint(mm / unit_mm).astype(np.uint16)


# kernel cases: name -> (raw_size, out_size, [(scene, calibration, unit_mm) per stored frame])
SIZES = {"ragged": ((37, 53), (61, 83)), "same": ((64, 64), (64, 64)), "up": ((48, 64), (96, 128)), "down": ((96, 128), (48, 64))}
THREE = [("plane", "general", 1.0), ("block", "leaving", 0.25), ("block", "behind", 2.5)]  # three calibrations and units in one launch
CASES = {
    "ragged_zero": ("ragged", [("zero", "general", 1.0)]),
    "ragged_plane": ("ragged", [("plane", "general", 1.0)]),
    "ragged_block": ("ragged", [("block", "baseline", 1.0)]),
    "ragged_leaving": ("ragged", [("plane", "leaving", 1.0)]),
    "ragged_behind": ("ragged", [("plane", "behind", 1.0)]),
    "ragged_three": ("ragged", THREE),
    "same_identity": ("same", [("block", "identity", 1.0)]),
    "up_block": ("up", [("block", "baseline", 1.0)]),
    "up_three": ("up", THREE),
    "down_block": ("down", [("block", "baseline", 0.5)]),
    "down_three": ("down", THREE),
}


def build(name):
    """-> (depth_raw [F][Hd][Wd] uint16, calib [F][21] float32, out_size)"""
    sizes, frames = CASES[name]
    raw_size, out_size = SIZES[sizes]
    raw = np.stack([scene(s, raw_size, u, seed=i) for i, (s, _, u) in enumerate(frames)])
    cal = np.stack([calib(c, raw_size, out_size, u) for _, c, u in frames])
    return raw, cal, out_size


def _dilate4(m):
    p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), bool)
    p[1:-1, 1:-1] = m
    return m | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]


def undecided(raw, cal, out_size, max_span, margin=1e-4):
    """[Hc][Wc] bool: the colour pixels that a raw pixel reaches through a decision of the FLOAT64 rule that lies within `margin` of its boundary -- a
    rectangle edge within margin of an integer (the column or row that the edge's ceil moves over), or the centre's Zc within margin of a rounding
    boundary of d, of the range ends of d, or of 0 (the whole rectangle, one pixel beyond it).  Where float32 and float64 may legitimately part."""
    Hc, Wc = out_size
    t = S.scatter_terms_host(raw, cal, out_size, max_span, np.float64)
    mask = np.zeros((Hc, Wc), bool)

    def mark(x0, x1, y0, y1):
        x0, x1, y0, y1 = max(int(x0), 0), min(int(x1), Wc - 1), max(int(y0), 0), min(int(y1), Hc - 1)
        if x0 <= x1 and y0 <= y1:
            mask[y0:y1 + 1, x0:x1 + 1] = True

    lo_u, hi_u, lo_v, hi_v = np.minimum(t["ua"], t["ub"]), np.maximum(t["ua"], t["ub"]), np.minimum(t["va"], t["vb"]), np.maximum(t["va"], t["vb"])
    big = 1e9
    with np.errstate(all="ignore"):
        fin = np.isfinite(lo_u) & np.isfinite(hi_u) & np.isfinite(lo_v) & np.isfinite(hi_v) & np.isfinite(t["zm"]) & (np.abs(hi_u) < big) & (np.abs(lo_u) < big) \
            & (np.abs(hi_v) < big) & (np.abs(lo_v) < big)
        near = lambda a: np.abs(a - np.rint(a)) <= margin  # noqa: E731
        z_near = near(t["zm"] - 0.5) | (np.abs(t["zm"]) <= margin)
        edge = near(lo_u) | near(hi_u) | near(lo_v) | near(hi_v)
    for i in np.flatnonzero(fin & (z_near | edge)):
        x0, x1, y0, y1 = t["x0"][i], t["x1"][i], t["y0"][i], t["y1"][i]
        if max(x1 - x0, y1 - y0) + 2 > 4 * S.MAX_SPAN:
            continue  # far beyond any max_span in float32 as well: written by neither
        # the union of the rectangles on either side of the undecided edges: an edge within margin of the integer k gives x0 in {k, k + 1}, x1 in {k - 1, k}
        xs, xe = (np.rint(lo_u[i]) if near(lo_u[i]) else x0), (np.rint(hi_u[i]) if near(hi_u[i]) else x1)
        ys, ye = (np.rint(lo_v[i]) if near(lo_v[i]) else y0), (np.rint(hi_v[i]) if near(hi_v[i]) else y1)
        if z_near[i] or max(xe - xs, ye - ys) + 1 > max_span:  # the depth itself, or an edge that also decides the span test
            mark(xs, xe, ys, ye)
            continue
        for a in (lo_u[i], hi_u[i]):
            if near(a):
                mark(np.rint(a), np.rint(a), ys, ye)
        for a in (lo_v[i], hi_v[i]):
            if near(a):
                mark(xs, xe, np.rint(a), np.rint(a))
    return mask


def may_differ(raw, cal, out_size, max_span, fill, margin=1e-4):
    """undecided(), and with the fill the empty pixels next to an undecided one (the fill reads its 4-neighbours in the unfilled map)"""
    m = undecided(raw, cal, out_size, max_span, margin)
    if fill:
        u32 = S.align_depth_host(raw[None], cal[None], out_size, max_span, 0, np.float32)["depth"][0]
        u64 = S.align_depth_host(raw[None], cal[None], out_size, max_span, 0, np.float64)["depth"][0]
        m = m | (_dilate4(m) & ((u32 == 0) | (u64 == 0)))
    return m
