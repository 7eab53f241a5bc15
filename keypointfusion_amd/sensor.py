"""The depth stream registered to the colour camera on the device (csrc/kpf_align.hip).

A live RGB-D camera delivers depth and colour from two sensors with their own intrinsics, often their own resolution, a few centimetres apart; everything
behind the camera here (DevicePreprocessor.prepare, TrackedStream.step, FrameOverlay.draw) takes ONE cam and ONE box for both images.  DepthAligner.align
takes the raw depth frames and gives the depth image of the colour camera, uint16 mm on the colour grid, in three launches on the current stream: no host
wait, no allocation after the constructor, capturable -- TrackedStream(aligner=...) runs it in front of prepare inside its captured step.

The rule is this project's own, stated exactly in include/kpf.h and restated here operation by operation by align_depth_host, whose float32 form gives the
kernels' bits and whose float64 form is the yardstick for how much the float32 rounding decides.  Pinhole models on both sides: no lens distortion.

Pixel convention.  Pixel (c, r) is the point (c, r) and its footprint c +- 0.5, r +- 0.5: the frame-level convention of kpf_uncrop_joint
and of camera calibrations.  A raw pixel's footprint corners are carried to the colour image at the pixel's own depth; the colour pixels whose centres lie
inside the box of the two carried corners take the pixel's depth, the nearest depth winning a contested pixel."""
import numpy as np
import torch

from . import lib as L

CALIB_FLOATS = 21  # fxd, fyd, u0d, v0d, fxc, fyc, u0c, v0c, R[9] row-major, t[3] mm (depth camera -> colour camera), unit_mm
MAX_FRAMES, MAX_PIXELS, MAX_SPAN = 32, 1 << 24, 16
STAT_NAMES = ("valid", "skipped", "too_large", "covered", "filled")
EMPTY = 0xFFFFFFFF  # an untouched entry of the integer z-buffer


def make_calib(K_depth, K_color, R=None, t=None, unit_mm=1.0):
    """One calibration row [21] float32.  K_depth, K_color: (fx, fy, u0, v0) or a 3 x 3 intrinsic matrix; R [3][3] and t [3] (mm) carry a point of the
    depth camera's frame into the colour camera's, X_c = R X_d + t (None: the identity, zero); unit_mm: millimetres per raw count."""
    def k4(K):
        K = np.asarray(K, np.float64)
        if K.shape == (3, 3):
            return np.asarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
        if K.shape != (4,):
            raise ValueError("make_calib: intrinsics are (fx, fy, u0, v0) or a 3 x 3 matrix (got shape %s)" % (K.shape,))
        return K
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError("make_calib: R must be [3][3] and t [3]")
    return np.concatenate([k4(K_depth), k4(K_color), R.reshape(9), t, [float(unit_mm)]]).astype(np.float32)


def check_calib(calib, frames=None):
    """-> calib as a contiguous float32 [F][21], refused as the entry refuses it: every entry finite, the focal lengths and unit_mm positive"""
    c = np.ascontiguousarray(np.asarray(calib, np.float32))
    if c.ndim == 1:
        c = c[None]
    if c.ndim != 2 or c.shape[1] != CALIB_FLOATS or not 1 <= c.shape[0] <= MAX_FRAMES:
        raise ValueError("calib must be [F][%d] float32 with 1 <= F <= %d (got %s)" % (CALIB_FLOATS, MAX_FRAMES, c.shape))
    if frames is not None and c.shape[0] != frames:
        raise ValueError("calib holds %d frames, the depth %d" % (c.shape[0], frames))
    if not np.isfinite(c).all():
        raise ValueError("calib holds a value that is not finite")
    if not (c[:, [0, 1, 4, 5, 20]] > 0).all():
        raise ValueError("calib: the focal lengths and unit_mm must be positive")
    return c


def _check_sizes(Hd, Wd, Hc, Wc, max_span, fill):
    if min(Hd, Wd, Hc, Wc) < 1 or Hd * Wd > MAX_PIXELS or Hc * Wc > MAX_PIXELS:
        raise ValueError("frames of %d x %d -> %d x %d: every side >= 1 and at most 2^24 pixels a frame" % (Hd, Wd, Hc, Wc))
    if not 1 <= int(max_span) <= MAX_SPAN or int(max_span) != max_span:
        raise ValueError("max_span = %r outside 1..%d" % (max_span, MAX_SPAN))
    if fill not in (0, 1):
        raise ValueError("fill = %r is neither 0 nor 1" % (fill,))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the rule, in numpy: with dtype = float32 every product, sum, difference and quotient below is ONE float32 operation
# ----------------------------------------------------------------------------------------------------------------------------------------
def _carry(pu, pv, z, k):
    """a point (pu, pv) of the depth image at depth z -> (u, v, Zc) in the colour camera; k: the 21 calibration values in the working type"""
    X = ((pu - k[2]) / k[0]) * z
    Y = ((pv - k[3]) / k[1]) * z
    Xc = ((k[8] * X + k[9] * Y) + k[10] * z) + k[17]
    Yc = ((k[11] * X + k[12] * Y) + k[13] * z) + k[18]
    Zc = ((k[14] * X + k[15] * Y) + k[16] * z) + k[19]
    return (Xc * k[4]) / Zc + k[6], (Yc * k[5]) / Zc + k[7], Zc


def scatter_terms_host(raw, k, out_size, max_span=8, dtype=np.float32):
    """Steps 1 - 7 of the rule for ONE frame's valid pixels in row-major order: raw [Hd][Wd] uint16, k [21] -> dict(index (the flat raw index), d (the
    depth written, float), keep (neither skipped nor too large), too_large, x0, x1, y0, y1 (the unclamped rectangle, float), X0, X1, Y0, Y1 (clamped,
    float), ua, ub, va, vb, zm (the carried corners and the centre's Zc)).  The tests read the float64 form's terms for their boundary margins."""
    f = dtype
    Hc, Wc = int(out_size[0]), int(out_size[1])
    raw = np.asarray(raw)
    Wd = raw.shape[1]
    k = np.asarray(k, np.float32).astype(f)
    index = np.flatnonzero(raw.reshape(-1) > 0)
    q = raw.reshape(-1)[index]
    c, r = (index % Wd).astype(f), (index // Wd).astype(f)
    half = f(0.5)
    with np.errstate(all="ignore"):
        z = q.astype(f) * k[20]
        ua, va, za = _carry(c - half, r - half, z, k)
        ub, vb, zb = _carry(c + half, r + half, z, k)
        um, vm, zm = _carry(c, r, z, k)
        d = np.rint(zm)
        ok = (za > 0) & (zb > 0) & (zm > 0) & (d >= 1) & (d <= 65535)
        for v in (ua, va, za, ub, vb, zb, um, vm, zm):
            ok &= np.isfinite(v)
        x0, x1 = np.ceil(np.minimum(ua, ub)), np.ceil(np.maximum(ua, ub)) - f(1)
        y0, y1 = np.ceil(np.minimum(va, vb)), np.ceil(np.maximum(va, vb)) - f(1)
        too_large = ok & ((((x1 - x0) + f(1)) > f(max_span)) | (((y1 - y0) + f(1)) > f(max_span)))
        X0, X1 = np.maximum(x0, f(0)), np.minimum(x1, f(Wc - 1))  # clamped as floats: converted only where the rectangle is not empty
        Y0, Y1 = np.maximum(y0, f(0)), np.minimum(y1, f(Hc - 1))
    return dict(index=index, d=d, keep=ok & ~too_large, skipped=~ok, too_large=too_large, x0=x0, x1=x1, y0=y0, y1=y1, X0=X0, X1=X1, Y0=Y0, Y1=Y1,
                ua=ua, ub=ub, va=va, vb=vb, zm=zm)


def fill_host(unfilled):
    """The finish pass's fill on one unfilled map [H][W] uint16 -> (filled map, number of pixels filled): a 0 takes the smallest non-zero value of its
    4-neighbours if at least two of them are non-zero; the neighbours are read from the UNFILLED map, and outside the grid they count as 0"""
    u = np.asarray(unfilled, np.uint16)
    p = np.zeros((u.shape[0] + 2, u.shape[1] + 2), np.uint32)
    p[1:-1, 1:-1] = u
    nb = np.stack([p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]])
    take = (u == 0) & ((nb != 0).sum(0) >= 2)
    least = np.where(nb != 0, nb, np.uint32(EMPTY)).min(0)
    return np.where(take, least, u).astype(np.uint16), int(take.sum())


def align_depth_host(depth_raw, calib, out_size, max_span=8, fill=1, dtype=np.float32, _order=None):
    """kpf_align_depth_u16 in numpy, the yardstick and the documentation of the rule: depth_raw [F][Hd][Wd] uint16 (or one frame [Hd][Wd]), calib [F][21]
    (make_calib's rows), out_size (Hc, Wc) -> dict(depth [F][Hc][Wc] uint16 mm, stats [F][5] int32 = valid input pixels, skipped, too_large, covered output
    pixels before the fill, filled pixels).  dtype = float32 gives the kernels' bits; float64 is the same rule without the float32 roundings.
    _order: None, "reversed", or an integer seed of a random permutation -- the order in which the pixels are scattered, which the result does not depend on."""
    raw = np.asarray(depth_raw)
    if raw.dtype != np.uint16:
        raise ValueError("depth_raw must be uint16 (got %s)" % raw.dtype)
    if raw.ndim == 2:
        raw = raw[None]
    if raw.ndim != 3:
        raise ValueError("depth_raw must be [F][Hd][Wd]")
    F, Hd, Wd = raw.shape
    Hc, Wc = int(out_size[0]), int(out_size[1])
    cal = check_calib(calib, F)
    _check_sizes(Hd, Wd, Hc, Wc, max_span, fill)
    depth, stats = np.zeros((F, Hc, Wc), np.uint16), np.zeros((F, 5), np.int32)
    for fr in range(F):
        t = scatter_terms_host(raw[fr], cal[fr], (Hc, Wc), max_span, dtype)
        zbuf = np.full(Hc * Wc, EMPTY, np.uint32)
        live = t["keep"] & (t["X0"] <= t["X1"]) & (t["Y0"] <= t["Y1"])
        sel = np.flatnonzero(live)
        if _order == "reversed":
            sel = sel[::-1]
        elif _order is not None:
            sel = np.random.Generator(np.random.PCG64(int(_order))).permutation(sel)
        X0, X1, Y0, Y1 = (t[n][sel].astype(np.int64) for n in ("X0", "X1", "Y0", "Y1"))
        d = t["d"][sel].astype(np.uint32)
        for dy in range(int((Y1 - Y0).max()) + 1 if sel.size else 0):
            for dx in range(int((X1 - X0).max()) + 1):
                m = (Y0 + dy <= Y1) & (X0 + dx <= X1)
                np.minimum.at(zbuf, (Y0[m] + dy) * Wc + (X0[m] + dx), d[m])  # unbuffered: every pixel takes min(current, d), in the order given
        zbuf = zbuf.reshape(Hc, Wc)
        unfilled = np.where(zbuf == EMPTY, 0, zbuf).astype(np.uint16)
        depth[fr], filled = fill_host(unfilled) if fill else (unfilled, 0)
        stats[fr] = (t["index"].size, int(t["skipped"].sum()), int(t["too_large"].sum()), int((zbuf != EMPTY).sum()), filled)
    return dict(depth=depth, stats=stats)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------------------------------------------------------------------
class DepthAligner:
    """DepthAligner(calib, raw_size, out_size, device).align(depth_raw) -> dict(depth [F][Hc][Wc] uint16 mm, stats [F][5] int32), on the device.

    calib [F][21] (make_calib's rows, one per stored frame: F <= 32), raw_size = (Hd, Wd), out_size = (Hc, Wc); max_span 1..16: a raw pixel whose carried
    footprint spans more colour pixels than this in x or y writes nothing (stats' too_large); fill 0 or 1: close the one-pixel resampling cracks.  The
    calibration is validated here and travels with every launch; the buffers are allocated here and never again."""

    def __init__(self, calib, raw_size, out_size, device, max_span=8, fill=1):
        self.device = torch.device(device)
        self.calib = check_calib(calib)
        self.F = int(self.calib.shape[0])
        self.Hd, self.Wd, self.Hc, self.Wc = int(raw_size[0]), int(raw_size[1]), int(out_size[0]), int(out_size[1])
        _check_sizes(self.Hd, self.Wd, self.Hc, self.Wc, max_span, fill)
        self.max_span, self.fill = int(max_span), int(fill)
        if self.device.type != "cuda":
            raise RuntimeError("DepthAligner lives on a GPU (there is no CPU fallback: sensor.align_depth_host is the host rule)")
        self._zbuf = torch.empty(self.F, self.Hc, self.Wc, dtype=torch.int32, device=self.device)
        self._depth = torch.zeros(self.F, self.Hc, self.Wc, dtype=torch.int16, device=self.device).view(torch.uint16)
        self._stats = torch.zeros(self.F, 5, dtype=torch.int32, device=self.device)

    def align(self, depth_raw, out=None):
        """depth_raw [F][Hd][Wd] uint16 raw counts (int16 storage is taken by its bits) -> the aligner's own tensors, overwritten by the next call.
        out: a uint16 [F][Hc][Wc] tensor to write the depth into in place of the aligner's (TrackedStream's static depth frame)."""
        if not (torch.is_tensor(depth_raw) and depth_raw.dtype in (torch.uint16, torch.int16) and tuple(depth_raw.shape) == (self.F, self.Hd, self.Wd)
                and depth_raw.device == self.device and depth_raw.is_contiguous()):
            raise ValueError("depth_raw must be a contiguous 16-bit integer tensor of shape %s on %s" % ((self.F, self.Hd, self.Wd), self.device))
        depth = self._depth if out is None else out
        if not (torch.is_tensor(depth) and depth.dtype in (torch.uint16, torch.int16) and tuple(depth.shape) == (self.F, self.Hc, self.Wc)
                and depth.device == self.device and depth.is_contiguous()):
            raise ValueError("out must be a contiguous 16-bit integer tensor of shape %s on %s" % ((self.F, self.Hc, self.Wc), self.device))
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_align_depth_u16(depth_raw.data_ptr(), self.Hd, self.Wd, self.calib.ctypes.data, self.F, self.Hc, self.Wc, self.max_span,
                                                 self.fill, self._zbuf.data_ptr(), depth.data_ptr(), self._stats.data_ptr(),
                                                 torch.cuda.current_stream(self.device).cuda_stream), "kpf_align_depth_u16")
        return dict(depth=depth, stats=self._stats)
