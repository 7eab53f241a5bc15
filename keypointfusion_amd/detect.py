"""The hands found in the depth frame on the device, and lost tracks seeded from them (csrc/kpf_detect.hip).

Everything behind the camera here takes a box per track, and until now the first box -- and the box of a track that lost its hand -- came from outside.
HandDetector.detect applies the classic depth-camera rule to the registered depth frame: the hand is the part of the nearest connected surface that reaches
towards the camera (the assumption of the NYU, ICVL and MSRA pipelines, and of the reference's get_center_from_bbx with its 171 .. 1500 mm window).  Six
launches on the current stream for any content, no host wait, no allocation after the constructor, capturable; HandDetector.assign, one more launch, hands
the slots no live track stands on to the tracks that have none.  TrackedStream(detector=...) runs both at the head of its captured step.

The rule is this project's own, stated exactly in include/kpf.h and restated here by detect_hands_host and assign_host, the yardsticks: every output of
the kernels equals theirs, word for word.  The restatement labels by plain propagation (every pixel takes the smallest label among its joined neighbours until
nothing changes), the kernels by union-find, and label_union_host by a sequential union-find over the joins in any order: three routes to one labelling.

Per frame: (1) a pixel is valid when near <= d <= far; (2) two 4-neighbours are joined when both are valid and |d_a - d_b| <= step_mm, components are the
classes of that relation, a component's label is its smallest linear index r * W + c; (3) a component of fewer than min_pixels pixels is dropped; (4) its
near slab is its pixels with d <= z_min + reach_mm; (5) the slab's back-projected area, sum of d^2 / (fx fy), must lie in [min_area_mm2, max_area_mm2];
(6) the candidates are ranked by (z_min, label) and the first K fill the slots; (7) a slot's box is tracking.next_bbox of the slab's pixel bounds.

Limitation: two hands joined through the body inside [near, far] are ONE component, and only the nearer reaches the slots: set `far` to arm's length.  And
two live tracks that drift onto one hand are not resolved by the assignment."""
import numpy as np
import torch

from . import lib as L
from .tracking import next_bbox

MAX_FRAMES, MAX_PIXELS, MAX_SLOTS = 32, 1 << 24, 8
DEFAULTS = dict(near=171, far=1500, step_mm=20, reach_mm=150, min_pixels=64, min_area_mm2=2000.0, max_area_mm2=40000.0, expansion=1.25, slots=4)
STAT_NAMES = ("valid", "components", "kept", "candidates", "emitted")
INFO_NAMES = ("label", "z_min", "n", "slab", "area_mm2", "u", "v", "d")


def check_params(**params):
    """-> the nine parameters as a dict with the defaults filled in, refused as the entry refuses them"""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown detector parameter(s): %s" % ", ".join(sorted(unknown)))
    p = dict(DEFAULTS, **params)
    for k in ("near", "far", "step_mm", "reach_mm", "min_pixels", "slots"):
        if int(p[k]) != p[k]:
            raise ValueError("%s = %r is not an integer" % (k, p[k]))
        p[k] = int(p[k])
    for k in ("min_area_mm2", "max_area_mm2", "expansion"):
        p[k] = float(p[k])
    if not 0 <= p["near"] <= p["far"] <= 65535:
        raise ValueError("near = %d, far = %d: 0 <= near <= far <= 65535" % (p["near"], p["far"]))
    if not (0 <= p["step_mm"] <= 65535 and 0 <= p["reach_mm"] <= 65535):
        raise ValueError("step_mm = %d, reach_mm = %d outside 0..65535" % (p["step_mm"], p["reach_mm"]))
    if p["min_pixels"] < 1:
        raise ValueError("min_pixels = %d < 1" % p["min_pixels"])
    if not 1 <= p["slots"] <= MAX_SLOTS:
        raise ValueError("slots = %d outside 1..%d" % (p["slots"], MAX_SLOTS))
    if not (np.isfinite(p["min_area_mm2"]) and np.isfinite(p["max_area_mm2"]) and 0 <= p["min_area_mm2"] <= p["max_area_mm2"]):
        raise ValueError("area gate [%r, %r]: finite, 0 <= min <= max" % (p["min_area_mm2"], p["max_area_mm2"]))
    if not 0 < np.float32(p["expansion"]) < 1e6:
        raise ValueError("expansion = %r: a positive factor" % p["expansion"])
    return p


def check_cam(cam, frames=None):
    """-> cam as a contiguous float32 [F][4] (fx, fy, u0, v0), refused as the entry refuses it: every entry finite, the focal lengths positive"""
    c = np.ascontiguousarray(np.asarray(cam, np.float32))
    if c.ndim == 1:
        c = c[None]
    if c.ndim != 2 or c.shape[1] != 4 or not 1 <= c.shape[0] <= MAX_FRAMES:
        raise ValueError("cam must be [F][4] float32 (fx, fy, u0, v0) with 1 <= F <= %d (got %s)" % (MAX_FRAMES, c.shape))
    if frames is not None and c.shape[0] != frames:
        raise ValueError("cam holds %d frames, the depth %d" % (c.shape[0], frames))
    if not np.isfinite(c).all():
        raise ValueError("cam holds a value that is not finite")
    if not (c[:, :2] > 0).all():
        raise ValueError("cam: the focal lengths must be positive")
    return c


def _check_size(H, W):
    if min(H, W) < 1 or H * W > MAX_PIXELS:
        raise ValueError("a frame of %d x %d: every side >= 1 and at most 2^24 pixels" % (H, W))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the rule, in numpy
# ----------------------------------------------------------------------------------------------------------------------------------------
def joins_host(depth, near, far, step_mm):
    """one frame [H][W] uint16 -> (valid [H][W], right [H][W-1], down [H-1][W]): the pixel is valid; it is joined to its right / lower neighbour"""
    d = np.asarray(depth).astype(np.int64)
    valid = (d >= near) & (d <= far)
    right = valid[:, :-1] & valid[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= step_mm)
    down = valid[:-1] & valid[1:] & (np.abs(d[:-1] - d[1:]) <= step_mm)
    return valid, right, down


def label_propagate_host(depth, near, far, step_mm):
    """Steps 1 and 2 by propagation: label = index; every pixel takes the smallest label among itself and its joined neighbours, then the label of the pixel
    its label names (a pixel of the same component with a label no larger), until a round changes nothing.  -> [H][W] int64, -1 where invalid."""
    valid, right, down = joins_host(depth, near, far, step_mm)
    H, W = valid.shape
    lab = np.arange(H * W, dtype=np.int64).reshape(H, W)
    while True:
        new = lab.copy()
        np.minimum(new[:, :-1], np.where(right, lab[:, 1:], new[:, :-1]), out=new[:, :-1])
        np.minimum(new[:, 1:], np.where(right, lab[:, :-1], new[:, 1:]), out=new[:, 1:])
        np.minimum(new[:-1], np.where(down, lab[1:], new[:-1]), out=new[:-1])
        np.minimum(new[1:], np.where(down, lab[:-1], new[1:]), out=new[1:])
        if np.array_equal(new, lab):  # the fixed point of the neighbour step alone: the component's minimum everywhere
            break
        lab = new.reshape(-1)[new]
    return np.where(valid, lab, -1)


def label_union_host(depth, near, far, step_mm, order=None):
    """Steps 1 and 2 by a second, independent route: a sequential union-find over the joins, linking to the smaller index, the joins taken in row-major
    order (order None), reversed ("reversed") or shuffled by an integer seed.  -> [H][W] int64, -1 where invalid."""
    valid, right, down = joins_host(depth, near, far, step_mm)
    H, W = valid.shape
    ys, xs = np.nonzero(right)
    yd, xd = np.nonzero(down)
    a = np.concatenate([ys * W + xs, yd * W + xd])
    b = np.concatenate([ys * W + xs + 1, (yd + 1) * W + xd])
    sel = np.arange(a.size)
    if isinstance(order, str):
        if order != "reversed":
            raise ValueError("order = %r" % (order,))
        sel = sel[::-1]
    elif order is not None:
        sel = np.random.Generator(np.random.PCG64(int(order))).permutation(sel)
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(a[sel].tolist(), b[sel].tolist()):
        i, j = find(i), find(j)
        if i != j:
            parent[max(i, j)] = min(i, j)
    lab = np.array([find(x) for x in range(H * W)], np.int64).reshape(H, W)
    return np.where(valid, lab, -1)


def detect_hands_host(depth, cam, labeller=label_propagate_host, **params):
    """kpf_detect_hands_u16 in numpy, the yardstick and the documentation of the rule: depth [F][H][W] uint16 mm (or one frame [H][W]), cam [F][4] float32
    (fx, fy, u0, v0) -> dict(boxes [F][K][4] float64 xywh, valid [F][K] int32, info [F][K][8] float64 (label, z_min, n, slab count, area_mm2, centroid u,
    v, d; an empty slot holds label -1 and zeros), labels [F][H][W] int32 (-1: invalid pixels and dropped components), stats [F][5] int32 (valid pixels,
    components, components >= min_pixels, candidates, emitted)).  A slot whose box the rule refuses (next_bbox's None) has valid 0 and a zero box.
    Two hands joined through the body inside [near, far] are one component: only the nearer reaches the slots (set `far` to arm's length)."""
    p = check_params(**params)
    dep = np.asarray(depth)
    if dep.dtype != np.uint16:
        raise ValueError("depth must be uint16 (got %s)" % dep.dtype)
    if dep.ndim == 2:
        dep = dep[None]
    if dep.ndim != 3:
        raise ValueError("depth must be [F][H][W]")
    F, H, W = dep.shape
    _check_size(H, W)
    cam = check_cam(cam, F)
    K = p["slots"]
    out = dict(boxes=np.zeros((F, K, 4), np.float64), valid=np.zeros((F, K), np.int32), info=np.zeros((F, K, 8), np.float64),
               labels=np.full((F, H, W), -1, np.int32), stats=np.zeros((F, 5), np.int32))
    out["info"][:, :, 0] = -1.0
    rows, cols = np.mgrid[0:H, 0:W]
    for f in range(F):
        d = dep[f].astype(np.int64)
        lab = labeller(dep[f], p["near"], p["far"], p["step_mm"])
        ok = lab >= 0
        roots, n = np.unique(lab[ok], return_counts=True)
        cands = []
        keep = n >= p["min_pixels"]
        kept = int(keep.sum())
        lab[np.isin(lab, roots[~keep])] = -1
        for label, count in zip(roots[keep].tolist(), n[keep].tolist()):
            member = lab == label
            z_min = int(d[member].min())
            slab = member & (d <= z_min + p["reach_mm"])
            ds, us, vs = d[slab], cols[slab], rows[slab]
            S2 = int((ds * ds).sum())
            area = np.float64(S2) / (np.float64(cam[f, 0]) * np.float64(cam[f, 1]))
            if p["min_area_mm2"] <= area <= p["max_area_mm2"]:
                cnt = int(slab.sum())
                cands.append((z_min, label, count, cnt, area, np.float64(int(us.sum())) / np.float64(cnt), np.float64(int(vs.sum())) / np.float64(cnt),
                              np.float64(int(ds.sum())) / np.float64(cnt), (int(us.min()), int(vs.min()), int(us.max()), int(vs.max()))))
        cands.sort(key=lambda c: (c[0], c[1]))
        for k, c in enumerate(cands[:K]):
            x0, y0, x1, y1 = c[8]
            box = next_bbox(np.array([[x0, y0], [x1, y1]], np.float32), W, H, p["expansion"])
            out["info"][f, k] = (c[1], c[0], c[2], c[3], c[4], c[5], c[6], c[7])
            if box is not None:
                out["boxes"][f, k], out["valid"][f, k] = box, 1
        out["labels"][f] = lab
        out["stats"][f] = (int(ok.sum()), roots.size, kept, len(cands), min(len(cands), K))
    return out


def assign_host(boxes, valid, info, frame_size, frame_index, bbox, lost, seeded, reseed_after):
    """kpf_detect_assign_f64 in numpy.  boxes [F][K][4], valid [F][K], info [F][K][8]: a detector's slots; frame_size (H, W); frame_index [B]: each track's
    stored frame; the state bbox [B][4] float64, lost [B], seeded [B] -> (bbox, lost, seeded, reseeded), new arrays.
    A track is FREE when seeded == 0 or lost >= reseed_after, otherwise LIVE.  A valid slot is taken when its slab centroid (u, v) lies inside the box of a
    live track of its frame (x <= u < x + w and y <= v < y + h).  The free tracks of a frame, in track order, take its untaken slots in rank order: the
    slot's box, lost = 0, seeded = 1, reseeded = 1.  A free track that gets nothing and was never seeded holds the whole frame (0, 0, W, H)."""
    boxes, valid, info = np.asarray(boxes, np.float64), np.asarray(valid), np.asarray(info, np.float64)
    bbox, lost, seeded = np.array(bbox, np.float64), np.array(lost, np.int32), np.array(seeded, np.int32)
    F, K = valid.shape
    H, W = int(frame_size[0]), int(frame_size[1])
    B = bbox.shape[0]
    if int(reseed_after) < 1:
        raise ValueError("reseed_after = %r < 1" % (reseed_after,))
    reseeded = np.zeros(B, np.int32)
    free = (seeded == 0) | (lost >= int(reseed_after))
    for f in range(F):
        tracks = [b for b in range(B) if int(frame_index[b]) == f]
        open_ = [bool(valid[f, k]) for k in range(K)]
        for b in tracks:
            if not free[b]:
                x, y, w, h = bbox[b]
                for k in range(K):
                    u, v = info[f, k, 5], info[f, k, 6]
                    if x <= u < x + w and y <= v < y + h:
                        open_[k] = False
        untaken = [k for k in range(K) if open_[k]]
        for b in tracks:
            if not free[b]:
                continue
            if untaken:
                bbox[b] = boxes[f, untaken.pop(0)]
                lost[b], seeded[b], reseeded[b] = 0, 1, 1
            elif seeded[b] == 0:
                bbox[b] = (0.0, 0.0, float(W), float(H))
    return bbox, lost, seeded, reseeded


# ----------------------------------------------------------------------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------------------------------------------------------------------
class HandDetector:
    """HandDetector(cam_frames, frame_size, device, **params).detect(depth) -> dict(boxes, valid, info, labels, stats) of STATIC device tensors.

    cam_frames [F][4] (fx, fy, u0, v0) of each stored frame's camera (F <= 32), frame_size = (H, W) with H * W <= 2^24; params: DEFAULTS' names.  The
    camera rows and the parameters are validated here and travel with every launch; the buffers are allocated here and never again: per stored frame
    64 bytes a pixel of scratch (the parents and the words a component's root gathers) beside the labels."""

    def __init__(self, cam_frames, frame_size, device, **params):
        self.device = torch.device(device)
        self.cam = check_cam(cam_frames)
        self.params = check_params(**params)
        self.F, self.K = int(self.cam.shape[0]), self.params["slots"]
        self.H, self.W = int(frame_size[0]), int(frame_size[1])
        _check_size(self.H, self.W)
        if self.device.type != "cuda":
            raise RuntimeError("HandDetector lives on a GPU (there is no CPU fallback: detect.detect_hands_host is the host rule)")
        F, K, N, dev = self.F, self.K, self.H * self.W, self.device
        words = int(L.load().kpf_detect_ws64_words(F, self.H, self.W, K))
        if words < 0:
            raise ValueError("kpf_detect_ws64_words refused F=%d H=%d W=%d K=%d" % (F, self.H, self.W, K))
        self._ws32 = torch.empty(F * 8 * N, dtype=torch.int32, device=dev)
        self._ws64 = torch.empty(words, dtype=torch.int64, device=dev)
        self.boxes = torch.zeros(F, K, 4, dtype=torch.float64, device=dev)
        self.valid = torch.zeros(F, K, dtype=torch.int32, device=dev)
        self.info = torch.zeros(F, K, 8, dtype=torch.float64, device=dev)
        self.labels = torch.full((F, self.H, self.W), -1, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(F, 5, dtype=torch.int32, device=dev)

    def detect(self, depth):
        """depth [F][H][W] uint16 mm, registered to the camera of cam_frames (int16 storage is taken by its bits) -> the detector's own tensors,
        overwritten by the next call"""
        if not (torch.is_tensor(depth) and depth.dtype in (torch.uint16, torch.int16) and tuple(depth.shape) == (self.F, self.H, self.W)
                and depth.device == self.device and depth.is_contiguous()):
            raise ValueError("depth must be a contiguous 16-bit integer tensor of shape %s on %s" % ((self.F, self.H, self.W), self.device))
        p = self.params
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_detect_hands_u16(depth.data_ptr(), self.F, self.H, self.W, self.cam.ctypes.data, p["near"], p["far"], p["step_mm"],
                                                  p["reach_mm"], p["min_pixels"], p["min_area_mm2"], p["max_area_mm2"], p["expansion"], self.K,
                                                  self._ws32.data_ptr(), self._ws64.data_ptr(), self.boxes.data_ptr(), self.valid.data_ptr(),
                                                  self.info.data_ptr(), self.labels.data_ptr(), self.stats.data_ptr(),
                                                  torch.cuda.current_stream(self.device).cuda_stream), "kpf_detect_hands_u16")
        return dict(boxes=self.boxes, valid=self.valid, info=self.info, labels=self.labels, stats=self.stats)

    def assign(self, frame_index, bbox, lost, seeded, reseeded, reseed_after):
        """The slots of the last detect() handed to the tracks: frame_index [B] int32 (preprocess_gpu.make_frame_index), the state bbox [B][4] float64,
        lost, seeded [B] int32, updated IN PLACE, and reseeded [B] int32, rewritten; all device tensors.  assign_host states the rule."""
        B = int(frame_index.shape[0]) if torch.is_tensor(frame_index) and frame_index.dim() == 1 else -1
        for name, t, dtype, shape in (("frame_index", frame_index, torch.int32, (B,)), ("bbox", bbox, torch.float64, (B, 4)), ("lost", lost, torch.int32, (B,)),
                                      ("seeded", seeded, torch.int32, (B,)), ("reseeded", reseeded, torch.int32, (B,))):
            if not (torch.is_tensor(t) and B >= 1 and t.dtype == dtype and tuple(t.shape) == shape and t.device == self.device and t.is_contiguous()):
                raise ValueError("HandDetector.assign: %s must be a contiguous %s tensor %s on %s" % (name, dtype, shape, self.device))
        if int(reseed_after) != reseed_after or int(reseed_after) < 1:
            raise ValueError("HandDetector.assign: reseed_after = %r (an integer >= 1)" % (reseed_after,))
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_detect_assign_f64(self.boxes.data_ptr(), self.valid.data_ptr(), self.info.data_ptr(), self.F, self.K, self.W, self.H,
                                                   frame_index.data_ptr(), B, int(reseed_after), bbox.data_ptr(), lost.data_ptr(), seeded.data_ptr(),
                                                   reseeded.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "kpf_detect_assign_f64")
        return reseeded
