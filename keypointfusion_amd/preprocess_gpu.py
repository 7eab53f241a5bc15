"""Device-side RGB-D preprocessing: frames and bounding boxes in, the model's seven inputs out, joints back to frame pixels.

The batched, graph-capturable form of `preprocess.prepare_rgbd` (which stays the yardstick: tests/test_preprocess_gpu.py pins this path to it) on the three
kpf_prep_* entry points of libkpf_hip.so (keypointfusion_amd/csrc/kpf_prep.hip).  No host synchronisation and no allocation per call: the outputs of one
`(B, Hs, Ws)` are preallocated and reused, every input is a device tensor (so a captured graph picks up new frames, boxes and seeds), and the launches go
to the current stream.

    pre = DevicePreprocessor(img_size=128, sample_num=1024)
    prep = pre.prepare(rgb_u8, depth_u16, bbox, cam, seed)             # [B][H][W][3] uint8, [B][H][W] uint16, [B][4] f64, [B][4] f64, [B] int64
    res, sws, _ = plan.forward(*[prep[k] for k in MODEL_INPUTS], 0.8, 128, 1)
    crop_px, frame_px = pre.uncrop(res[5], prep)                       # joints in crop pixels and in frame pixels

By the dataset protocol (the reference's DexYCB / HO3D items at test time: the crop around an annotated 3-D centre, left hands mirrored, and the labels;
`preprocess.prepare_annotated` is the yardstick, tests/test_prep_annot_gpu.py pins this path to it bit for bit):

    prep = pre.prepare_annotated(rgb_u8, depth_u16, joints_mm, cam32, seed, mirror=left)   # [B][J][3] f32 mm, [B][4] f32, [B] int64, [B] uint8
    evaluator.update(res, prep["img"], prep["joint"], prep["center"], prep["M"], prep["cube"], prep["cam_para"])   # xyz_gt = prep["joint"]
    crop_px, frame_px = pre.uncrop(res[5], prep)                       # a mirrored sample's u comes back in the camera's own frame

Training from frames (the reference's items at TRAINING time: the same crop, then one of its augmentations per sample; `preprocess.prepare_augmented` is the
yardstick, tests/test_prep_augment_gpu.py pins this path to it bit for bit):

    prep = pre.prepare_augmented(rgb_u8, depth_u16, joints_mm, cam32, seed, mirror=left)   # parameters drawn on the device from seed, which advances by B
    loss = step(train_batch(prep))                                     # training.GraphedTrainStep: uvd_gt = prep["joint_img"], xyz_gt = prep["joint"]

A frame may be uploaded as a window: `origin=(x0, y0), frame_size=(H, W)` says where the stored [Hs][Ws] image sits in the camera frame; pixels outside
it read as zero.  The point sample is drawn from a counter hash of (seed[b], candidate) and is not numpy's RandomState stream: it has the same
distribution (n candidates without replacement in random order; a cloud smaller than n tiled first), see kpf_prep_pcl_sample in include/kpf.h.
"""
import torch

from . import lib

MODEL_INPUTS = ("img_rgb", "img", "pcl", "center", "M", "cube", "cam_para")  # the argument order of KPFusion.forward / plan.forward
MAX_PIXELS = 16384  # img_size ** 2: one 8-byte sort element per pixel in the 160-KiB LDS of a CU (kpf_prep_pcl_sample)


def _pow2ceil(v):
    return 1 << max(int(v) - 1, 0).bit_length()


def _named(rgb, depth, bbox, cam, seed, frame_index):
    named = (("rgb", rgb), ("depth", depth), ("bbox", bbox), ("cam", cam), ("seed", seed))
    return named if frame_index is None else named + (("frame_index", frame_index),)


def _check_tensors(where, table):
    """table: rows (name, tensor) or (name, tensor, shape, dtype).  Every row must be a torch tensor, and of that shape and dtype where they are given."""
    for name, t, *want in table:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch tensor on the GPU (got %s)" % (where, name, type(t).__name__))
        if want and tuple(t.shape) != want[0]:
            raise ValueError("%s: %s has shape %s, expected %s" % (where, name, tuple(t.shape), want[0]))
        if want and t.dtype != want[1]:
            raise TypeError("%s: %s must be %s (got %s)" % (where, name, want[1], t.dtype))


def _check_frames(where, rgb, depth, origin, frame_size, frame_index):
    """The stored frames, the frame index and the window of one batch (depth is uint16: each caller says why).  Returns (F, B, Hs, Ws, x0, y0, H, W): F stored
    frames, B samples (the length of frame_index when there is one)."""
    if rgb.dtype != torch.uint8:
        raise TypeError("%s: rgb must be torch.uint8 (got %s)" % (where, rgb.dtype))
    if depth.dim() != 3 or min(depth.shape) < 1:
        raise ValueError("%s: depth must be a non-empty [B][Hs][Ws] (got %s)" % (where, tuple(depth.shape)))
    F, Hs, Ws = (int(v) for v in depth.shape)
    if tuple(rgb.shape) != (F, Hs, Ws, 3):
        raise ValueError("%s: rgb %s does not match depth %s (expected [B][Hs][Ws][3])" % (where, tuple(rgb.shape), tuple(depth.shape)))
    B = F
    if frame_index is not None:
        if frame_index.dtype != torch.int32:
            raise TypeError("%s: frame_index must be torch.int32 (got %s): build it with make_frame_index" % (where, frame_index.dtype))
        if frame_index.dim() != 1 or frame_index.shape[0] < 1:
            raise ValueError("%s: frame_index has shape %s, expected [B]" % (where, tuple(frame_index.shape)))
        B = int(frame_index.shape[0])
    if (origin is None) != (frame_size is None):
        raise ValueError("%s: origin=(x0, y0) and frame_size=(H, W) go together" % where)
    x0, y0 = (0, 0) if origin is None else (int(origin[0]), int(origin[1]))
    H, W = (Hs, Ws) if frame_size is None else (int(frame_size[0]), int(frame_size[1]))
    if x0 < 0 or y0 < 0 or x0 + Ws > W or y0 + Hs > H:
        raise ValueError("%s: the %d x %d window at (%d, %d) leaves the %d x %d frame" % (where, Ws, Hs, x0, y0, W, H))
    return F, B, Hs, Ws, x0, y0, H, W


def _require_on(where, named, dev, host_path):
    """Every tensor of named (None: an optional one left out) on the GPU `dev` and contiguous; host_path: the function of preprocess.py to use instead."""
    for name, t in named:
        if t is None:
            continue
        if t.device.type != "cuda" or t.device != dev:
            raise RuntimeError("%s: %s is on %s; every input must be on the same GPU (there is no CPU fallback: preprocess.%s is the host path)"
                               % (where, name, t.device, host_path))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (where, name))


def _ptr(t):
    return None if t is None else t.data_ptr()


CROP_OUTPUTS = ("img", "img_rgb", "center", "M", "cube", "cam_para", "com", "bounds", "M64")  # the order the three crop entry points take them in


def make_frame_index(indices, frames, device):
    """[B] int32 device tensor for prepare(..., frame_index=): track b reads stored frame indices[b] of `frames`.  The values are checked HERE, on the host
    list, before anything reaches a device (the kernel clamps as well, but a wrong index is a caller's bug, not a frame to crop)."""
    try:
        idx = [int(v) for v in indices]
        exact = all(v == i for v, i in zip(indices, idx))
    except (TypeError, ValueError):
        idx, exact = [], False
    if isinstance(indices, torch.Tensor) or not exact or not idx:
        raise TypeError("make_frame_index: indices must be a non-empty host sequence of integers (got %r)" % (indices,))
    frames = int(frames)
    bad = [v for v in idx if not 0 <= v < frames]
    if bad:
        raise ValueError("make_frame_index: frame index %d outside [0, %d)" % (bad[0], frames))
    return torch.tensor(idx, dtype=torch.int32, device=device)


class DevicePreprocessor:
    def __init__(self, img_size=128, sample_num=1024, cube=(250.0, 250.0, 250.0), debug_candidates=False):
        """debug_candidates: prepare() also returns `candidates` [B][img_size**2][3], every foreground point at its candidate index (rows >= pcl_count
        are not written) — what `pcl_index` points into; for tests and debugging."""
        self.img_size, self.sample_num = int(img_size), int(sample_num)
        if not 0 < self.img_size ** 2 <= MAX_PIXELS:
            raise ValueError("DevicePreprocessor: img_size %d unsupported (img_size ** 2 <= %d)" % (self.img_size, MAX_PIXELS))
        if not 0 < self.sample_num <= self.img_size ** 2:
            raise ValueError("DevicePreprocessor: sample_num %d of at most img_size ** 2 = %d pixels" % (self.sample_num, self.img_size ** 2))
        if (_pow2ceil(self.img_size ** 2) + _pow2ceil(self.sample_num)) * 8 + 128 > 160 * 1024:
            raise ValueError("DevicePreprocessor: img_size %d with sample_num %d exceeds the LDS of a compute unit" % (self.img_size, self.sample_num))
        self.cube = tuple(float(c) for c in cube)
        if len(self.cube) != 3 or min(self.cube) <= 0:
            raise ValueError("DevicePreprocessor: cube is three positive sizes in mm")
        self.debug_candidates = bool(debug_candidates)
        self._bufs = {}

    # -- argument checks: nothing here touches a device
    @staticmethod
    def check_inputs(rgb, depth, bbox, cam, seed, origin=None, frame_size=None, frame_index=None):
        """Validates one batch and returns (B, Hs, Ws, x0, y0, H, W).  Raises TypeError / ValueError with the reason.  frame_index ([B] int32, from
        make_frame_index): rgb and depth hold F stored frames and B, the number of samples, is the length of the index."""
        where = "DevicePreprocessor.prepare"
        _check_tensors(where, _named(rgb, depth, bbox, cam, seed, frame_index))
        if depth.dtype != torch.uint16:
            raise TypeError("%s: depth must be torch.uint16 millimetres (got %s); the host path's z-clamp for float depth differs "
                            "and is not reproduced here: use preprocess.prepare_rgbd for float depth" % (where, depth.dtype))
        _, B, Hs, Ws, x0, y0, H, W = _check_frames(where, rgb, depth, origin, frame_size, frame_index)
        _check_tensors(where, (("bbox", bbox, (B, 4), torch.float64), ("cam", cam, (B, 4), torch.float64), ("seed", seed, (B,), torch.int64)))
        return B, Hs, Ws, x0, y0, H, W

    def _buffers(self, dev, B, Hs, Ws, kind, J=None):
        """This object's outputs for one shape.  kind: "crop" (prepare), "annot" (prepare_annotated) or "augment" (prepare_augmented): each path keeps a
        set of its own, so that the result of one outlives a call of another."""
        key = (dev, B, Hs, Ws, kind, J)
        b = self._bufs.get(key)
        if b is None:
            S, n = self.img_size, self.sample_num
            f32, f64, i32 = (dict(device=dev, dtype=dt) for dt in (torch.float32, torch.float64, torch.int32))
            b = dict(img_rgb=torch.zeros(B, 3, S, S, **f32), img=torch.zeros(B, 1, S, S, **f32), pcl=torch.zeros(B, n, 3, **f32), center=torch.zeros(B, 3, **f32),
                     M=torch.zeros(B, 3, 3, **f32), cube=torch.zeros(B, 3, **f32), cam_para=torch.zeros(B, 4, **f32), pcl_index=torch.zeros(B, n, **i32),
                     pcl_count=torch.zeros(B, **i32), com=torch.zeros(B, 3, **f64), bounds=torch.zeros(B, 6, **i32), M64=torch.zeros(B, 3, 3, **f64),
                     _cube64=torch.tensor([self.cube] * B, **f64))
            if kind != "crop":
                b.update(joint=torch.zeros(B, J, 3, **f32), joint_img=torch.zeros(B, J, 3, **f32), _cam64=torch.zeros(B, 4, **f64),
                         _right=torch.zeros(B, device=dev, dtype=torch.uint8))
            if kind == "augment":
                b.update(cube64=torch.zeros(B, 3, **f64), aug_status=torch.zeros(B, **i32), _pcl_seed=torch.zeros(B, device=dev, dtype=torch.int64),
                         _aug=dict(mode=torch.zeros(B, **i32), off=torch.zeros(B, 3, **f64), sc=torch.zeros(B, **f64), rot=torch.zeros(B, **f64),
                                   rot_cs=torch.zeros(B, 2, **f64), color=torch.zeros(B, 3, **f64)))
            if self.debug_candidates:
                b["candidates"] = torch.zeros(B, S * S, 3, **f32)
            self._bufs[key] = b
        return b

    def _sample(self, l, o, cube64, cam64_ptr, seed, st):
        """kpf_prep_pcl_sample on the crop in o: the point cloud, its candidate indices and the candidate count."""
        cand = o["candidates"].data_ptr() if self.debug_candidates else None
        lib.check(l.kpf_prep_pcl_sample(o["img"].data_ptr(), o["center"].data_ptr(), o["M64"].data_ptr(), cube64.data_ptr(), cam64_ptr, seed.data_ptr(),
                                        int(o["pcl_count"].shape[0]), self.img_size, self.sample_num, o["pcl"].data_ptr(), o["pcl_index"].data_ptr(),
                                        o["pcl_count"].data_ptr(), cand, st), "kpf_prep_pcl_sample")

    @staticmethod
    def _result(o, **extra):
        """The buffers a caller sees (not the ones named _...), plus what the path adds."""
        out = {k: v for k, v in o.items() if not k.startswith("_")}
        out.update(extra)
        return out

    def prepare(self, rgb, depth, bbox, cam, seed, origin=None, frame_size=None, frame_index=None):
        """rgb [B][Hs][Ws][3] uint8, depth [B][Hs][Ws] uint16 (mm), bbox [B][4] float64 (x, y, w, h; x, y the top-left corner), cam [B][4] float64
        (fx, fy, u0, v0), seed [B] int64: contiguous tensors on one GPU.  Returns a dict of device tensors: the keys of preprocess.prepare_rgbd that the
        model consumes (MODEL_INPUTS, batched) plus pcl_index [B][n] (candidate index of every sample, -1 for an empty cloud), pcl_count [B], com [B][3]
        float64, bounds [B][6] int32 (xs, xe, ys, ye, resize width, resize height) and M64 (M before its rounding to float32).  The tensors are this
        object's buffers for (B, Hs, Ws): the next prepare() of the same shape overwrites them.
        frame_index ([B] int32 device tensor of make_frame_index): several samples on one stored frame — rgb and depth are [F][Hs][Ws]..., sample b reads
        frame frame_index[b], and bbox, cam and seed stay [B].  Without it sample b reads frame b."""
        B, Hs, Ws, x0, y0, H, W = self.check_inputs(rgb, depth, bbox, cam, seed, origin, frame_size, frame_index)
        dev = depth.device
        _require_on("DevicePreprocessor.prepare", _named(rgb, depth, bbox, cam, seed, frame_index), dev, "prepare_rgbd")
        l = lib.load()
        o = self._buffers(dev, B, Hs, Ws, "crop")
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            tail = (bbox.data_ptr(), cam.data_ptr(), o["_cube64"].data_ptr(), B, Hs, Ws, x0, y0, H, W, self.img_size, *[o[k].data_ptr() for k in CROP_OUTPUTS], st)
            if frame_index is None:
                lib.check(l.kpf_prep_crop_u16(rgb.data_ptr(), depth.data_ptr(), *tail), "kpf_prep_crop_u16")
            else:
                lib.check(l.kpf_prep_crop_u16_indexed(rgb.data_ptr(), depth.data_ptr(), frame_index.data_ptr(), int(depth.shape[0]), *tail),
                          "kpf_prep_crop_u16_indexed")
            self._sample(l, o, o["_cube64"], cam.data_ptr(), seed, st)
        return self._result(o)

    # -- the dataset protocol
    @staticmethod
    def check_annotated(rgb, depth, joints_mm, cam, seed, mirror=None, center_xyz=None, origin=None, frame_size=None, frame_index=None):
        """Validates one annotated batch and returns (B, J, Hs, Ws, x0, y0, H, W).  Raises TypeError / ValueError with the reason; touches no device."""
        where = "DevicePreprocessor.prepare_annotated"
        if joints_mm is None and center_xyz is None:
            raise ValueError("%s: neither joints_mm nor center_xyz: nothing to crop around" % where)
        _check_tensors(where, [("rgb", rgb), ("depth", depth), ("cam", cam), ("seed", seed)] + [(k, v) for k, v in (
            ("joints_mm", joints_mm), ("mirror", mirror), ("center_xyz", center_xyz), ("frame_index", frame_index)) if v is not None])
        if depth.dtype != torch.uint16:
            raise TypeError("%s: depth must be torch.uint16 millimetres (got %s): the z-clamp truncates the near plane to the sensor's type" % (where, depth.dtype))
        _, B, Hs, Ws, x0, y0, H, W = _check_frames(where, rgb, depth, origin, frame_size, frame_index)
        J = 21
        if joints_mm is not None:
            if joints_mm.dim() != 3 or joints_mm.shape[0] != B or joints_mm.shape[2] != 3 or joints_mm.shape[1] < 1:
                raise ValueError("%s: joints_mm has shape %s, expected (%d, J, 3)" % (where, tuple(joints_mm.shape), B))
            J = int(joints_mm.shape[1])
            if J > 64:
                raise ValueError("%s: J = %d joints; at most 64 (one lane of a wave per joint)" % (where, J))
        checks = [("cam", cam, (B, 4), torch.float32), ("seed", seed, (B,), torch.int64)]
        checks += [("joints_mm", joints_mm, (B, J, 3), torch.float32)] if joints_mm is not None else []
        checks += [("center_xyz", center_xyz, (B, 3), torch.float32)] if center_xyz is not None else []
        checks += [("mirror", mirror, (B,), torch.uint8)] if mirror is not None else []
        _check_tensors(where, checks)
        return B, J, Hs, Ws, x0, y0, H, W

    def prepare_annotated(self, rgb, depth, joints_mm, cam, seed, mirror=None, center_xyz=None, origin=None, frame_size=None, frame_index=None):
        """The reference's dataset items at test time on the device (preprocess.prepare_annotated, bit for bit): the crop around an annotated 3-D centre, left
        hands mirrored, and the labels.  rgb, depth, seed, origin / frame_size and frame_index as prepare(); joints_mm [B][J][3] float32 (camera space, mm,
        the model's joint order; None with a given centre: no ground truth, the labels are zeros and J = 21), cam [B][4] float32 (fx, fy, u0, v0), mirror
        None or [B] uint8 (non-zero: a left hand), center_xyz None (the mean of the joints) or [B][3] float32.  Two launches, no allocation.  Returns
        prepare()'s dict plus joint [B][J][3] (normalised xyz: DeviceEvaluator.update's xyz_gt), joint_img [B][J][3] (normalised uvd), mirror ([B] uint8: the
        tensor given, or zeros) and frame_w (int, the width the mirror acts on); uncrop() takes a mirrored sample's u back to the camera's frame."""
        B, J, Hs, Ws, x0, y0, H, W = self.check_annotated(rgb, depth, joints_mm, cam, seed, mirror, center_xyz, origin, frame_size, frame_index)
        dev = depth.device
        _require_on("DevicePreprocessor.prepare_annotated", (("rgb", rgb), ("depth", depth), ("joints_mm", joints_mm), ("cam", cam), ("seed", seed), ("mirror", mirror),
                                                              ("center_xyz", center_xyz), ("frame_index", frame_index)), dev, "prepare_annotated")
        l = lib.load()
        o = self._buffers(dev, B, Hs, Ws, "annot", J)
        mir = o["_right"] if mirror is None else mirror
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            lib.check(l.kpf_prep_annot_u16(rgb.data_ptr(), depth.data_ptr(), _ptr(frame_index), int(depth.shape[0]), _ptr(joints_mm), cam.data_ptr(), _ptr(center_xyz),
                                           mir.data_ptr(), o["_cube64"].data_ptr(), B, J, Hs, Ws, x0, y0, H, W, self.img_size,
                                           *[o[k].data_ptr() for k in CROP_OUTPUTS + ("joint", "joint_img", "_cam64")], st), "kpf_prep_annot_u16")
            self._sample(l, o, o["_cube64"], o["_cam64"].data_ptr(), seed, st)
        return self._result(o, mirror=mir, frame_w=W)

    # -- training augmentation by the dataset protocol
    AUG_KEYS = (("mode", (), torch.int32), ("off", (3,), torch.float64), ("sc", (), torch.float64), ("rot", (), torch.float64), ("rot_cs", (2,), torch.float64))

    @staticmethod
    def check_augmented(rgb, depth, joints_mm, cam, seed, aug=None, mirror=None, center_xyz=None, origin=None, frame_size=None, frame_index=None,
                        sigma_com=10, sigma_sc=0.2, rot_range=180, color_factor=0):
        """Validates one batch for prepare_augmented and returns check_annotated's tuple.  Raises TypeError / ValueError with the reason; touches no device."""
        where = "DevicePreprocessor.prepare_augmented"
        if joints_mm is None:
            raise ValueError("%s: joints_mm is required: a training item has labels" % where)
        shape = DevicePreprocessor.check_annotated(rgb, depth, joints_mm, cam, seed, mirror, center_xyz, origin, frame_size, frame_index)
        B = shape[0]
        for name, v in (("sigma_com", sigma_com), ("sigma_sc", sigma_sc), ("rot_range", rot_range), ("color_factor", color_factor)):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not 0 <= float(v) < float("inf"):
                raise ValueError("%s: %s must be a finite number >= 0 (got %r)" % (where, name, v))
        if aug is not None:
            if not isinstance(aug, dict):
                raise TypeError("%s: aug must be a dict of device tensors (mode, off, sc, rot, rot_cs and optionally color), got %s" % (where, type(aug).__name__))
            keys = DevicePreprocessor.AUG_KEYS + ((("color", (3,), torch.float64),) if aug.get("color") is not None else ())
            _check_tensors(where, [("aug[%r]" % k, aug.get(k), (B,) + tail, dt) for k, tail, dt in keys])
        return shape

    def prepare_augmented(self, rgb, depth, joints_mm, cam, seed, aug=None, mirror=None, center_xyz=None, origin=None, frame_size=None, frame_index=None,
                          sigma_com=10, sigma_sc=0.2, rot_range=180, color_factor=0):
        """The reference's dataset items at TRAINING time on the device (preprocess.prepare_augmented, bit for bit): prepare_annotated's crop, then the
        reference's augmentation — one of rot / com / sc / none per sample — of both crops and the labels.  Inputs as prepare_annotated (joints_mm is
        required).  aug: dict of device tensors mode [B] int32 (0 rot, 1 com, 2 sc, 3 none), off [B][3], sc [B], rot [B] (degrees), rot_cs [B][2] = (cos,
        sin) of mod(rot, 360) pi / 180, optionally color [B][3], all float64.  aug=None: the parameters are DRAWN on the device from seed (the reference's
        rand_augment with sigma_com, sigma_sc, rot_range; color_factor > 0 also draws HO3D's colour scale; preprocess.draw_augment is the host twin), and seed
        is ADVANCED in place by B, so that the next call — or the next replay of a captured graph — draws anew; the point sample uses the seed before the
        advance.  Draw, crop and sample are three launches; no allocation.  Returns prepare_annotated's dict plus cube64, aug (the parameters used) and
        aug_status [B] int32 (bit 0: the depth side was augmented; bit 1: refused parameters — not finite, sc <= 0, degenerate bounds — prepared as mode
        none).  bounds are those of the base crop.  The result is marked `augmented`: uncrop() refuses it."""
        B, J, Hs, Ws, x0, y0, H, W = self.check_augmented(rgb, depth, joints_mm, cam, seed, aug, mirror, center_xyz, origin, frame_size, frame_index, sigma_com,
                                                          sigma_sc, rot_range, color_factor)
        dev = depth.device
        named = [("rgb", rgb), ("depth", depth), ("joints_mm", joints_mm), ("cam", cam), ("seed", seed), ("mirror", mirror), ("center_xyz", center_xyz),
                 ("frame_index", frame_index)] + [("aug[%r]" % k, v) for k, v in (aug or {}).items()]
        _require_on("DevicePreprocessor.prepare_augmented", named, dev, "prepare_augmented")
        l = lib.load()
        o = self._buffers(dev, B, Hs, Ws, "augment", J)
        mir = o["_right"] if mirror is None else mirror
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            pcl_seed = seed
            if aug is None:
                a = o["_aug"]
                pcl_seed = o["_pcl_seed"]
                pcl_seed.copy_(seed)  # (a device copy on the current stream: capturable)
                lib.check(l.kpf_prep_aug_draw(seed.data_ptr(), B, float(sigma_com), float(sigma_sc), float(rot_range), float(color_factor), B, a["mode"].data_ptr(),
                                              a["off"].data_ptr(), a["sc"].data_ptr(), a["rot"].data_ptr(), a["rot_cs"].data_ptr(), a["color"].data_ptr(), st),
                          "kpf_prep_aug_draw")
                used = dict(a) if float(color_factor) != 0 else {k: v for k, v in a.items() if k != "color"}
            else:
                used = {k: aug[k] for k in ("mode", "off", "sc", "rot", "rot_cs")}
                if aug.get("color") is not None:
                    used["color"] = aug["color"]
            lib.check(l.kpf_prep_augment_u16(rgb.data_ptr(), depth.data_ptr(), _ptr(frame_index), int(depth.shape[0]), joints_mm.data_ptr(), cam.data_ptr(),
                                             _ptr(center_xyz), mir.data_ptr(), o["_cube64"].data_ptr(), *[used[k].data_ptr() for k, _, _ in self.AUG_KEYS],
                                             _ptr(used.get("color")), B, J, Hs, Ws, x0, y0, H, W, self.img_size,
                                             *[o[k].data_ptr() for k in CROP_OUTPUTS + ("joint", "joint_img", "_cam64", "cube64", "aug_status")], st),
                      "kpf_prep_augment_u16")
            self._sample(l, o, o["cube64"], o["_cam64"].data_ptr(), pcl_seed, st)
        return self._result(o, mirror=mir, frame_w=W, aug=used, augmented=True)

    def uncrop(self, joints_nl, prep):
        """joints_nl [B][J][3] float32 normalised to the cube (the model's xyz outputs) + a prepare() result (or any dict with center, M, cube, cam_para)
        -> (crop_px [B][J][3]: u, v in crop pixels and d in mm; frame_px [B][J][3]: u, v in frame pixels and d in mm).  New tensors.  A
        prepare_annotated() result carries mirror and frame_w: a mirrored sample's frame u is frame_w - 1 - u, back in the camera's own frame (its depth and
        the predicted xyz stay in the mirrored camera's space, as in the reference)."""
        if prep.get("augmented"):
            raise ValueError("DevicePreprocessor.uncrop: an augmented crop is refused: after a rotation the crop is no longer an axis-aligned window of the "
                             "frame, and M alone does not take its pixels back (un-crop a prepare() or prepare_annotated() result)")
        if not isinstance(joints_nl, torch.Tensor) or joints_nl.dim() != 3 or joints_nl.shape[2] != 3 or joints_nl.dtype != torch.float32:
            raise ValueError("DevicePreprocessor.uncrop: joints must be a float32 tensor [B][J][3]")
        B, J = int(joints_nl.shape[0]), int(joints_nl.shape[1])
        dev = joints_nl.device
        if dev.type != "cuda":
            raise RuntimeError("DevicePreprocessor.uncrop: joints are on %s (no CPU fallback: preprocess.project_to_crop / uncrop_points are the host path)" % dev)
        par = []
        for k, shape in (("center", (B, 3)), ("M", (B, 3, 3)), ("cube", (B, 3)), ("cam_para", (B, 4))):
            t = prep[k]
            if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev:
                raise ValueError("DevicePreprocessor.uncrop: prep[%r] must be float32 %s on %s" % (k, shape, dev))
            par.append(t.contiguous())
        j = joints_nl.contiguous()
        crop_px, frame_px = torch.empty_like(j), torch.empty_like(j)
        mirror = prep.get("mirror")
        if mirror is not None:
            if not isinstance(mirror, torch.Tensor) or tuple(mirror.shape) != (B,) or mirror.dtype != torch.uint8 or mirror.device != dev:
                raise ValueError("DevicePreprocessor.uncrop: prep['mirror'] must be uint8 (%d,) on %s" % (B, dev))
            with torch.cuda.device(dev):
                lib.check(lib.load().kpf_prep_uncrop_mirror_f32(j.data_ptr(), *[t.data_ptr() for t in par], mirror.contiguous().data_ptr(), int(prep["frame_w"]),
                                                                B, J, crop_px.data_ptr(), frame_px.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                          "kpf_prep_uncrop_mirror_f32")
            return crop_px, frame_px
        with torch.cuda.device(dev):
            lib.check(lib.load().kpf_prep_uncrop_f32(j.data_ptr(), *[t.data_ptr() for t in par], B, J, crop_px.data_ptr(), frame_px.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream), "kpf_prep_uncrop_f32")
        return crop_px, frame_px


def train_batch(prep, epoch=None):
    """The dict GraphedTrainStep and training.kpfusion_loss take, from a prepare_augmented() (or prepare_annotated()) result: MODEL_INPUTS plus uvd_gt =
    joint_img and xyz_gt = joint, and `epoch` when given.  The tensors are the preprocessor's buffers, not copies."""
    missing = [k for k in MODEL_INPUTS + ("joint_img", "joint") if k not in prep]
    if missing:
        raise ValueError("train_batch: the preprocessing result has no %s: it takes a prepare_augmented() or prepare_annotated() result" % ", ".join(missing))
    batch = {k: prep[k] for k in MODEL_INPUTS}
    batch.update(uvd_gt=prep["joint_img"], xyz_gt=prep["joint"])
    if epoch is not None:
        batch["epoch"] = epoch
    return batch
