"""Hands tracked through a video on the device: the joints of frame t give the bounding box of frame t + 1.

The box rule is the reference loader's (dataloader/loader.py:1250-1251: `get_bbox(joints, expansion_factor=1.5)` then `process_bbox(bbox, width, height,
expansion_factor=1.0)`, :1432-1480).  `next_bbox` restates it on the host in the loader's own precisions and is the yardstick (tests/test_tracking_host.py pins
it to the reference bit for bit); `kpf_track_step_f32` (keypointfusion_amd/csrc/kpf_track.hip) evaluates the same arithmetic behind the forward and leaves the
next box in device memory, so the steady state of a stream is one captured graph per frame with only the frames uploaded:

    pre = DevicePreprocessor(img_size=128, sample_num=1024)
    ts = TrackedStream(model, pre, cam, frame_size=(480, 640), frames=1, frame_index=[0, 0])   # two hands in one camera frame
    ts.reseed(boxes)                             # [B][4] float64 (x, y, w, h) on the device: the first boxes, from outside -- or none at all:
    # TrackedStream(..., detector=detect.HandDetector(cam_frames, (480, 640), dev), reseed_after=3) finds the hands in the depth frame inside the step
    for rgb, depth in camera:                    # [F][H][W][3] uint8, [F][H][W] uint16 device tensors
        out = ts.step(rgb, depth)                # no host wait; out["frame_px"], out["cam_mm"], out["status"], out["lost"], ...

The reference has no video loop: the loop is an extension, the arithmetic of the box rule is the reference's.
"""
import numpy as np
import torch

from . import lib
from .preprocess_gpu import MODEL_INPUTS, make_frame_index

MAX_JOINTS = 64  # one lane of a wave64 per joint (kpf_track_step_f32)
STATUS_NO_BOX, STATUS_NO_FOREGROUND, STATUS_NOT_FINITE = 1, 2, 4  # bits of `status`


def next_bbox(joints_px, frame_w, frame_h, expansion=1.5):
    """joints_px [J][>= 2] float32 frame pixels (u, v, ...) -> the next frame's box as a float64 array (x, y, w, h), or None when the rule gives no box
    (coincident joints, joints outside the frame).  get_bbox in float32 — its inputs are float32 scalars, so every operation rounds to float32 — then
    process_bbox with expansion 1 and aspect ratio 1 in float64 on those four float32 values."""
    j = np.asarray(joints_px)
    if j.dtype != np.float32 or j.ndim != 2 or j.shape[0] < 1 or j.shape[1] < 2:
        raise ValueError("next_bbox: joints_px must be a float32 array [J][>= 2] (got %s %s)" % (j.dtype, j.shape))
    f32, e = np.float32, np.float32(expansion)

    def extent(col):  # (corner, size) of the joints' extent grown by e about its middle, float32 throughout
        lo, hi = col.min(), col.max()
        c = (lo + hi) / f32(2)
        w = (hi - lo) * e
        a = c - f32(0.5) * w
        b = c + f32(0.5) * w
        return a, b - a

    with np.errstate(over="ignore", invalid="ignore"):
        (bx, bw), (by, bh) = extent(j[:, 0]), extent(j[:, 1])
        assert bx.dtype == bw.dtype == np.float32
        bx, by, bw, bh = (np.float64(v) for v in (bx, by, bw, bh))
        zero = np.float64(0)
        pmax = lambda a, b: a if a >= b else b  # np.max / np.min over a pair, first argument first
        pmin = lambda a, b: a if a <= b else b
        x1, y1 = pmax(zero, bx), pmax(zero, by)
        x2 = pmin(np.float64(int(frame_w) - 1), x1 + pmax(zero, bw - 1))
        y2 = pmin(np.float64(int(frame_h) - 1), y1 + pmax(zero, bh - 1))
        if not (bw * bh > 0 and x2 >= x1 and y2 >= y1):
            return None
        w, h = x2 - x1, y2 - y1
        cx, cy = x1 + w / 2, y1 + h / 2
        if w > h:
            h = w
        elif w < h:
            w = h
        return np.array([cx - w / 2, cy - h / 2, w, h], np.float64)


def check_detector(detector, frames, height, width, device, reseed_after):
    """TrackedStream's refusal of a detect.HandDetector that does not read the stream's frames: their number, their size and the device must match"""
    if (detector.F, detector.H, detector.W) != (frames, height, width) or detector.device != device:
        raise ValueError("TrackedStream: the detector reads %d frames of %d x %d on %s, the stream holds %d of %d x %d on %s"
                         % (detector.F, detector.H, detector.W, detector.device, frames, height, width, device))
    if int(reseed_after) != reseed_after or int(reseed_after) < 1:
        raise ValueError("TrackedStream: reseed_after = %r (an integer >= 1)" % (reseed_after,))


class TrackedStream:
    """B tracks through a video of F stored frames per step: prepare (indexed) -> forward -> kpf_track_step_f32 on the current stream, no host wait.

    model: a KPFusion on the GPU in eval mode (its plan's forward gives the joints, results[stage]); pre: a DevicePreprocessor; cam [B][4] float64 device
    tensor (fx, fy, u0, v0) per track; frame_size (H, W); frames = F; frame_index: host list of B stored-frame numbers (None: F == B, track b on frame b).
    forward: any callable (prep, frame_no) -> joints [B][J][3] float32 normalised to the cube, in place of the model (other estimators, tests); frame_no is a
    one-element int64 DEVICE tensor holding the number of the frame in work, because a captured callable is replayed and can only read device memory.

    graph=True: frames 0 and 1 run eagerly (the warm-up, and real steps), frame 2 is captured and replayed, every later frame is one replay plus the copy of
    the frames into the static buffers.  Capturing executes nothing, so it neither advances nor disturbs the state; it waits for the device once.  A graphed
    and an eager stream give identical bits from frame 0.  `graph_replays` counts the replays.

    State (device, updated in place by every step): bbox [B][4] float64, seed [B] int64 (+ B per frame, so that no two (track, frame) share a seed), lost [B]
    int32 (frames since the last good box).  A frame with status != 0 keeps its box; reseed() writes detector boxes.

    aligner: a sensor.DepthAligner whose out_size is frame_size and which holds F frames -- step() then takes the RAW depth [F][Hd][Wd] of the depth sensor, and
    the body registers it to the colour camera (cam is the colour camera's) in front of prepare, inside the captured step; the step's outputs gain
    align_stats [F][5] int32.  None: depth arrives registered, and nothing of the aligner's runs.

    detector: a detect.HandDetector that holds F frames of frame_size on this device -- the body then finds the hands in the (registered) depth frame and
    hands the slots no live track stands on to the free tracks (never seeded, or lost >= reseed_after; detect.assign_host states the rule), behind the
    aligner and in front of prepare, inside the captured step: a stream starts without a box from outside and a lost track finds its hand again.  The
    state gains seeded [B] int32 (reseed() sets it for the tracks it writes), the outputs detections (the detector's dict), reseeded and seeded [B] int32.
    None: no tensor, launch or output is added."""

    def __init__(self, model, pre, cam, frame_size, frames, frame_index=None, expansion=1.5, stage=5, seed=0, graph=True, forward=None, aligner=None,
                 detector=None, reseed_after=3):
        if not isinstance(cam, torch.Tensor) or cam.dim() != 2 or cam.shape[1] != 4 or cam.dtype != torch.float64:
            raise ValueError("TrackedStream: cam must be a float64 tensor [B][4] (fx, fy, u0, v0)")
        if cam.device.type != "cuda":
            raise RuntimeError("TrackedStream: cam is on %s; the stream lives on a GPU (there is no CPU fallback: tracking.next_bbox is the host rule)" % cam.device)
        if model is None and forward is None:
            raise ValueError("TrackedStream: give a model or a forward= callable")
        self.model, self.pre, self.dev = model, pre, cam.device
        self.B, self.F = int(cam.shape[0]), int(frames)
        self.H, self.W = int(frame_size[0]), int(frame_size[1])
        if self.F < 1 or self.H < 1 or self.W < 1:
            raise ValueError("TrackedStream: frames = %d of %d x %d" % (self.F, self.H, self.W))
        if frame_index is None:
            if self.F != self.B:
                raise ValueError("TrackedStream: %d tracks on %d stored frames need a frame_index" % (self.B, self.F))
            frame_index = list(range(self.B))
        if len(frame_index) != self.B:
            raise ValueError("TrackedStream: frame_index has %d entries for %d tracks" % (len(frame_index), self.B))
        self.expansion, self.stage, self.graph = float(expansion), int(stage), bool(graph)
        if not self.expansion > 0:
            raise ValueError("TrackedStream: expansion must be positive")
        self._forward = forward
        dev, B = self.dev, self.B
        self.cam = cam.contiguous()
        self._fi = make_frame_index(frame_index, self.F, dev)
        self._rgb = torch.zeros(self.F, self.H, self.W, 3, dtype=torch.uint8, device=dev)  # the static inputs of the captured step
        self._depth = torch.zeros(self.F, self.H, self.W, dtype=torch.int16, device=dev).view(torch.uint16)  # (torch's 16-bit unsigned type has copies but few kernels: zeros come from int16)
        self.aligner, self._raw = aligner, None
        if aligner is not None:
            if (aligner.F, aligner.Hc, aligner.Wc) != (self.F, self.H, self.W) or aligner.device != dev:
                raise ValueError("TrackedStream: the aligner registers %d frames to %d x %d on %s, the stream holds %d of %d x %d on %s"
                                 % (aligner.F, aligner.Hc, aligner.Wc, aligner.device, self.F, self.H, self.W, dev))
            self._raw = torch.zeros(self.F, aligner.Hd, aligner.Wd, dtype=torch.int16, device=dev).view(torch.uint16)  # the static raw depth of the captured step
        self.detector, self.reseed_after, self.seeded, self.reseeded = detector, int(reseed_after), None, None
        if detector is not None:
            check_detector(detector, self.F, self.H, self.W, dev, reseed_after)
            self.seeded = torch.zeros(B, dtype=torch.int32, device=dev)
            self.reseeded = torch.zeros(B, dtype=torch.int32, device=dev)
        self.bbox = torch.zeros(B, 4, dtype=torch.float64, device=dev)
        self.seed = int(seed) + torch.arange(B, dtype=torch.int64, device=dev)
        self.lost = torch.zeros(B, dtype=torch.int32, device=dev)
        self.frame_no = torch.zeros(1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.bbox_used = torch.zeros(B, 4, dtype=torch.float64, device=dev)
        self._out = None  # crop_px, frame_px, cam_mm: allocated with the first joints (J)
        self._result = None
        self._graph = None
        self.frames_done = 0
        self.graph_replays = 0

    def reseed(self, bbox, mask=None):
        """Detector boxes [B][4] float64 (x, y, w, h; top-left) on the device: all tracks (the start of a stream), or the tracks where mask [B] bool is set
        (re-detection of lost ones).  A stream-ordered write into the state between two steps — graph replays included; enqueued, no wait."""
        if not isinstance(bbox, torch.Tensor) or tuple(bbox.shape) != (self.B, 4) or bbox.dtype != torch.float64 or bbox.device != self.dev:
            raise ValueError("TrackedStream.reseed: bbox must be a float64 tensor [%d][4] on %s" % (self.B, self.dev))
        if mask is None:
            self.bbox.copy_(bbox)
            self.lost.zero_()
            if self.seeded is not None:
                self.seeded.fill_(1)
            return
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (self.B,) or mask.dtype != torch.bool or mask.device != self.dev:
            raise ValueError("TrackedStream.reseed: mask must be a bool tensor [%d] on %s" % (self.B, self.dev))
        self.bbox.copy_(torch.where(mask.view(-1, 1), bbox, self.bbox))
        self.lost.copy_(torch.where(mask, torch.zeros_like(self.lost), self.lost))
        if self.seeded is not None:
            self.seeded.copy_(torch.where(mask, torch.ones_like(self.seeded), self.seeded))

    def _body(self):
        """One frame on the static buffers: what is captured.  Only launches on the current stream."""
        pre, B = self.pre, self.B
        align_stats = None
        if self.aligner is not None:  # the raw depth registered to the colour camera, into the static depth frame prepare reads
            align_stats = self.aligner.align(self._raw, out=self._depth)["stats"]
        detections = None
        if self.detector is not None:  # the hands of this frame, and the free tracks seeded from them: the boxes prepare is about to read
            detections = self.detector.detect(self._depth)
            self.detector.assign(self._fi, self.bbox, self.lost, self.seeded, self.reseeded, self.reseed_after)
        prep = pre.prepare(self._rgb, self._depth, self.bbox, self.cam, self.seed, frame_index=self._fi)
        if self._forward is not None:
            joints = self._forward(prep, self.frame_no)
            self.frame_no.add_(1)
        else:
            plan = self.model._plan(self.dev)
            res, _, _ = plan.forward(*[prep[k] for k in MODEL_INPUTS], 0.8, pre.img_size, 1)
            joints = res[self.stage]
        if not isinstance(joints, torch.Tensor) or joints.dim() != 3 or tuple(joints.shape[::2]) != (B, 3) or joints.dtype != torch.float32 or joints.device != self.dev:
            raise ValueError("TrackedStream: the forward must give float32 joints [%d][J][3] on %s" % (B, self.dev))
        J = int(joints.shape[1])
        if not 0 < J <= MAX_JOINTS:
            raise ValueError("TrackedStream: %d joints (kpf_track_step_f32 takes one lane of a wave64 per joint: J <= %d)" % (J, MAX_JOINTS))
        joints = joints.contiguous()
        if self._out is None or self._out[0].shape[1] != J:
            if self._graph is not None:
                raise RuntimeError("TrackedStream: the number of joints changed after the step was captured")
            self._out = tuple(torch.zeros(B, J, 3, dtype=torch.float32, device=self.dev) for _ in range(3))
        crop_px, frame_px, cam_mm = self._out
        with torch.cuda.device(self.dev):
            lib.check(lib.load().kpf_track_step_f32(joints.data_ptr(), prep["center"].data_ptr(), prep["M"].data_ptr(), prep["cube"].data_ptr(),
                                                    prep["cam_para"].data_ptr(), prep["pcl_count"].data_ptr(), B, J, self.W, self.H, self.expansion, B,
                                                    self.bbox.data_ptr(), self.seed.data_ptr(), self.lost.data_ptr(), crop_px.data_ptr(), frame_px.data_ptr(),
                                                    cam_mm.data_ptr(), self.bbox_used.data_ptr(), self.status.data_ptr(),
                                                    torch.cuda.current_stream(self.dev).cuda_stream), "kpf_track_step_f32")
        out = dict(frame_px=frame_px, crop_px=crop_px, cam_mm=cam_mm, bbox_used=self.bbox_used, bbox=self.bbox, status=self.status, lost=self.lost,
                   com=prep["com"], bounds=prep["bounds"], pcl_count=prep["pcl_count"], joints=joints,
                   pcl=prep["pcl"], cube=prep["cube"], center=prep["center"])  # what mano_fit.cloud_mm needs: the sampled depth points and their frame
        if align_stats is not None:
            out["align_stats"] = align_stats
        if detections is not None:
            out["detections"], out["reseeded"], out["seeded"] = detections, self.reseeded, self.seeded
        return out

    def step(self, rgb, depth):
        """rgb [F][H][W][3] uint8, depth [F][H][W] uint16 (mm) device tensors -> dict of STATIC device tensors, valid in stream order until the next step
        overwrites them: frame_px, crop_px [B][J][3] (u, v px, d mm), cam_mm [B][J][3], bbox_used [B][4] (this frame's box), bbox (the next frame's),
        status, lost [B] int32, and the prepare record com [B][3] float64, bounds [B][6], pcl_count [B] (+ joints, the forward's normalised output, and pcl
        [B][n][3], cube, center [B][3]: the sampled depth points normalised to the cube, mano_fit.cloud_mm(out) puts them back in camera space).
        With an aligner, depth is the depth sensor's raw frame [F][Hd][Wd] uint16 and the outputs hold align_stats [F][5] int32 as well; with a detector
        they hold detections (HandDetector.detect's dict), reseeded and seeded [B] int32."""
        depth_in = self._depth if self.aligner is None else self._raw
        for name, t, want in (("rgb", rgb, self._rgb), ("depth", depth, depth_in)):
            if not isinstance(t, torch.Tensor) or t.dtype != want.dtype or tuple(t.shape) != tuple(want.shape):
                raise ValueError("TrackedStream.step: %s must be %s %s (got %s)" % (name, want.dtype, tuple(want.shape),
                                                                                    (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
            if t.device != self.dev:
                raise RuntimeError("TrackedStream.step: %s is on %s, the stream on %s (no CPU fallback)" % (name, t.device, self.dev))
        with torch.no_grad(), torch.cuda.device(self.dev):
            self._rgb.copy_(rgb)
            depth_in.copy_(depth)
            if not self.graph or self.frames_done < 2:
                self._result = self._body()
            else:
                if self._graph is None:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):  # (records the launches of one frame, executes none: the state is as frame 1 left it)
                        self._result = self._body()
                    self._graph = graph
                self._graph.replay()
                self.graph_replays += 1
        self.frames_done += 1
        return self._result
