"""Device-resident mesh evaluation: the mesh counterpart of `evaluation_gpu.DeviceEvaluator`.

For a predicted mesh against a ground-truth mesh of the same V vertices (V = 778 for MANO): the per-vertex error, the same after the Umeyama similarity
alignment, the nearest-vertex distances in both directions, F-scores at given thresholds and the pooled vertex PCK curve / AUC -- the figures the HO3D /
FreiHAND servers report -- accumulated on the GPU by the two kpf_eval_mesh_* entry points of libkpf_hip.so (keypointfusion_amd/csrc/kpf_eval.hip;
arithmetic: include/kpf.h).  `evaluation_mesh` is the float64 yardstick (tests/test_evaluation_mesh_gpu.py pins this path to it).  `update` makes two launches
on the current stream, neither synchronises nor allocates (after the first call of a (device, B)) and can be captured in a `torch.cuda.graph`; `summary` makes
the only device -> host copy.  The arithmetic order is fixed, so the state after a sequence of batches is reproducible bit for bit.

    ev = DeviceMeshEvaluator()                                        # 778 vertices, PCK thresholds 0..50 mm in 100 steps, F-scores at 5 and 15 mm
    ev.update(mesh["verts3d"], gt_verts, valid=(mesh["status"] == 0).to(torch.uint8))
    figures = ev.summary()                                            # mean_error, pa_mean_error, f_score[5.0], pa_f_score[15.0], auc, ...

A sample whose predicted vertices all coincide has no alignment: its aligned errors are NaN and so are the aligned sums from then on (its aligned counts
are 0); the plain figures are unaffected.  Not covered: point-to-surface distances (the F-score is vertex to vertex), mesh-to-depth scoring
(`ManoFitter.render_depth`'s stats give that) and the HO3D json dump.
"""
import numpy as np
import torch

from . import evaluation_mesh as EM
from . import lib

MAX_VERTS, MAX_THRESHOLDS, MAX_F_THRESHOLDS = 1024, 256, 8  # MESH_MAX_V / MESH_MAX_T / MESH_MAX_TF of csrc/kpf_eval.hip


class DeviceMeshEvaluator:
    def __init__(self, verts=778, thresholds=(0.0, 50.0, 100), f_thresholds=(5.0, 15.0)):
        """verts: V, the vertices of both meshes.  thresholds: (val_min, val_max, steps) in mm for the PCK curve.  f_thresholds: the F-score thresholds in mm."""
        self.verts = int(verts)
        if not 1 <= self.verts <= MAX_VERTS:
            raise ValueError("DeviceMeshEvaluator: verts = %d (1 .. %d: both sets are held in LDS as float64)" % (self.verts, MAX_VERTS))
        lo, hi, steps = thresholds
        if not 2 <= int(steps) <= MAX_THRESHOLDS or not float(lo) < float(hi):
            raise ValueError("DeviceMeshEvaluator: thresholds = (val_min, val_max, steps) with val_min < val_max and 2 <= steps <= %d" % MAX_THRESHOLDS)
        self.thresholds = np.linspace(float(lo), float(hi), int(steps))  # numpy's bits: the table the device compares against
        self.f_thresholds = tuple(float(t) for t in f_thresholds)
        if not 1 <= len(self.f_thresholds) <= MAX_F_THRESHOLDS or any(not t >= 0.0 for t in self.f_thresholds) or len(set(self.f_thresholds)) != len(self.f_thresholds):
            raise ValueError("DeviceMeshEvaluator: f_thresholds must be 1 .. %d distinct distances >= 0 (got %r)" % (MAX_F_THRESHOLDS, f_thresholds))
        self.device = None
        self._state = None
        self._bufs = {}

    # -- state: one flat 8-byte buffer [int64 part | float64 part], so that reset() is one fill and summary() one copy
    def _layout(self):
        """[(name, shape, is_float, offset)], number of int64 elements, number of elements."""
        V, T, Tf = self.verts, len(self.thresholds), len(self.f_thresholds)
        fields, o = [], 0
        for name, shape, is_float in (("n_samples", (1,), False), ("n_batches", (1,), False), ("pck", (2, T), False),
                                      ("sum_mean_err", (2,), True), ("sum_vert", (2, V), True), ("sum_f", (2, Tf, 3), True)):
            fields.append((name, shape, is_float, o))
            o += int(np.prod(shape))
        return fields, 2 + 2 * T, o

    def _views(self, flat_i64, as_f64):
        fields, _, _ = self._layout()
        return {name: (as_f64(flat_i64[o:o + int(np.prod(shape))]) if is_float else flat_i64[o:o + int(np.prod(shape))]).reshape(shape)
                for name, shape, is_float, o in fields}

    def _bind(self, dev):
        if self._state is None:
            _, self._n_int, n_total = self._layout()
            with torch.cuda.device(dev):
                flat = torch.zeros(n_total, device=dev, dtype=torch.int64)
                self._state_views = self._views(flat, lambda t: t.view(torch.float64))
                self._th = torch.from_numpy(self.thresholds).to(dev)
                self._fth = torch.tensor(self.f_thresholds, dtype=torch.float64).to(dev)
            self._state, self.device = flat, dev
        elif dev != self.device:
            raise RuntimeError("DeviceMeshEvaluator: the state lives on %s, this batch is on %s (one evaluator per device; merge() combines them)" % (self.device, dev))

    def state(self):
        """The state tensors by name (views of one device buffer): n_samples, n_batches, pck [2][T] (int64), sum_mean_err [2], sum_vert [2][V],
        sum_f [2][Tf][3] (float64; F, P, R).  Leading index 0 plain, 1 aligned.  None before the first update() or merge()."""
        return None if self._state is None else dict(self._state_views)

    def reset(self):
        """Zero the state, asynchronously on the current stream."""
        if self._state is not None:
            self._state.zero_()

    def merge(self, other):
        """Add another evaluator's state (a data-parallel shard's) to this one's on the device: int64 and float64 adds.  The sums of the two parts are added
        as they are, which rounds differently from one evaluator that saw every batch; the integer state is exactly that evaluator's."""
        if not isinstance(other, DeviceMeshEvaluator):
            raise TypeError("DeviceMeshEvaluator.merge: expected a DeviceMeshEvaluator, got %s" % type(other).__name__)
        if (other.verts, other.f_thresholds) != (self.verts, self.f_thresholds) or not np.array_equal(other.thresholds, self.thresholds):
            raise ValueError("DeviceMeshEvaluator.merge: the two evaluators differ in vertices or thresholds")
        if other._state is None:
            return self
        self._bind(other.device if self._state is None else self.device)
        src = other._state.to(self.device)
        n = self._n_int
        self._state[:n] += src[:n]
        self._state[n:].view(torch.float64).add_(src[n:].view(torch.float64))
        return self

    # -- argument checks: nothing here touches a device
    def check_inputs(self, pred_verts, gt_verts, valid=None, pred_origin=None, gt_origin=None):
        """Validates one batch and returns B.  Raises TypeError / ValueError with the reason."""
        return self._check(pred_verts, gt_verts, valid, pred_origin, gt_origin)[0]

    def _check(self, pred_verts, gt_verts, valid, pred_origin, gt_origin):
        who, V = "DeviceMeshEvaluator.update", self.verts
        if (pred_origin is None) != (gt_origin is None):
            raise ValueError("%s: pred_origin and gt_origin are given together or not at all" % who)
        named = [("pred_verts", pred_verts), ("gt_verts", gt_verts)] + ([] if pred_origin is None else [("pred_origin", pred_origin), ("gt_origin", gt_origin)])
        for name, t in named:
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a torch tensor on the GPU (got %s)" % (who, name, type(t).__name__))
            if t.dtype != torch.float32:
                raise TypeError("%s: %s must be torch.float32 (got %s)" % (who, name, t.dtype))
        if gt_verts.dim() != 3 or tuple(gt_verts.shape[1:]) != (V, 3) or gt_verts.shape[0] < 1:
            raise ValueError("%s: gt_verts must be [B][%d][3] (got %s): V = %d vertices" % (who, V, tuple(gt_verts.shape), V))
        B = int(gt_verts.shape[0])
        if tuple(pred_verts.shape) != (B, V, 3):
            raise ValueError("%s: pred_verts must be [%d][%d][3] (got %s): V = %d vertices" % (who, B, V, tuple(pred_verts.shape), V))
        for name, t in named[2:]:
            if tuple(t.shape) != (B, 3):
                raise ValueError("%s: %s has shape %s, expected %s" % (who, name, tuple(t.shape), (B, 3)))
        if valid is not None:
            if not isinstance(valid, torch.Tensor):
                raise TypeError("%s: valid must be a torch.uint8 tensor [B] on the GPU (got %s)" % (who, type(valid).__name__))
            if valid.dtype != torch.uint8:
                raise TypeError("%s: valid must be torch.uint8 (got %s)" % (who, valid.dtype))
            if tuple(valid.shape) != (B,):
                raise ValueError("%s: valid has shape %s, expected %s" % (who, tuple(valid.shape), (B,)))
            named = named + [("valid", valid)]
        if B * V >= 1 << 28:
            raise ValueError("%s: B = %d samples of %d vertices: split the batch" % (who, B, V))
        return B, named

    def _buffers(self, dev, B):
        b = self._bufs.get((dev, B))
        if b is None:
            V, T, Tf = self.verts, len(self.thresholds), len(self.f_thresholds)
            b = dict(err=torch.zeros(2, B, V, device=dev, dtype=torch.float32), nn=torch.zeros(2, 2, B, V, device=dev, dtype=torch.float32),
                     nn_idx=torch.zeros(2, 2, B, V, device=dev, dtype=torch.int32), mean_err=torch.zeros(2, B, device=dev, dtype=torch.float64),
                     pck_cnt=torch.zeros(2, B, T, device=dev, dtype=torch.int32), f_cnt=torch.zeros(2, B, Tf, 2, device=dev, dtype=torch.int32))
            self._bufs[(dev, B)] = b
        return b

    def update(self, pred_verts, gt_verts, valid=None, pred_origin=None, gt_origin=None):
        """One batch: pred_verts, gt_verts [B][V][3] in mm, pred_origin / gt_origin None or [B][3] (subtracted from their set: root-relative figures):
        contiguous float32 tensors on one GPU.  valid: None, or [B] uint8 -- 0 drops a sample from the accumulation (a failed fit, or the padding of a last
        partial batch with B kept fixed for a captured graph); its logged values are computed all the same.  Returns a dict of views of this object's buffers
        for (device, B), which the next update() of the same B overwrites: err [2][B][V] float32 (0 plain, 1 aligned), nn [2][2][B][V] float32 and nn_idx
        [2][2][B][V] int32 (second index 0 pred -> gt, 1 gt -> pred), mean_err [2][B] float64, and the per-sample counts the accumulation adds up, pck_cnt
        [2][B][T] and f_cnt [2][B][Tf][2] int32."""
        B, named = self._check(pred_verts, gt_verts, valid, pred_origin, gt_origin)
        dev = gt_verts.device
        for name, t in named:
            if t.device.type != "cuda" or t.device != dev:
                raise RuntimeError("DeviceMeshEvaluator.update: %s is on %s; every input must be on the same GPU (there is no CPU fallback: "
                                   "evaluation_mesh.evaluate_meshes is the host path)" % (name, t.device))
            if not t.is_contiguous():
                raise ValueError("DeviceMeshEvaluator.update: %s must be contiguous" % name)
        l = lib.load()
        self._bind(dev)
        o = self._buffers(dev, B)
        V, T, Tf = self.verts, len(self.thresholds), len(self.f_thresholds)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            lib.check(l.kpf_eval_mesh_f32(pred_verts.data_ptr(), gt_verts.data_ptr(), ptr(pred_origin), ptr(gt_origin), self._th.data_ptr(), T,
                                          self._fth.data_ptr(), Tf, B, V, o["err"].data_ptr(), o["nn"].data_ptr(), o["nn_idx"].data_ptr(),
                                          o["mean_err"].data_ptr(), o["pck_cnt"].data_ptr(), o["f_cnt"].data_ptr(), st), "kpf_eval_mesh_f32")
            v = self._state_views
            lib.check(l.kpf_eval_mesh_accumulate(o["err"].data_ptr(), o["mean_err"].data_ptr(), o["pck_cnt"].data_ptr(), o["f_cnt"].data_ptr(), ptr(valid), B, V, T,
                                                 Tf, v["n_samples"].data_ptr(), v["n_batches"].data_ptr(), v["sum_mean_err"].data_ptr(), v["sum_vert"].data_ptr(),
                                                 v["pck"].data_ptr(), v["sum_f"].data_ptr(), st), "kpf_eval_mesh_accumulate")
        return dict(o)

    def summary(self):
        """One device -> host copy of the state, then a dict: samples, batches, mean_error (MPVPE: the mean over samples of the per-sample mean vertex error),
        per_vertex_mean [V], pck_curve [T] and auc over all vertices of all samples (`evaluation_mesh.mesh_pck_auc_from_counts`; thresholds:
        `self.thresholds`), f_score / precision / recall {threshold: mean over samples}, and the same keys with the prefix pa_ after the alignment."""
        if self._state is None:
            raise RuntimeError("DeviceMeshEvaluator.summary: nothing has been accumulated (no update() or merge() yet)")
        host = self._state.cpu().numpy()
        v = self._views(host, lambda a: a.view(np.float64))
        n, nb = int(v["n_samples"][0]), int(v["n_batches"][0])
        if n == 0:
            raise RuntimeError("DeviceMeshEvaluator.summary: nothing has been accumulated (no valid sample since reset())")
        out = {"samples": n, "batches": nb}
        for a, pre in ((0, ""), (1, "pa_")):
            out[pre + "mean_error"] = float(v["sum_mean_err"][a] / n)
            out[pre + "per_vertex_mean"] = v["sum_vert"][a] / n
            out[pre + "pck_curve"], out[pre + "auc"] = EM.mesh_pck_auc_from_counts(v["pck"][a], n * self.verts, self.thresholds)
            for c, key in enumerate(("f_score", "precision", "recall")):
                out[pre + key] = {tau: float(v["sum_f"][a, k, c] / n) for k, tau in enumerate(self.f_thresholds)}
        return out
