"""Device-resident evaluation: the figures of the reference's test loop (train.py:326-399) accumulated on the GPU, one transfer at the end.

The batched, graph-capturable form of `evaluation.evaluate_batch` + `evaluation.pck_auc` (which stay the yardsticks: tests/test_evaluation_gpu.py pins this path
to them) on the two kpf_eval_* entry points of libkpf_hip.so (keypointfusion_amd/csrc/kpf_eval.hip).  For every stage: the mean per-joint error, the
Procrustes-aligned mean error, and the PCK curve / AUC of both, over the whole threshold range and over 20-50 mm.  `update` neither synchronises nor allocates
(after the first call of a (device, B)) and goes to the current stream, so it can follow `serving.PipelinedEval.collect` without draining the pipeline and can be
captured in a `torch.cuda.graph`; `summary` makes the only device -> host copy.

    ev = DeviceEvaluator()                                                    # STAGE_TYPE (1, 1, 2, 3, 2, 3), 21 joints, thresholds 0..50 mm in 20 steps
    ev.update(results, img, xyz_gt, center, M, cube, cam_para, valid=None)    # per batch: at most five launches
    stages = ev.summary()                                                     # list of one dict per stage

Launches of one update: `kpf_inv3x3_f32` and one `kpf_offset2joint_f32` per dense stage (stage type 1, decoded as `evaluation.decode_stage` does: M^-1 and the
DEPTH image for both), then `kpf_eval_errors_f32` (one wave per sample and stage: errors and Umeyama alignment in float64, rounded once to float32) and
`kpf_eval_accumulate` (one workgroup per stage: sequential float64 sums, integer PCK counts).  The arithmetic order is fixed (include/kpf.h), so the state after a
sequence of batches is reproducible bit for bit, eagerly or from a replayed graph.

A sample whose predicted joints all coincide has no similarity alignment: its aligned errors are NaN (as in `evaluation.similarity_align` and the reference)
and so are the aligned sums from then on; the plain figures are unaffected.  Under stream capture, and on a host whose `torch.linalg.inv` follows neither known
rounding order (`inv3x3.host_mode() < 0`), M^-1 is computed on the device in the separately rounded order: M never leaves the device here.

Not reproduced: the STB translation-only alignment (train.py:349-352, which indexes the batch rather than the joint) and `z2error`.  The mesh is scored by
`evaluation_mesh_gpu.DeviceMeshEvaluator` (vertex errors, Procrustes, F-scores, vertex PCK: what the challenge server derives from the reference's mesh
dump); the json dump itself is not written.
"""
import ctypes as C

import numpy as np
import torch

from . import evaluation as EV
from . import lib

MAX_STAGES, MAX_JOINTS = 8, 64  # EVAL_MAX_STAGES / EVAL_MAX_JOINTS of csrc/kpf_eval.hip
DENSE_JOINTS, DENSE_CHANNELS = 21, 105  # kpf_offset2joint_f32 decodes 21 joints from 5 maps each


class DeviceEvaluator:
    def __init__(self, stage_type=EV.STAGE_TYPE, joints=21, score_joints=None, thresholds=(0.0, 50.0, 20), kernel=0.8, img_size=128, flip=1):
        """stage_type: per result 1 (dense offset maps, decoded here) or 2 / 3 (already xyz joints, read in place).  score_joints: None, or the joint indices
        that are scored, in order (`evaluation.NYU_SCORED_JOINTS` for NYU's 23 predicted joints); the alignment always uses all `joints`.  thresholds:
        (val_min, val_max, steps) in mm, as `evaluation.pck_auc` takes them."""
        self.stage_type = tuple(int(s) for s in stage_type)
        if not 1 <= len(self.stage_type) <= MAX_STAGES:
            raise ValueError("DeviceEvaluator: %d stages (1 .. %d)" % (len(self.stage_type), MAX_STAGES))
        if any(s not in (1, 2, 3) for s in self.stage_type):
            raise ValueError("DeviceEvaluator: stage types are 1 (dense), 2 or 3 (xyz), got %r" % (self.stage_type,))
        self.joints = int(joints)
        if not 1 <= self.joints <= MAX_JOINTS:
            raise ValueError("DeviceEvaluator: joints = %d (1 .. %d: one lane per joint)" % (self.joints, MAX_JOINTS))
        if 1 in self.stage_type and self.joints != DENSE_JOINTS:
            raise ValueError("DeviceEvaluator: dense stages decode %d joints, joints = %d" % (DENSE_JOINTS, self.joints))
        self.score_joints = None if score_joints is None else tuple(int(j) for j in score_joints)
        if self.score_joints is not None and (not 1 <= len(self.score_joints) <= MAX_JOINTS or any(not 0 <= j < self.joints for j in self.score_joints)):
            raise ValueError("DeviceEvaluator: score_joints must be 1 .. %d indices in [0, %d)" % (MAX_JOINTS, self.joints))
        self.scored = self.joints if self.score_joints is None else len(self.score_joints)
        lo, hi, steps = thresholds
        if int(steps) < 10 or not float(lo) < float(hi):
            raise ValueError("DeviceEvaluator: thresholds = (val_min, val_max, steps) with val_min < val_max and steps >= 10 (auc_20_50 starts at index 8)")
        self.thresholds = np.linspace(float(lo), float(hi), int(steps))  # numpy's bits: the table the device compares against
        self.kernel, self.img_size, self.flip = float(kernel), int(img_size), int(flip)
        self.device = None
        self._state = None
        self._bufs = {}

    # -- state: one flat 8-byte buffer [int64 part | float64 part], so that reset() is one fill and summary() one copy
    def _layout(self):
        """[(name, shape, is_float, offset)], number of int64 elements, number of elements."""
        S, Jq, T = len(self.stage_type), self.scored, len(self.thresholds)
        fields, o = [], 0
        for name, shape, is_float in (("n_samples", (1,), False), ("n_batches", (1,), False), ("pck", (S, Jq, T), False), ("pck_pa", (S, Jq, T), False),
                                      ("sum_err", (S, Jq), True), ("sum_pa", (S, Jq), True), ("sum_batch_mean", (S,), True), ("sum_batch_pa_mean", (S,), True)):
            fields.append((name, shape, is_float, o))
            o += int(np.prod(shape))
        return fields, 2 + 2 * S * Jq * T, o

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
                self._score = None if self.score_joints is None else torch.tensor(self.score_joints, device=dev, dtype=torch.int32)
            self._state, self.device = flat, dev
        elif dev != self.device:
            raise RuntimeError("DeviceEvaluator: the state lives on %s, this batch is on %s (one evaluator per device; merge() combines them)" % (self.device, dev))

    def state(self):
        """The state tensors by name (views of one device buffer): n_samples, n_batches, pck, pck_pa (int64), sum_err, sum_pa, sum_batch_mean,
        sum_batch_pa_mean (float64).  None before the first update() or merge()."""
        return None if self._state is None else dict(self._state_views)

    def reset(self):
        """Zero the state, asynchronously on the current stream."""
        if self._state is not None:
            self._state.zero_()

    def merge(self, other):
        """Add another evaluator's state (a data-parallel shard's) to this one's on the device: int64 and float64 adds.  The sums of the two parts are added
        as they are, which rounds differently from one evaluator that saw every batch; the integer state is exactly that evaluator's."""
        if not isinstance(other, DeviceEvaluator):
            raise TypeError("DeviceEvaluator.merge: expected a DeviceEvaluator, got %s" % type(other).__name__)
        if (other.stage_type, other.joints, other.score_joints) != (self.stage_type, self.joints, self.score_joints) or not np.array_equal(other.thresholds, self.thresholds):
            raise ValueError("DeviceEvaluator.merge: the two evaluators differ in stages, joints, scored joints or thresholds")
        if other._state is None:
            return self
        self._bind(other.device if self._state is None else self.device)
        src = other._state.to(self.device)
        n = self._n_int
        self._state[:n] += src[:n]
        self._state[n:].view(torch.float64).add_(src[n:].view(torch.float64))
        return self

    # -- argument checks: nothing here touches a device
    def check_inputs(self, results, img, xyz_gt, center, M, cube, cam_para, valid=None):
        """Validates one batch and returns B.  Raises TypeError / ValueError with the reason."""
        return self._check(results, img, xyz_gt, center, M, cube, cam_para, valid)[0]

    def _check(self, results, img, xyz_gt, center, M, cube, cam_para, valid):
        who = "DeviceEvaluator.update"
        if not isinstance(results, (list, tuple)) or len(results) != len(self.stage_type):
            raise ValueError("%s: results must be the list of %d stage outputs (got %s)" % (
                who, len(self.stage_type), len(results) if isinstance(results, (list, tuple)) else type(results).__name__))
        dense = 1 in self.stage_type
        named = [("results[%d]" % i, r) for i, r in enumerate(results)] + [("xyz_gt", xyz_gt), ("cube", cube)]
        if dense:
            named += [("img", img), ("center", center), ("M", M), ("cam_para", cam_para)]
        for name, t in named:
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a torch tensor on the GPU (got %s)" % (who, name, type(t).__name__))
            if t.dtype != torch.float32:
                raise TypeError("%s: %s must be torch.float32 (got %s)" % (who, name, t.dtype))
        J = self.joints
        if xyz_gt.dim() != 3 or tuple(xyz_gt.shape[1:]) != (J, 3) or xyz_gt.shape[0] < 1:
            raise ValueError("%s: xyz_gt must be [B][%d][3] (got %s): J = %d joints" % (who, J, tuple(xyz_gt.shape), J))
        B = int(xyz_gt.shape[0])
        for i, (r, st) in enumerate(zip(results, self.stage_type)):
            if st == 1:
                if r.dim() != 4 or r.shape[0] != B or r.shape[1] != DENSE_CHANNELS or r.shape[2] != r.shape[3]:
                    raise ValueError("%s: results[%d] (stage type 1) must be [%d][%d][F][F] offset maps (got %s)" % (who, i, B, DENSE_CHANNELS, tuple(r.shape)))
            elif tuple(r.shape) != (B, J, 3):
                raise ValueError("%s: results[%d] (stage type %d) must be [%d][%d][3] (got %s): J = %d joints" % (who, i, st, B, J, tuple(r.shape), J))
        shapes = [("cube", cube, (B, 3))]
        if dense:
            if img.dim() != 4 or img.shape[0] != B or img.shape[1] != 1 or img.shape[2] != img.shape[3]:
                raise ValueError("%s: img must be the [%d][1][S][S] depth crop (got %s)" % (who, B, tuple(img.shape)))
            shapes += [("center", center, (B, 3)), ("M", M, (B, 3, 3)), ("cam_para", cam_para, (B, 4))]
        for name, t, shape in shapes:
            if tuple(t.shape) != shape:
                raise ValueError("%s: %s has shape %s, expected %s" % (who, name, tuple(t.shape), shape))
        if valid is not None:
            if not isinstance(valid, torch.Tensor):
                raise TypeError("%s: valid must be a torch.uint8 tensor [B] on the GPU (got %s)" % (who, type(valid).__name__))
            if valid.dtype != torch.uint8:
                raise TypeError("%s: valid must be torch.uint8 (got %s)" % (who, valid.dtype))
            if tuple(valid.shape) != (B,):
                raise ValueError("%s: valid has shape %s, expected %s" % (who, tuple(valid.shape), (B,)))
            named = named + [("valid", valid)]
        if 2 * B * self.scored * 4 + B > 64 * 1024:
            raise ValueError("%s: B = %d samples of %d scored joints exceed the 64-KiB LDS plan of kpf_eval_accumulate: split the batch" % (who, B, self.scored))
        return B, named

    def _buffers(self, dev, B):
        b = self._bufs.get((dev, B))
        if b is None:
            f32 = dict(device=dev, dtype=torch.float32)
            b = dict(err=torch.zeros(2, len(self.stage_type), B, self.scored, **f32))
            if 1 in self.stage_type:
                b.update(minv=torch.zeros(B, 3, 3, **f32), uvd=torch.zeros(B, DENSE_JOINTS, 3, **f32),
                         xyz=[torch.zeros(B, DENSE_JOINTS, 3, **f32) if st == 1 else None for st in self.stage_type])
            self._bufs[(dev, B)] = b
        return b

    def update(self, results, img, xyz_gt, center, M, cube, cam_para, valid=None):
        """One batch: results = the model's stage outputs (float32; dense stages [B][105][F][F], xyz stages [B][J][3]), img [B][1][S][S] the depth crop,
        xyz_gt [B][J][3] normalised ground truth, center [B][3], M [B][3][3], cube [B][3], cam_para [B][4]: contiguous float32 tensors on one GPU (img, center,
        M and cam_para are only read when a stage is dense and may be None otherwise).  valid: None, or [B] uint8 — 0 drops a sample (the padding of a last
        partial batch, with B kept fixed for a captured graph).  Returns (joint_errors, pa_joint_errors), [S][B][Jsel] float32 in mm: views of this object's
        buffer for (device, B), which the next update() of the same B overwrites."""
        B, named = self._check(results, img, xyz_gt, center, M, cube, cam_para, valid)
        dev = xyz_gt.device
        for name, t in named:
            if t.device.type != "cuda" or t.device != dev:
                raise RuntimeError("DeviceEvaluator.update: %s is on %s; every input must be on the same GPU (there is no CPU fallback: "
                                   "evaluation.evaluate_batch and evaluation.pck_auc are the host-driven path)" % (name, t.device))
            if not t.is_contiguous():
                raise ValueError("DeviceEvaluator.update: %s must be contiguous" % name)
        l = lib.load()
        self._bind(dev)
        o = self._buffers(dev, B)
        S, J = len(self.stage_type), self.joints
        stages = (C.c_void_p * S)()
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            if 1 in self.stage_type:
                from .inv3x3 import host_mode
                lib.check(l.kpf_inv3x3_f32(M.data_ptr(), o["minv"].data_ptr(), B, max(host_mode(), 0), st), "kpf_inv3x3_f32")
            for i, (r, stype) in enumerate(zip(results, self.stage_type)):
                if stype == 1:  # evaluation.decode_stage: both dense stages with the DEPTH image (train.py:339)
                    lib.check(l.kpf_offset2joint_f32(r.data_ptr(), img.data_ptr(), center.data_ptr(), o["minv"].data_ptr(), cube.data_ptr(), cam_para.data_ptr(),
                                                     o["uvd"].data_ptr(), o["xyz"][i].data_ptr(), B, int(img.shape[-1]), int(r.shape[-1]), self.kernel, self.img_size,
                                                     self.flip, st), "kpf_offset2joint_f32")
                    stages[i] = o["xyz"][i].data_ptr()
                else:
                    stages[i] = r.data_ptr()
            lib.check(l.kpf_eval_errors_f32(stages, S, xyz_gt.data_ptr(), cube.data_ptr(), None if self._score is None else self._score.data_ptr(), B, J,
                                            self.scored, o["err"].data_ptr(), st), "kpf_eval_errors_f32")
            v = self._state_views
            lib.check(l.kpf_eval_accumulate(o["err"].data_ptr(), None if valid is None else valid.data_ptr(), self._th.data_ptr(), S, B, self.scored,
                                            len(self.thresholds), v["n_samples"].data_ptr(), v["n_batches"].data_ptr(), v["sum_err"].data_ptr(),
                                            v["sum_pa"].data_ptr(), v["sum_batch_mean"].data_ptr(), v["sum_batch_pa_mean"].data_ptr(), v["pck"].data_ptr(),
                                            v["pck_pa"].data_ptr(), st), "kpf_eval_accumulate")
        return o["err"][0], o["err"][1]

    def summary(self):
        """One device -> host copy of the state, then per stage a dict: samples, batches, mean_error / pa_mean_error (sample-weighted: sum / (n * Jsel)),
        mean_error_of_batch_means / pa_mean_error_of_batch_means (the two figures train.py:393-397 prints), per_joint_mean / pa_per_joint_mean [Jsel],
        pck_curve [T], auc, auc_20_50 and pa_pck_curve, pa_auc, pa_auc_20_50 (`evaluation.pck_auc_from_counts`).  Thresholds: `self.thresholds`."""
        if self._state is None:
            raise RuntimeError("DeviceEvaluator.summary: nothing has been accumulated (no update() or merge() yet)")
        host = self._state.cpu().numpy()
        v = self._views(host, lambda a: a.view(np.float64))
        n, nb = int(v["n_samples"][0]), int(v["n_batches"][0])
        if n == 0:
            raise RuntimeError("DeviceEvaluator.summary: nothing has been accumulated (no valid sample since reset())")
        out = []
        for s in range(len(self.stage_type)):
            auc, curve, _, sub = EV.pck_auc_from_counts(v["pck"][s], n, self.thresholds)
            pa_auc, pa_curve, _, pa_sub = EV.pck_auc_from_counts(v["pck_pa"][s], n, self.thresholds)
            out.append({"samples": n, "batches": nb,
                        "mean_error": float(np.sum(v["sum_err"][s]) / (n * self.scored)), "pa_mean_error": float(np.sum(v["sum_pa"][s]) / (n * self.scored)),
                        "mean_error_of_batch_means": float(v["sum_batch_mean"][s] / nb), "pa_mean_error_of_batch_means": float(v["sum_batch_pa_mean"][s] / nb),
                        "per_joint_mean": v["sum_err"][s] / n, "pa_per_joint_mean": v["sum_pa"][s] / n,
                        "pck_curve": curve, "auc": auc, "auc_20_50": sub, "pa_pck_curve": pa_curve, "pa_auc": pa_auc, "pa_auc_20_50": pa_sub})
        return out
