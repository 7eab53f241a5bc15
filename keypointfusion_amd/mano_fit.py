"""Joints to mesh: fit the MANO layer's pose, shape and a translation to 21 camera-space joints per hand — kpf_mano_fit_f32 (csrc/kpf_mano.hip).
The fit of one hand is independent of every other, so one workgroup runs all Adam iterations of one sample inside a single launch: state, moments and the
recomputed hand model stay on chip, and a call is one launch with no host wait and no device -> host copy (it can be captured in torch.cuda.graph).

Per sample  L = (1 / sum w) sum_i w_i |J_map[i](theta, beta) + t - y_i|^2 + lambda_shape |beta|^2 + lambda_pose |theta[3:]|^2  (mm^2), minimised by exactly
torch.optim.Adam's update (no weight decay, no amsgrad, moments zero at the start of every call), one learning rate each for pose, shape and translation.

Why eps defaults to 1.0 and not torch's 1e-8: with 1e-8 Adam's first steps are lr * sign(g), so a component whose gradient is rounding noise — the
translation right after init_trans, whose gradient is analytically zero — moves by a full step in a direction the noise picks.  On the CPU restatement of
this fit (tests/mano_cases.py) fp32 and float64 then part by 1 mm in the joints and 4 mm in the vertices after 10 steps; with eps = 1.0 (gradients are in
mm, so 1.0 is small against any gradient that matters) they agree to 1e-4 mm, and convergence is the same: 8.5 -> 1.5 mm in 50 steps against 8.5 -> 1.4 mm."""
import torch

from . import lib as L
from .heads import mano_model_arrays


class ManoFitter:
    """ManoFitter(sd_or_module, device, iters=50, lr=(pose, shape, trans), ...).fit(joints_mm) -> mesh, joints and MANO parameters of the fitted hands.

    sd_or_module: a state dict with the `mano_layer.th_*` buffers (keys may carry a prefix ending in `mano_layer.`), or a module that owns them
    (model.mano_head.mano_regHead).  joint_map[i] is the model joint, in the order of the head's `joints3d`, that target row i is compared with; the default is
    the identity.  Which permutation a dataset's joint order needs is the caller's business."""

    def __init__(self, sd_or_module, device, iters=50, lr=(0.02, 0.05, 1.0), eps=1.0, lambda_shape=1.0, lambda_pose=0.0, joint_map=None, betas=(0.9, 0.999)):
        sd = sd_or_module.state_dict() if hasattr(sd_or_module, "state_dict") else sd_or_module
        key = next((k for k in sd if k.endswith("mano_layer.th_shapedirs")), None)
        if key is None:
            raise KeyError("no mano_layer.th_shapedirs among the given tensors")
        self.device = torch.device(device)
        self.model = mano_model_arrays(sd, self.device, key[:-len("th_shapedirs")])
        jm = list(range(21)) if joint_map is None else [int(j) for j in joint_map]
        if sorted(jm) != list(range(21)):
            raise ValueError("joint_map must be a permutation of 0..20")
        self.cfg = L.ManoFitCfg(int(iters), float(lr[0]), float(lr[1]), float(lr[2]), float(betas[0]), float(betas[1]), float(eps), float(lambda_shape),
                                float(lambda_pose), 1, (L.C.c_int * 21)(*jm))
        self._bufs = {}

    def new_state(self, B):
        """(pose_aa [B, 48], betas [B, 10], trans [B, 3]) zeros: the cold start."""
        return tuple(torch.zeros(B, n, device=self.device, dtype=torch.float32) for n in (48, 10, 3))

    def _buffers(self, B):
        if B not in self._bufs:  # static per batch size: a captured graph keeps writing where it was captured
            e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
            self._bufs[B] = {"verts3d": e(B, 778, 3), "joints3d": e(B, 21, 3), "mano_pose": e(B, 16, 3, 3), "residual": e(B, 2),
                             "status": torch.empty(B, device=self.device, dtype=torch.int32), "state": self.new_state(B)}
        return self._bufs[B]

    def fit(self, joints_mm, weight=None, state=None, init_trans=True):
        """joints_mm [B, 21, 3] float32 on the device (mm, camera space), weight [B, 21] >= 0 or None (= ones).  state: None (start from zeros, in the
        fitter's own tensors) or the caller's (pose_aa, betas, trans), updated in place — the warm start from the previous video frame.  Cold-start on the
        first frame only (state=None, init_trans=True); a warm start passes init_trans=False so that the carried-over trans is used as given
        (init_trans=True replaces it by the weighted mean offset before iteration 1).

        Returns verts3d [B, 778, 3] and joints3d [B, 21, 3] (target order) in mm with the translation added, mano_pose_aa, mano_shape, trans (the state),
        mano_pose [B, 16, 3, 3] = rodrigues(mano_pose_aa), residual [B, 2] (mean weighted joint distance in mm before the first and after the last
        iteration) and status [B] int32 (bit 1: the weights sum to 0; bit 2: a target with positive weight is not finite; either way the state is left as
        it was and the outputs evaluate it).  The output tensors are the fitter's own, overwritten by the next call of the same batch size."""
        y = joints_mm
        B = y.shape[0]
        if not (y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (B, 21, 3)):
            raise ValueError("joints_mm must be a contiguous float32 [B, 21, 3] tensor on the device")
        if weight is not None and not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous() and tuple(weight.shape) == (B, 21)):
            raise ValueError("weight must be a contiguous float32 [B, 21] tensor on the device")
        o = self._buffers(B)
        if state is None:
            state = o["state"]
            for s in state:
                s.zero_()
        pose, betas, trans = state
        for s, n in zip(state, (48, 10, 3)):
            if not (s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and tuple(s.shape) == (B, n)):
                raise ValueError("state must be contiguous float32 tensors [B, 48], [B, 10], [B, 3] on the device")
        self.cfg.init_trans = 1 if init_trans else 0
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_fit_f32(y.data_ptr(), None if weight is None else weight.data_ptr(), *[m.data_ptr() for m in self.model],
                                              L.C.byref(self.cfg), pose.data_ptr(), betas.data_ptr(), trans.data_ptr(), o["verts3d"].data_ptr(),
                                              o["joints3d"].data_ptr(), o["mano_pose"].data_ptr(), o["residual"].data_ptr(), o["status"].data_ptr(), B,
                                              torch.cuda.current_stream().cuda_stream), "kpf_mano_fit_f32")
        return {"verts3d": o["verts3d"], "joints3d": o["joints3d"], "mano_pose_aa": pose, "mano_shape": betas, "trans": trans, "mano_pose": o["mano_pose"],
                "residual": o["residual"], "status": o["status"]}
