"""Joints to mesh: fit the MANO layer's pose, shape and a translation to 21 camera-space joints per hand — kpf_mano_fit_f32 (csrc/kpf_mano_fit.hip; the surface entries are in
csrc/kpf_mano_surface.hip).
The fit of one hand is independent of every other, so one workgroup runs all Adam iterations of one sample inside a single launch: state, moments and the
recomputed hand model stay on chip, and a call is one launch with no host wait and no device -> host copy (it can be captured in torch.cuda.graph).

Per sample  L = (1 / sum w) sum_i w_i |J_map[i](theta, beta) + t - y_i|^2 + lambda_shape |beta|^2 + lambda_pose |theta[3:]|^2  (mm^2), minimised by exactly
torch.optim.Adam's update (no weight decay, no amsgrad, moments zero at the start of every call), one learning rate each for pose, shape and translation.

Why eps defaults to 1.0 and not torch's 1e-8: with 1e-8 Adam's first steps are lr * sign(g), so a component whose gradient is rounding noise — the
translation right after init_trans, whose gradient is analytically zero — moves by a full step in a direction the noise picks.  On the CPU restatement of
this fit (tests/mano_cases.py) fp32 and float64 then part by 1 mm in the joints and 4 mm in the vertices after 10 steps; with eps = 1.0 (gradients are in
mm, so 1.0 is small against any gradient that matters) they agree to 1e-4 mm, and convergence is the same: 8.5 -> 1.5 mm in 50 steps against 8.5 -> 1.4 mm.

Joints put the mesh where 21 points on the skeleton can: the shape is barely observable and nothing ties the skin to the sensor.  fit_mesh adds a vertex term
(kpf_mano_fit_mesh_f32: 778 weighted vertex targets, a ground-truth mesh or the output of associate), associate gives every depth point its nearest vertex and
every vertex the weighted centroid of its points (kpf_mano_assoc_f32; sum_n w_n |V - p_n|^2 and W |V - c|^2 have the same gradient, so the fit needs no
atomics), and fit_cloud alternates the two on the depth points the preprocessing already sampled (cloud_mm).  DESIGN.md 4.12.

fit_gn is the joint fit by damped Gauss-Newton (kpf_mano_fit_gn_f32): the same objective and state, 8 iterations where Adam takes 50, one
launch; fit_cloud(joint_solver="gn") uses it for its first stage.  fit_mesh_gn is the same for the fit with the vertex term (kpf_mano_fit_mesh_gn_f32,
DESIGN.md 4.14); fit_cloud(cloud_solver="gn") uses it for its vertex rounds.

The surface: normals gives the mesh's area-weighted vertex normals from the model's faces (kpf_mano_normals_f32), associate(normals=...)
matches the depth points to the vertices that face the camera only (kpf_mano_assoc_vis_f32), fit_mesh_gn(vert_normal=...) measures the vertex term along the
normals (kpf_mano_fit_mesh_gn_plane_f32: one point-to-plane row per vertex, which does not punish sliding along the surface), and
fit_cloud(metric="plane") chains the three.

Self-occlusion: render_depth is a z-buffer render of the mesh into the crop's pixel grid (kpf_mano_raster_f32: depth, owning face, the
vertices hidden behind another part of the mesh, and the comparison with the observed depth crop), associate(vert_mask=...) keeps hidden vertices out of the
candidates (kpf_mano_assoc_vis_mask_f32), and fit_cloud(occlusion="zbuffer") chains them; crop_camera and crop_depth_mm take the camera, the crop map and
the observed depth from the preprocessing's outputs.

Free space: every row above starts from a depth point, so nothing tells the mesh where it must not be.  silhouette turns the observed
crop into per-pixel maps once per frame (kpf_depth_silhouette_f32: the nearest observed pixel, its distance, the nearest observed depth around it),
free_space gives every vertex that lies outside the observed silhouette, or in front of the observed surface, a target of its own in place of the cloud's
(kpf_mano_free_space_f32; csrc/kpf_mano_free.hip), and fit_cloud(free_space="silhouette") puts it between associate and fit_mesh_gn.  Off by default."""
import torch

from . import lib as L
from .heads import mano_faces, mano_model_arrays


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
        self.faces = mano_faces(sd, self.device, key[:-len("th_shapedirs")])  # [F, 3] int32 on the device, or None when the tensors carry no th_faces
        jm = list(range(21)) if joint_map is None else [int(j) for j in joint_map]
        if sorted(jm) != list(range(21)):
            raise ValueError("joint_map must be a permutation of 0..20")
        self.cfg = L.ManoFitCfg(int(iters), float(lr[0]), float(lr[1]), float(lr[2]), float(betas[0]), float(betas[1]), float(eps), float(lambda_shape),
                                float(lambda_pose), 1, (L.C.c_int * 21)(*jm))
        self.mesh_cfg = L.ManoFitMeshCfg(*[getattr(self.cfg, n) for n, _ in L.ManoFitCfg._fields_], 1.0)
        self.gn_cfg = L.ManoFitGnCfg(8, 0.1, 1e-2, float(lambda_shape), float(lambda_pose), 1, (L.C.c_int * 21)(*jm))
        self.mesh_gn_cfg = L.ManoFitMeshGnCfg(*[getattr(self.gn_cfg, n) for n, _ in L.ManoFitGnCfg._fields_], 1.0)
        self._bufs, self._mesh_bufs, self._assoc_bufs, self._gn_bufs, self._mesh_gn_bufs, self._normal_bufs = {}, {}, {}, {}, {}, {}
        self._raster_bufs = {}
        self._sil_bufs, self._free_bufs = {}, {}

    def new_state(self, B):
        """(pose_aa [B, 48], betas [B, 10], trans [B, 3]) zeros: the cold start."""
        return tuple(torch.zeros(B, n, device=self.device, dtype=torch.float32) for n in (48, 10, 3))

    def _fit_buffers(self, cache, B, res_w, **more):
        """A fit method's own outputs for batch size B, from its own cache (static per batch size: a captured graph keeps writing where it was captured).
        more: further entries of a new record (the Gauss-Newton methods' history={})."""
        if B not in cache:
            e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
            cache[B] = {"verts3d": e(B, 778, 3), "joints3d": e(B, 21, 3), "mano_pose": e(B, 16, 3, 3), "residual": e(B, res_w),
                        "status": torch.empty(B, device=self.device, dtype=torch.int32), "state": self.new_state(B), **more}
        return cache[B]

    def _take_state(self, o, state, B):
        """The caller's state, checked, or (None) the method's own, zeroed: the cold start."""
        if state is None:
            state = o["state"]
            for s in state:
                s.zero_()
        self._check_state(state, B)
        return state

    @staticmethod
    def _out_ptrs(o):
        return [o[k].data_ptr() for k in ("verts3d", "joints3d", "mano_pose", "residual", "status")]

    @staticmethod
    def _fit_result(o, state, **extra):
        out = {"verts3d": o["verts3d"], "joints3d": o["joints3d"], "mano_pose_aa": state[0], "mano_shape": state[1], "trans": state[2],
               "mano_pose": o["mano_pose"], "residual": o["residual"], "status": o["status"]}
        out.update(extra)
        return out

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
        self._check(y, (B, 21, 3), "joints_mm", "[B, 21, 3]")
        if weight is not None:
            self._check(weight, (B, 21), "weight", "[B, 21]")
        o = self._fit_buffers(self._bufs, B, 2)
        state = self._take_state(o, state, B)
        self.cfg.init_trans = 1 if init_trans else 0
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_fit_f32(y.data_ptr(), None if weight is None else weight.data_ptr(), *[m.data_ptr() for m in self.model],
                                              L.C.byref(self.cfg), *[s.data_ptr() for s in state], *self._out_ptrs(o), B,
                                              torch.cuda.current_stream().cuda_stream), "kpf_mano_fit_f32")
        return self._fit_result(o, state)

    def fit_gn(self, joints_mm, weight=None, state=None, init_trans=True, iters=None, mu=0.1, nu=1e-2, jacobian=False):
        """fit by damped Gauss-Newton (kpf_mano_fit_gn_f32): the same objective, state, targets, weights, joint_map and status convention,
        an order of magnitude fewer iterations.  Per iteration, with r_i = sqrt(w_i / sum w) (J_map[i] + t - y_i) and J = d r / d (pose, betas, trans):
        solve (J^T J + Lambda + mu diag(J^T J) + nu I) delta = J^T r + Lambda p by Cholesky and step p <- p - delta; the damping is fixed, nothing is
        accepted or rejected.  iters=None: 8 (the fitter's `iters` is Adam's); 0 <= iters <= 64.  mu = 0 diverges on real starts: keep the damping.

        Returns what fit returns plus history [B, iters + 1] (the mean weighted joint distance in mm before iteration 1 and after each iteration; its
        first and last entries are residual's) and, with jacobian=True, jacobian [B, 63, 61]: the unweighted d (J_map[i] + t) / d p of the state on entry,
        rows in target order.  status bit 4: the matrix was not positive definite -- the state holds the last completed iteration.  Own output tensors per
        batch size (and per iters, for history); one launch, no host wait."""
        B = joints_mm.shape[0]
        self._check(joints_mm, (B, 21, 3), "joints_mm")
        if weight is not None:
            self._check(weight, (B, 21), "weight")
        n = 8 if iters is None else int(iters)
        if not 0 <= n <= 64:
            raise ValueError("fit_gn takes 0 <= iters <= 64, not %d" % n)
        o = self._fit_buffers(self._gn_bufs, B, 2, history={})
        if n not in o["history"]:
            o["history"][n] = torch.empty(B, n + 1, device=self.device, dtype=torch.float32)
        if jacobian and "jacobian" not in o:
            o["jacobian"] = torch.empty(B, 63, 61, device=self.device, dtype=torch.float32)
        hist = o["history"][n]
        state = self._take_state(o, state, B)
        c = self.gn_cfg
        c.iters, c.mu, c.nu, c.init_trans = n, float(mu), float(nu), 1 if init_trans else 0
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_fit_gn_f32(joints_mm.data_ptr(), None if weight is None else weight.data_ptr(), *[m.data_ptr() for m in self.model],
                                                 L.C.byref(c), *[s.data_ptr() for s in state], *self._out_ptrs(o), hist.data_ptr(),
                                                 o["jacobian"].data_ptr() if jacobian else None, B, torch.cuda.current_stream().cuda_stream),
                    "kpf_mano_fit_gn_f32")
        return self._fit_result(o, state, history=hist, **({"jacobian": o["jacobian"]} if jacobian else {}))

    def _check_state(self, state, B):
        for s, n in zip(state, (48, 10, 3)):
            if not (s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and tuple(s.shape) == (B, n)):
                raise ValueError("state must be contiguous float32 tensors [B, 48], [B, 10], [B, 3] on the device")

    @staticmethod
    def _check(t, shape, name, said=None):  # said: how the refusal writes the shape (fit's says B), else the numbers
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError("%s must be a contiguous float32 %s tensor on the device" % (name, said or list(shape)))

    def fit_mesh(self, joints_mm=None, weight=None, vert_target=None, vert_weight=None, state=None, init_trans=True, lambda_verts=1.0, iters=None):
        """fit with a vertex term: + lambda_verts (1 / sum u) sum_v u_v |V_v + t - c_v|^2, vert_target c [B, 778, 3] in mm and vert_weight u [B, 778] >= 0
        (both or neither; neither is exactly fit).  joints_mm=None, or a weight of all zeros, is a vertex-only fit; then init_trans takes the translation
        from the vertices.  iters=None: the fitter's.  Returns what fit returns, with residual [B, 4]: the mean weighted joint distance before and after, then
        the mean weighted vertex distance before and after (0 for a term without weight); status bit 1 needs BOTH weight sums to be 0, bit 2 a non-finite
        joint or vertex target under a positive weight.  Own output tensors per batch size, apart from fit's; one launch, no host wait."""
        if (vert_target is None) != (vert_weight is None):
            raise ValueError("vert_target and vert_weight go together")
        given = [t for t in (joints_mm, vert_target, state[0] if state is not None else None) if t is not None]
        if not given:
            raise ValueError("fit_mesh needs joints_mm, vert_target or a state to take the batch size from")
        B = given[0].shape[0]
        if joints_mm is not None:
            self._check(joints_mm, (B, 21, 3), "joints_mm")
        if weight is not None:
            self._check(weight, (B, 21), "weight")
        if vert_target is not None:
            self._check(vert_target, (B, 778, 3), "vert_target")
            self._check(vert_weight, (B, 778), "vert_weight")
        o = self._fit_buffers(self._mesh_bufs, B, 4)
        state = self._take_state(o, state, B)
        c = self.mesh_cfg
        c.iters = self.cfg.iters if iters is None else int(iters)
        c.init_trans = 1 if init_trans else 0
        c.lambda_verts = float(lambda_verts)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_fit_mesh_f32(ptr(joints_mm), ptr(weight), ptr(vert_target), ptr(vert_weight), *[m.data_ptr() for m in self.model],
                                                   L.C.byref(c), *[s.data_ptr() for s in state], *self._out_ptrs(o), B,
                                                   torch.cuda.current_stream().cuda_stream), "kpf_mano_fit_mesh_f32")
        return self._fit_result(o, state)

    def fit_mesh_gn(self, joints_mm=None, weight=None, vert_target=None, vert_weight=None, state=None, init_trans=True, lambda_verts=1.0, iters=None,
                    mu=0.1, nu=1e-2, jacobian=False, vert_normal=None):
        """fit_mesh by damped Gauss-Newton (kpf_mano_fit_mesh_gn_f32): fit_gn's iteration over the 63 joint rows and the 2334 vertex rows
        sqrt(lambda_verts u_v / sum u) (V_v + t - c_v), with fit_mesh's arguments, init_trans rule and status bits 1 and 2, and fit_gn's bit 4.  iters=None: 8;
        0 <= iters <= 64.  Without vert_target the launch is fit_gn's kernel and its bits.

        Returns what fit_mesh returns plus history [B, iters + 1, 2] (the mean weighted joint and vertex distance in mm before iteration 1 and after each
        iteration) and, with jacobian=True, jacobian [B, 63, 61] (as fit_gn) and vert_jacobian [B, 2334, 61]: the unweighted d (V_v + t) / d p of the state
        on entry, row v * 3 + d (zeros without a vertex term).  Own output tensors per batch size (and per iters, for history); one launch, no host wait.

        vert_normal [B, 778, 3] (normals' output, fixed for the call): the vertex term becomes point-to-plane (kpf_mano_fit_mesh_gn_plane_f32),
        one row sqrt(lambda_verts u_v / sum u) n_v . (V_v + t - c_v) per vertex; the vertex columns of history and residual are then the mean weighted
        |n_v . (V_v + t - c_v)|, status bit 2 is also set by a non-finite normal under a positive weight, and a vertex term is required.  None: today's
        call and bits."""
        if (vert_target is None) != (vert_weight is None):
            raise ValueError("vert_target and vert_weight go together")
        if joints_mm is None and vert_target is None:
            raise ValueError("fit_mesh_gn needs joints_mm or vert_target")
        if vert_normal is not None and vert_target is None:
            raise ValueError("vert_normal needs vert_target and vert_weight")
        B = (joints_mm if joints_mm is not None else vert_target).shape[0]
        if joints_mm is not None:
            self._check(joints_mm, (B, 21, 3), "joints_mm")
        if weight is not None:
            self._check(weight, (B, 21), "weight")
        if vert_target is not None:
            self._check(vert_target, (B, 778, 3), "vert_target")
            self._check(vert_weight, (B, 778), "vert_weight")
        if vert_normal is not None:
            self._check(vert_normal, (B, 778, 3), "vert_normal")
        n = 8 if iters is None else int(iters)
        if not 0 <= n <= 64:
            raise ValueError("fit_mesh_gn takes 0 <= iters <= 64, not %d" % n)
        o = self._fit_buffers(self._mesh_gn_bufs, B, 4, history={})
        if n not in o["history"]:
            o["history"][n] = torch.empty(B, n + 1, 2, device=self.device, dtype=torch.float32)
        if jacobian and "jacobian" not in o:
            o["jacobian"] = torch.empty(B, 63, 61, device=self.device, dtype=torch.float32)
            o["vert_jacobian"] = torch.zeros(B, 2334, 61, device=self.device, dtype=torch.float32)
        hist = o["history"][n]
        state = self._take_state(o, state, B)
        c = self.mesh_gn_cfg
        c.iters, c.mu, c.nu, c.init_trans, c.lambda_verts = n, float(mu), float(nu), 1 if init_trans else 0, float(lambda_verts)
        if jacobian and vert_target is None:
            o["vert_jacobian"].zero_()
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        name = "kpf_mano_fit_mesh_gn_f32" if vert_normal is None else "kpf_mano_fit_mesh_gn_plane_f32"
        extra = [] if vert_normal is None else [vert_normal.data_ptr()]
        with torch.cuda.device(self.device):
            L.check(getattr(L.load(), name)(ptr(joints_mm), ptr(weight), ptr(vert_target), ptr(vert_weight), *extra, *[m.data_ptr() for m in self.model],
                                            L.C.byref(c), *[s.data_ptr() for s in state], *self._out_ptrs(o), hist.data_ptr(),
                                            o["jacobian"].data_ptr() if jacobian else None,
                                            o["vert_jacobian"].data_ptr() if jacobian and vert_target is not None else None, B,
                                            torch.cuda.current_stream().cuda_stream), name)
        return self._fit_result(o, state, history=hist, **({"jacobian": o["jacobian"], "vert_jacobian": o["vert_jacobian"]} if jacobian else {}))

    def normals(self, verts3d, sign=1.0, _slot=0):
        """verts3d [B, 778, 3] -> the area-weighted unit vertex normals [B, 778, 3] by the model's faces (th_faces, F <= 2048): sign * normalize(the sum of
        (v1 - v0) x (v2 - v0) over the corners of the faces at the vertex), (0, 0, 0) for a vertex in no face or a sum that is 0 or not finite.  sign = -1
        for a mirrored (left) hand or the other winding.  The fitter's own tensor per batch size; one launch, no host wait (kpf_mano_normals_f32)."""
        B = int(verts3d.shape[0])
        self._check(verts3d, (B, 778, 3), "verts3d")
        if self.faces is None:
            raise KeyError("no mano_layer.th_faces among the given tensors")
        if float(sign) not in (1.0, -1.0):
            raise ValueError("sign must be +1 or -1, not %r" % (sign,))
        key = (B, _slot)
        if key not in self._normal_bufs:
            self._normal_bufs[key] = torch.empty(B, 778, 3, device=self.device, dtype=torch.float32)
        out = self._normal_bufs[key]
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_normals_f32(verts3d.data_ptr(), self.faces.data_ptr(), int(self.faces.shape[0]), float(sign), out.data_ptr(), B,
                                                  torch.cuda.current_stream().cuda_stream), "kpf_mano_normals_f32")
        return out

    def render_depth(self, verts3d, cam, M=None, size=(128, 128), margin=10.0, depth_obs=None, _slot=0):
        """z-buffer render of the mesh into a crop's pixel grid (kpf_mano_raster_f32).  verts3d [B, 778, 3] mm in the camera frame of
        cloud_mm; cam [B, 4] = fx, fy, u0, v0 and M [B, 2, 3], the map from frame pixels to crop coordinates (crop_camera's; None: the identity -- a render
        into the frame's own top-left window); size = (H, W), H * W <= 16384; depth_obs [B, H, W] mm or None (crop_depth_mm's).  Crop pixel (c, r) is sampled
        where the preprocessing back-projects it from, (c + 0.5, r + 0.5).  Two-sided, no near-plane clipping: a face with a vertex at z <= 0 is dropped.

        Returns depth [B, H, W] (mm, 0 = background), face [B, H, W] int32 (the owning face, -1 = background), occluded [B, 778] int32 (1: the vertex lies more
        than `margin` mm behind the surface that owns its nearest pixel; a vertex outside the window or on background is not occluded), stats [B, 4]
        (covered pixels, observed pixels -- depth_obs finite and > 0 --, pixels that are both, the mean |depth - depth_obs| over those; without depth_obs
        entries 1..3 are 0) and, with depth_obs, iou [B] = both / (covered + observed - both) (NaN when neither has a pixel).  The fitter's own tensors per
        (B, H, W, slot); one launch, no host wait."""
        H, W = int(size[0]), int(size[1])
        if not (H >= 1 and W >= 1 and H * W <= 16384):
            raise ValueError("render_depth takes 1 <= H, W and H * W <= 16384, not %d x %d" % (H, W))
        if not (0.0 <= float(margin) < float("inf")):
            raise ValueError("margin must be finite and >= 0, not %r" % (margin,))
        B = int(verts3d.shape[0])
        self._check(verts3d, (B, 778, 3), "verts3d")
        self._check(cam, (B, 4), "cam")
        if M is not None:
            self._check(M, (B, 2, 3), "M")
        if self.faces is None:
            raise KeyError("no mano_layer.th_faces among the given tensors")
        if depth_obs is not None:
            self._check(depth_obs, (B, H, W), "depth_obs")
        key = (B, H, W, _slot)
        if key not in self._raster_bufs:
            e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
            i = lambda *s: torch.empty(*s, device=self.device, dtype=torch.int32)  # noqa: E731
            self._raster_bufs[key] = {"depth": e(B, H, W), "face": i(B, H, W), "occluded": i(B, 778), "stats": e(B, 4)}
        o = self._raster_bufs[key]
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_raster_f32(verts3d.data_ptr(), self.faces.data_ptr(), int(self.faces.shape[0]), cam.data_ptr(),
                                                 None if M is None else M.data_ptr(), H, W, float(margin),
                                                 None if depth_obs is None else depth_obs.data_ptr(), o["depth"].data_ptr(), o["face"].data_ptr(),
                                                 o["occluded"].data_ptr(), o["stats"].data_ptr(), B, torch.cuda.current_stream().cuda_stream),
                    "kpf_mano_raster_f32")
        out = dict(o)
        if depth_obs is not None:
            st = o["stats"]
            out["iou"] = st[:, 2] / (st[:, 0] + st[:, 1] - st[:, 2])
        return out

    def silhouette(self, depth_obs, _slot=0):
        """The silhouette of an observed depth crop, once per frame (kpf_depth_silhouette_f32).  depth_obs [B, H, W] mm (crop_depth_mm's),
        H * W <= 16384; a pixel is observed iff its depth is finite and > 0, render_depth's rule.

        Returns nearest [B, H, W] int32 (r' * W + c' of the nearest observed pixel, the lowest linear index among equally near ones) and dist2 [B, H, W]
        int32 (its squared distance in pixels; 0 on an observed pixel), both -1 for a hand without an observed pixel; front [B, H, W] (the smallest observed
        depth of the pixel's 3 x 3 neighbourhood, 0 where none is observed) and count [B] int32 (the observed pixels).  The fitter's own tensors per
        (B, H, W, slot); one launch, no host wait."""
        if not (hasattr(depth_obs, "dim") and depth_obs.dim() == 3):
            raise ValueError("depth_obs must be a contiguous float32 [B, H, W] tensor on the device")
        B, H, W = (int(s) for s in depth_obs.shape)
        if not (H >= 1 and W >= 1 and H * W <= 16384):
            raise ValueError("silhouette takes 1 <= H, W and H * W <= 16384, not %d x %d" % (H, W))
        self._check(depth_obs, (B, H, W), "depth_obs")
        key = (B, H, W, _slot)
        if key not in self._sil_bufs:
            i = lambda *s: torch.empty(*s, device=self.device, dtype=torch.int32)  # noqa: E731
            self._sil_bufs[key] = {"nearest": i(B, H, W), "dist2": i(B, H, W), "front": torch.empty(B, H, W, device=self.device, dtype=torch.float32),
                                   "count": i(B)}
        o = self._sil_bufs[key]
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_depth_silhouette_f32(depth_obs.data_ptr(), H, W, o["nearest"].data_ptr(), o["dist2"].data_ptr(), o["front"].data_ptr(),
                                                      o["count"].data_ptr(), B, torch.cuda.current_stream().cuda_stream), "kpf_depth_silhouette_f32")
        return dict(o)

    def free_space(self, verts3d, cam, M, sil, slack2=1, margin=5.0, step=20.0, lambda_free=1.0, vert_target=None, vert_weight=None, vert_normal=None,
                   _slot=0):
        """The free-space term, once per round (kpf_mano_free_space_f32): where the mesh must not be.  verts3d [B, 778, 3], cam [B, 4] and
        M [B, 2, 3] or None as render_depth takes them; sil: silhouette's output for the crop.  A vertex is judged at its nearest pixel (one outside the
        window at the nearest window pixel):
          kind 1, outside the silhouette: dist2 there > slack2 (pixels^2).  Its target is the point of its own depth on the ray through the centre of the
                  nearest observed pixel;
          kind 2, in front of the observed surface: the pixel is observed and z < front - margin (mm; float("inf"): the rule is off).  Its target is the
                  vertex moved along its own ray to depth front - margin;
          kind 0, neither -- also a vertex that is not finite or has z <= 0, and every vertex of a hand with a singular M or without an observed pixel.
        A target farther than `step` mm from its vertex is pulled in to that distance (float("inf"): no clamp).

        vert_target [B, 778, 3] and vert_weight [B, 778] (both or neither) and vert_normal [B, 778, 3] are associate's and normals' outputs: a vertex of
        kind 0 passes them through bit for bit (zeros without them), a vertex of kind 1 or 2 is overridden by its target, the weight lambda_free (one depth
        point weighs 1) and the unit direction of the pull as its normal -- the cloud's matches on it are dropped for the round.

        Returns vert_target, vert_weight, vert_normal (fit_mesh_gn's inputs), kind [B, 778] int32 and stats [B, 4] (the vertices of kind 1, their mean
        distance to the silhouette in pixels, the vertices of kind 2, their mean front - z in mm).  The fitter's own tensors per (B, slot); one launch, no
        host wait."""
        if not (isinstance(slack2, int) and slack2 >= 0):
            raise ValueError("slack2 must be an integer >= 0, not %r" % (slack2,))
        if not float(margin) > 0.0:
            raise ValueError("margin must be > 0 or float(\"inf\"), not %r" % (margin,))
        if not float(step) > 0.0:
            raise ValueError("step must be > 0 or float(\"inf\"), not %r" % (step,))
        if not 0.0 <= float(lambda_free) < float("inf"):
            raise ValueError("lambda_free must be finite and >= 0, not %r" % (lambda_free,))
        if (vert_target is None) != (vert_weight is None):
            raise ValueError("vert_target and vert_weight go together")
        if not (isinstance(sil, dict) and all(k in sil for k in ("nearest", "dist2", "front"))):
            raise ValueError("sil must be silhouette's output")
        B = int(verts3d.shape[0])
        self._check(verts3d, (B, 778, 3), "verts3d")
        self._check(cam, (B, 4), "cam")
        if M is not None:
            self._check(M, (B, 2, 3), "M")
        H, W = (int(s) for s in sil["front"].shape[1:])
        self._check(sil["front"], (B, H, W), "sil[\"front\"]")
        for k in ("nearest", "dist2"):
            t = sil[k]
            if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (B, H, W)):
                raise ValueError("sil[\"%s\"] must be a contiguous int32 %s tensor on the device" % (k, [B, H, W]))
        if vert_target is not None:
            self._check(vert_target, (B, 778, 3), "vert_target")
            self._check(vert_weight, (B, 778), "vert_weight")
        if vert_normal is not None:
            self._check(vert_normal, (B, 778, 3), "vert_normal")
        key = (B, _slot)
        if key not in self._free_bufs:
            e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
            self._free_bufs[key] = {"vert_target": e(B, 778, 3), "vert_weight": e(B, 778), "vert_normal": e(B, 778, 3),
                                    "kind": torch.empty(B, 778, device=self.device, dtype=torch.int32), "stats": e(B, 4)}
        o = self._free_bufs[key]
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_free_space_f32(verts3d.data_ptr(), cam.data_ptr(), ptr(M), H, W, sil["nearest"].data_ptr(), sil["dist2"].data_ptr(),
                                                     sil["front"].data_ptr(), slack2, float(margin), float(step), float(lambda_free), ptr(vert_target),
                                                     ptr(vert_weight), ptr(vert_normal), o["vert_target"].data_ptr(), o["vert_weight"].data_ptr(),
                                                     o["vert_normal"].data_ptr(), o["kind"].data_ptr(), o["stats"].data_ptr(), B,
                                                     torch.cuda.current_stream().cuda_stream), "kpf_mano_free_space_f32")
        return dict(o)

    def associate(self, points_mm, verts3d, point_weight=None, max_dist=20.0, _slot=0, normals=None, facing_min=0.0, vert_mask=None):
        """points_mm [B, N, 3] (camera-space mm, 1 <= N <= 4096), verts3d [B, 778, 3] (a fit's), point_weight [B, N] >= 0 or None (= ones), max_dist: the gate
        in mm (float("inf"): none) -> idx [B, N] int32 (each point's nearest vertex, -1 if its weight is 0, a coordinate is not finite or the vertex is
        farther than max_dist), vert_target [B, 778, 3] and vert_weight [B, 778] (per vertex the weighted centroid and the summed weight of its points; 0
        and 0 without any), stats [B, 2] (matched points, their mean distance in mm).  The fitter's own tensors per (B, N); one launch, no host wait.

        normals [B, 778, 3] (normals' output): only the vertices that face the camera -- the origin of the frame -- are candidates
        (kpf_mano_assoc_vis_f32): n_v . V_v < -facing_min |V_v|, 0 <= facing_min < 1.  Also returned then: visible [B, 778] int32, and stats is [B, 4]: the
        matched points, their mean distance to their vertex, their mean distance to that vertex's tangent plane, the visible vertices.

        vert_mask [B, 778] int32 (needs normals): a vertex whose entry is 0 is no candidate either (kpf_mano_assoc_vis_mask_f32) --
        1 - render_depth's occluded; visible and stats[:, 3] report the combination.  None or all ones: the bits without it."""
        if vert_mask is not None and normals is None:
            raise ValueError("vert_mask needs normals")
        B, N = int(points_mm.shape[0]), int(points_mm.shape[1]) if points_mm.dim() == 3 else -1
        self._check(points_mm, (B, N, 3), "points_mm")
        self._check(verts3d, (B, 778, 3), "verts3d")
        if point_weight is not None:
            self._check(point_weight, (B, N), "point_weight")
        if not 1 <= N <= 4096:
            raise ValueError("associate takes 1 <= N <= 4096 points per hand, not %d" % N)
        if normals is not None:
            return self._associate_vis(points_mm, verts3d, point_weight, max_dist, _slot, normals, facing_min, B, N, vert_mask)
        key = (B, N, _slot)
        if key not in self._assoc_bufs:
            e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
            self._assoc_bufs[key] = {"idx": torch.empty(B, N, device=self.device, dtype=torch.int32), "vert_target": e(B, 778, 3), "vert_weight": e(B, 778),
                                     "stats": e(B, 2)}
        o = self._assoc_bufs[key]
        with torch.cuda.device(self.device):
            L.check(L.load().kpf_mano_assoc_f32(points_mm.data_ptr(), None if point_weight is None else point_weight.data_ptr(), verts3d.data_ptr(),
                                                float(max_dist) * float(max_dist), o["idx"].data_ptr(), o["vert_target"].data_ptr(),
                                                o["vert_weight"].data_ptr(), o["stats"].data_ptr(), B, N, torch.cuda.current_stream().cuda_stream),
                    "kpf_mano_assoc_f32")
        return dict(o)

    def _associate_vis(self, points_mm, verts3d, point_weight, max_dist, _slot, normals, facing_min, B, N, vert_mask=None):
        self._check(normals, (B, 778, 3), "normals")
        if vert_mask is not None and not (vert_mask.is_cuda and vert_mask.dtype == torch.int32 and vert_mask.is_contiguous()
                                          and tuple(vert_mask.shape) == (B, 778)):
            raise ValueError("vert_mask must be a contiguous int32 [%d, 778] tensor on the device" % B)
        if not 0.0 <= float(facing_min) < 1.0:
            raise ValueError("facing_min must be in [0, 1), not %r" % (facing_min,))
        key = (B, N, _slot, "vis")
        if key not in self._assoc_bufs:
            e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)  # noqa: E731
            self._assoc_bufs[key] = {"idx": torch.empty(B, N, device=self.device, dtype=torch.int32), "vert_target": e(B, 778, 3), "vert_weight": e(B, 778),
                                     "visible": torch.empty(B, 778, device=self.device, dtype=torch.int32), "stats": e(B, 4)}
        o = self._assoc_bufs[key]
        name = "kpf_mano_assoc_vis_f32" if vert_mask is None else "kpf_mano_assoc_vis_mask_f32"
        extra = [] if vert_mask is None else [vert_mask.data_ptr()]
        with torch.cuda.device(self.device):
            L.check(getattr(L.load(), name)(points_mm.data_ptr(), None if point_weight is None else point_weight.data_ptr(), verts3d.data_ptr(),
                                            normals.data_ptr(), *extra, float(max_dist) * float(max_dist), float(facing_min), o["idx"].data_ptr(),
                                            o["vert_target"].data_ptr(), o["vert_weight"].data_ptr(), o["visible"].data_ptr(), o["stats"].data_ptr(), B, N,
                                            torch.cuda.current_stream().cuda_stream), name)
        return dict(o)

    def fit_cloud(self, joints_mm, points_mm, weight=None, point_weight=None, state=None, init_trans=True, rounds=3, iters_cloud=None, max_dist=20.0,
                  lambda_verts=1.0, joint_solver="adam", cloud_solver="adam", metric="point", facing_min=0.0, normal_sign=1.0, occlusion=None, camera=None,
                  raster_size=(128, 128), occlusion_margin=10.0, depth_obs=None, free_space=None, free_slack2=1, free_margin=5.0, free_step=20.0,
                  lambda_free=1.0):
        """Joints, then the depth points: one fit on the joints, then `rounds` times associate followed by fit_mesh (warm start, init_trans=False, the joints
        kept in the objective, iters_cloud iterations each; None = the fitter's), and last one associate on the final vertices: 2 * rounds + 2 launches and no
        host wait.  Returns the last fit's outputs plus cloud_before and cloud_after (the stats of the first and the last association: matched points and
        their mean distance to the mesh in mm) and the last association's idx, vert_target and vert_weight.  rounds=0 is fit plus one associate.
        joint_solver: "adam" (fit) or "gn" (fit_gn with its defaults) for the first stage.  cloud_solver: "adam" (fit_mesh) or "gn" (fit_mesh_gn; iters_cloud=None
        is then 2 -- the alternation limits the chain, not the solver, so the rounds should be many and short: rounds=6) for the vertex rounds.  The two are
        independent; on the synthetic hand the Adam joint stage is the better start for the cloud.

        metric: "point" (the above, its bits) or "plane" (needs cloud_solver="gn"): each round is normals -> associate(normals=, facing_min)
        -> fit_mesh_gn(vert_normal=), and a last normals + associate: 3 * rounds + 3 launches, no host wait.  Also returned then: normals and visible of the
        final mesh, and cloud_before / cloud_after are the 4-wide stats.  normal_sign: normals' sign.

        occlusion: None (the above, its bits) or "zbuffer" (needs metric="plane" and camera=(cam, M) as crop_camera gives them): each round
        is normals -> render_depth(raster_size, occlusion_margin) -> associate(normals=, vert_mask=1 - occluded) -> fit_mesh_gn(vert_normal=), and a last
        normals + render_depth(depth_obs=) + associate: 4 * rounds + 4 launches and the mask's elementwise op, no host wait.  Also returned then: depth,
        face, occluded and depth_stats of the final mesh's render (render_depth's stats) and, with depth_obs [B, H, W] (crop_depth_mm's), iou.

        free_space: None (the above, its bits and launches) or "silhouette" (needs cloud_solver="gn", camera=(cam, M) and depth_obs; either
        metric, with or without occlusion="zbuffer"): one silhouette(depth_obs) per call, and in each round free_space(free_slack2, free_margin, free_step,
        lambda_free) between associate and fit_mesh_gn -- a vertex outside the observed silhouette, or more than free_margin mm in front of the observed
        surface, gets its free-space target in place of the cloud's (metric="point" takes the target and the weight, "plane" the merged normal too) -- and
        a last free_space on the final vertices for the report: rounds + 2 launches more.  Also returned then: free_before and free_after (free_space's
        stats of the first and the last call), free_kind (the last call's kind) and silhouette (silhouette's output).  Off by default: with few joints
        weighted and a far start the term can make the vertex error worse; free_margin=float("inf") switches the in-front rule off."""
        if free_space not in (None, "silhouette"):
            raise ValueError("free_space must be None or \"silhouette\", not %r" % (free_space,))
        if free_space is not None and cloud_solver != "gn":
            raise ValueError("free_space=\"silhouette\" needs cloud_solver=\"gn\"")
        if free_space is not None and (camera is None or len(camera) != 2):
            raise ValueError("free_space=\"silhouette\" needs camera=(cam, M)")
        if free_space is not None and depth_obs is None:
            raise ValueError("free_space=\"silhouette\" needs depth_obs")
        if occlusion not in (None, "zbuffer"):
            raise ValueError("occlusion must be None or \"zbuffer\", not %r" % (occlusion,))
        if occlusion == "zbuffer" and metric != "plane":
            raise ValueError("occlusion=\"zbuffer\" needs metric=\"plane\"")
        if occlusion == "zbuffer" and (camera is None or len(camera) != 2):
            raise ValueError("occlusion=\"zbuffer\" needs camera=(cam, M)")
        if metric not in ("point", "plane"):
            raise ValueError("metric must be \"point\" or \"plane\", not %r" % (metric,))
        if metric == "plane" and cloud_solver != "gn":
            raise ValueError("metric=\"plane\" needs cloud_solver=\"gn\"")
        if joint_solver not in ("adam", "gn"):
            raise ValueError("joint_solver must be \"adam\" or \"gn\", not %r" % (joint_solver,))
        if cloud_solver not in ("adam", "gn"):
            raise ValueError("cloud_solver must be \"adam\" or \"gn\", not %r" % (cloud_solver,))
        if joint_solver == "gn":
            out = self.fit_gn(joints_mm, weight, state=state, init_trans=init_trans)
        else:
            out = self.fit(joints_mm, weight, state=state, init_trans=init_trans)
        state = (out["mano_pose_aa"], out["mano_shape"], out["trans"])
        first = None
        sil, free_first = None, None
        if free_space is not None:
            sil = self.silhouette(depth_obs)

        def free(verts, slot, a=None, nrm=None):  # free_space on `verts`, over the association `a` (and the normals); the report's call has neither
            return self.free_space(verts, camera[0], camera[1], sil, free_slack2, free_margin, free_step, lambda_free,
                                   None if a is None else a["vert_target"], None if a is None else a["vert_weight"], nrm, _slot=slot)

        def free_report(out, verts):  # the last call, on the final vertices
            if sil is not None:
                rep = free(verts, 2)
                out.update(free_before=(rep if free_first is None else free_first)["stats"], free_after=rep["stats"], free_kind=rep["kind"], silhouette=sil)
        if metric == "plane":
            zbuf = occlusion == "zbuffer"

            def mask_of(verts, slot, obs=None):  # (the render, 1 - occluded) of the z-buffer, or (None, None)
                if not zbuf:
                    return None, None
                ren = self.render_depth(verts, camera[0], camera[1], raster_size, occlusion_margin, depth_obs=obs, _slot=slot)
                return ren, 1 - ren["occluded"]

            for r in range(int(rounds)):
                nrm = self.normals(out["verts3d"], normal_sign)
                _, mask = mask_of(out["verts3d"], 0)
                a = self.associate(points_mm, out["verts3d"], point_weight, max_dist, _slot=1 if r == 0 else 0, normals=nrm, facing_min=facing_min,
                                   vert_mask=mask)
                first = a if first is None else first
                tgt, pull = a, nrm
                if sil is not None:
                    tgt = free(out["verts3d"], 1 if r == 0 else 0, a, nrm)
                    free_first, pull = tgt if free_first is None else free_first, tgt["vert_normal"]
                out = self.fit_mesh_gn(joints_mm, weight, tgt["vert_target"], tgt["vert_weight"], state=state, init_trans=False, lambda_verts=lambda_verts,
                                       iters=2 if iters_cloud is None else iters_cloud, vert_normal=pull)
            nrm = self.normals(out["verts3d"], normal_sign, _slot=2)
            ren, mask = mask_of(out["verts3d"], 2, depth_obs)
            last = self.associate(points_mm, out["verts3d"], point_weight, max_dist, _slot=2, normals=nrm, facing_min=facing_min, vert_mask=mask)
            out = dict(out)
            out.update(cloud_before=(last if first is None else first)["stats"], cloud_after=last["stats"], idx=last["idx"], vert_target=last["vert_target"],
                       vert_weight=last["vert_weight"], normals=nrm, visible=last["visible"])
            if zbuf:
                out.update(depth=ren["depth"], face=ren["face"], occluded=ren["occluded"], depth_stats=ren["stats"])
                if depth_obs is not None:
                    out["iou"] = ren["iou"]
            free_report(out, out["verts3d"])
            return out
        for r in range(int(rounds)):
            a = self.associate(points_mm, out["verts3d"], point_weight, max_dist, _slot=1 if r == 0 else 0)
            first = a if first is None else first
            if sil is not None:
                a = free(out["verts3d"], 1 if r == 0 else 0, a)
                free_first = a if free_first is None else free_first
            if cloud_solver == "gn":
                out = self.fit_mesh_gn(joints_mm, weight, a["vert_target"], a["vert_weight"], state=state, init_trans=False, lambda_verts=lambda_verts,
                                       iters=2 if iters_cloud is None else iters_cloud)
            else:
                out = self.fit_mesh(joints_mm, weight, a["vert_target"], a["vert_weight"], state=state, init_trans=False, lambda_verts=lambda_verts,
                                    iters=iters_cloud)
        last = self.associate(points_mm, out["verts3d"], point_weight, max_dist, _slot=2)
        out = dict(out)
        out.update(cloud_before=(last if first is None else first)["stats"], cloud_after=last["stats"], idx=last["idx"], vert_target=last["vert_target"],
                   vert_weight=last["vert_weight"])
        free_report(out, out["verts3d"])
        return out


def cloud_mm(prep):
    """The depth points the preprocessing sampled for the model, back in camera-space mm: (points [B, n, 3], point_weight [B, n]) as device tensors, the
    inputs of ManoFitter.associate / fit_cloud.  points = prep["pcl"] * prep["cube"][:, None] / 2 + prep["center"][:, None]; the weight is 1, and 0 for every
    point of a hand whose prep["pcl_count"] is 0 (its cloud is all zeros, which would sit at the crop's centre).

    The frame: preprocess.depth_to_pcl back-projects a crop pixel as x = (u - u0) / fx * d, y = +(v - v0) / fy * d (flip = 1), z = d and normalises it by
    (xyz - center) / (cube / 2), center being image_to_3d of the centre of mass with the same sign; kpf_prep_pcl_sample restates exactly that.  The tracker's
    cam_mm (kpf_track.hip) is joints * cube / 2 + center of the model's cube-normalised joints, which the same kernel projects with u = x fx / z + u0,
    v = y fy / z + v0.  So both are the one camera frame, y growing with the image row, no sign change between them, and this cloud can be compared with
    cam_mm and with a fit to it as it stands.  Two things to know: the sampler clips a point to the cube ([-1, 1] per axis), so a point outside it lies on
    a face of the cube and not on the surface -- the gate of associate (max_dist) is what keeps such points from pulling the mesh; and a cloud smaller than n
    repeats its points."""
    pts = prep["pcl"] * prep["cube"][:, None] / 2 + prep["center"][:, None]
    w = (prep["pcl_count"] > 0).to(pts.dtype)[:, None].expand(pts.shape[0], pts.shape[1]).contiguous()
    return pts.contiguous(), w


def crop_camera(prep):
    """The camera and the crop map of the preprocessing's outputs, as ManoFitter.render_depth and fit_cloud(camera=) take them: (cam [B, 4] float32 = fx,
    fy, u0, v0 from prep["cam_para"], M [B, 2, 3] float32 = the top two rows of prep["M"]), device tensors.

    The frame and the pixel convention: prep["M"] maps FRAME pixels (u, v, 1) to CROP coordinates (its last row is 0 0 1 -- the crop is affine), and
    preprocess.depth_to_pcl back-projects crop pixel (column c, row r) from the crop coordinates (c + 0.5, r + 0.5) through inv(M) and then
    x = (u - u0) / fx * d, y = (v - v0) / fy * d, z = d: cloud_mm's frame.  render_depth projects with u = x fx / z + u0, v = y fy / z + v0, applies M and
    samples pixel (c, r) at those same crop coordinates (c + 0.5, r + 0.5), so a rendered depth, back-projected the preprocessing's way, lies on the mesh,
    and a render can be compared pixel by pixel with crop_depth_mm."""
    return prep["cam_para"].to(torch.float32).contiguous(), prep["M"][:, :2, :].to(torch.float32).contiguous()


def crop_depth_mm(prep):
    """The observed depth crop in mm, [B, H, W] float32 on the device: what render_depth(depth_obs=) and fit_cloud(depth_obs=) compare a render with.
    preprocess.depth_to_pcl's rule: prep["img"] [B, 1, H, W] * prep["cube"][:, 2] / 2 + prep["center"][:, 2], and 0 (background: not observed) where img is
    close to 1 by that function's test, numpy.isclose(img, 1).  Pixel (row r, column c) of the result is the crop's pixel (c, r), z along the camera axis:
    the convention of crop_camera."""
    img = prep["img"][:, 0].to(torch.float32)
    d = img * (prep["cube"][:, 2].to(torch.float32) / 2)[:, None, None] + prep["center"][:, 2].to(torch.float32)[:, None, None]
    return torch.where(torch.isclose(img, torch.ones_like(img)), torch.zeros_like(d), d).contiguous()
