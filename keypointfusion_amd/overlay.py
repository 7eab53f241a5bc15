"""The result drawn over the frame on the device: shaded mesh and skeleton (csrc/kpf_overlay.hip).

FrameOverlay.draw takes the stored camera frames, the fitted meshes (ManoFitter.fit*'s verts3d, normals) and the joints in pixels (TrackedStream.step's
frame_px) and returns the picture, a per-pixel label, the owning hand and primitive, and the full-frame model depth -- two launches on the current
stream, no host wait, no allocation after the first call of a batch size, so that it can be captured in a torch.cuda.graph.  All hands of one camera
frame share one z-buffer: the nearest surface wins a pixel whichever hand it belongs to, and an observed depth frame hides the mesh behind the scene.

The drawing rule is this project's own, stated exactly (include/kpf.h) and restated here in numpy float32 by draw_host, which gives the kernels' bits: the
reference's demo draws with OpenCV's line and circle, whose pixels are not reproduced.  The reference's painter's order is kept: a hand's joints as filled
circles, then its bones over them, one colour per finger.

Pixel convention.  Grid pixel (c, r) is sampled at sx = c, sy = r, with sx = (M (u, v, 1)).x - sample_offset.  A crop grid reached through M takes
sample_offset = 0.5 (render_depth's convention: the preprocessing back-projects crop pixel (c, r) from (c + 0.5, r + 0.5)).  The frame itself (M None)
takes 0: the un-crop of a joint (kpf_uncrop_joint, TrackedStream's frame_px) is u = x fx / z + u0 with no half-pixel shift, and the skeleton takes pixel
(c, r) as the point (c, r) of those coordinates, so only with 0 do a model joint projected by cam and the same joint in frame_px land on the same pixel."""
import numpy as np
import torch

from . import lib as L

NV = 778
LABEL_NONE, LABEL_MESH, LABEL_BONE, LABEL_JOINT, LABEL_HIDDEN = 0, 1, 2, 3, 4

# The skeleton over the model's 21 joints in the head's order (joints3d: the wrist, three joints per finger in the order index, middle, little, ring,
# thumb, then the tips of index, middle, little, ring, thumb): five chains from the wrist.  Another dataset's order is the caller's business, as joint_map.
MANO21_CHAINS = {"thumb": (0, 13, 14, 15, 20), "index": (0, 1, 2, 3, 16), "middle": (0, 4, 5, 6, 17), "ring": (0, 10, 11, 12, 19), "little": (0, 7, 8, 9, 18)}
MANO21_BONES = tuple((c[i], c[i + 1]) for c in MANO21_CHAINS.values() for i in range(4))
FINGER_COLOR = {"thumb": (230, 60, 60), "index": (240, 170, 40), "middle": (70, 200, 70), "ring": (60, 150, 240), "little": (180, 90, 220)}
WRIST_COLOR = (240, 240, 240)
MANO21_BONE_COLOR = tuple(FINGER_COLOR[n] for n in MANO21_CHAINS for _ in range(4))
MANO21_JOINT_COLOR = tuple(next((FINGER_COLOR[n] for n, c in MANO21_CHAINS.items() if j in c[1:]), WRIST_COLOR) for j in range(21))
MESH_COLOR = (205.0, 175.0, 150.0)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the rule, in numpy: every product, sum, difference and quotient below is ONE float32 operation
# ----------------------------------------------------------------------------------------------------------------------------------------
def project_host(verts, normals, cam, M, sample_offset, ambient, H, W):
    """kpf_overlay_project_f32 in numpy float32: verts [B, 778, 3], normals the same or None, cam [B, 4], M [B, 2, 3] or None ->
    dict(sx, sy, iz, shade [B, 778] float32, ok [B, 778] int32, rect [B, 4] int32)"""
    f = np.float32
    V, c = np.ascontiguousarray(verts, f), np.ascontiguousarray(cam, f)
    B = V.shape[0]
    m = np.tile(np.asarray([[1, 0, 0], [0, 1, 0]], f), (B, 1, 1)) if M is None else np.ascontiguousarray(M, f)
    off, amb = f(sample_offset), f(ambient)
    with np.errstate(all="ignore"):
        x, y, z = V[..., 0], V[..., 1], V[..., 2]
        U, Vv = (x * c[:, None, 0]) / z + c[:, None, 2], (y * c[:, None, 1]) / z + c[:, None, 3]
        sx = ((m[:, None, 0, 0] * U + m[:, None, 0, 1] * Vv) + m[:, None, 0, 2]) - off
        sy = ((m[:, None, 1, 0] * U + m[:, None, 1, 1] * Vv) + m[:, None, 1, 2]) - off
        iz = f(1) / z
        ok = np.isfinite(V).all(-1) & (z > 0)
        if normals is None:
            shade = np.ones((B, NV), f)
        else:
            n = np.ascontiguousarray(normals, f)
            some = np.isfinite(n).all(-1) & ~(n == 0).all(-1)
            shade = np.where(some, amb + (f(1) - amb) * np.abs(n[..., 2]), amb).astype(f)
        rect = np.zeros((B, 4), np.int32)
        inf = f(np.inf)
        for b in range(B):
            lox, loy = np.fmin.reduce(sx[b][ok[b]], initial=inf), np.fmin.reduce(sy[b][ok[b]], initial=inf)
            hix, hiy = np.fmax.reduce(sx[b][ok[b]], initial=-inf), np.fmax.reduce(sy[b][ok[b]], initial=-inf)
            rect[b] = (int(min(max(np.ceil(lox), f(0)), f(W))), int(min(max(np.ceil(loy), f(0)), f(H))),
                       int(max(min(np.floor(hix), f(W - 1)), f(-1))), int(max(min(np.floor(hiy), f(H - 1)), f(-1))))
    return dict(sx=sx.astype(f), sy=sy.astype(f), iz=iz.astype(f), shade=shade, ok=ok.astype(np.int32), rect=rect)


def _edge(sx, sy, a, b, px, py):
    """kpf_mano_raster_f32's edge function of the directed edge a -> b at (px, py): evaluated from the lower vertex index, negated if a > b"""
    lo, hi = (a, b) if a < b else (b, a)
    e = (sx[hi] - sx[lo]) * (py - sy[lo]) - (sy[hi] - sy[lo]) * (px - sx[lo])
    return -e if a > b else e


def _mesh_host(p, b, faces, H, W, best, owner, prim, shade):
    """hand b's faces in ascending order into one frame's buffers: a candidate replaces the pixel's only if it is strictly nearer, and the hands arrive in
    ascending order, which is the smallest (d, hand, face)"""
    f = np.float32
    sx, sy, iz, ok, sh = p["sx"][b], p["sy"][b], p["iz"][b], p["ok"][b], p["shade"][b]
    for k, (i0, i1, i2) in enumerate(faces):
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= NV or i0 == i1 or i1 == i2 or i0 == i2 or not (ok[i0] and ok[i1] and ok[i2]):
            continue
        area = _edge(sx, sy, i0, i1, sx[i2], sy[i2])
        if area == 0 or not np.isfinite(area):
            continue
        xs, ys = sx[[i0, i1, i2]], sy[[i0, i1, i2]]
        x0, x1 = max(np.ceil(xs.min()), 0.0), min(np.floor(xs.max()), float(W - 1))  # clamped as floats, then converted
        y0, y1 = max(np.ceil(ys.min()), 0.0), min(np.floor(ys.max()), float(H - 1))
        if not (x0 <= x1 and y0 <= y1):
            continue
        x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
        py, px = np.meshgrid(np.arange(y0, y1 + 1).astype(f), np.arange(x0, x1 + 1).astype(f), indexing="ij")
        w0, w1, w2 = _edge(sx, sy, i1, i2, px, py), _edge(sx, sy, i2, i0, px, py), _edge(sx, sy, i0, i1, px, py)
        inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) if area > 0 else ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        tot = (w0 + w1) + w2
        q0, q1, q2 = w0 / tot, w1 / tot, w2 / tot
        d = f(1) / ((q0 * iz[i0] + q1 * iz[i1]) + q2 * iz[i2])
        s = (q0 * sh[i0] + q1 * sh[i1]) + q2 * sh[i2]
        win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        upd = inside & np.isfinite(d) & (d > 0) & (d < best[win])
        best[win] = np.where(upd, d, best[win])
        owner[win] = np.where(upd, np.int32(b), owner[win])
        prim[win] = np.where(upd, np.int32(k), prim[win])
        shade[win] = np.where(upd, s, shade[win])


def _byte_host(v):
    """floor(v + 0.5) clamped to 0..255, NaN -> 0"""
    return np.fmin(np.fmax(np.floor(v + np.float32(0.5)), np.float32(0)), np.float32(255)).astype(np.uint8)


def _skeleton_host(jp, bones, R, hw, H, W):
    """one hand's covering primitives in the painter's order, joints then bones -> [(is_bone, index, covered [H, W] bool), ...]"""
    f = np.float32
    py, px = np.meshgrid(np.arange(H).astype(f), np.arange(W).astype(f), indexing="ij")
    one, R2, hw2 = f(1), R * R, hw * hw
    out = []
    for j in range(jp.shape[0]):
        u, v = jp[j, 0], jp[j, 1]
        if not (np.isfinite(u) and np.isfinite(v)):
            continue
        box = (px >= (u - R) - one) & (px <= (u + R) + one) & (py >= (v - R) - one) & (py <= (v + R) + one)
        dx, dy = px - u, py - v
        out.append((False, j, box & ((dx * dx + dy * dy) <= R2)))
    for i, (ia, ib) in enumerate(bones):
        ax, ay, bx, by = jp[ia, 0], jp[ia, 1], jp[ib, 0], jp[ib, 1]
        if not np.isfinite([ax, ay, bx, by]).all():
            continue
        box = ((px >= (min(ax, bx) - hw) - one) & (px <= (max(ax, bx) + hw) + one) & (py >= (min(ay, by) - hw) - one) & (py <= (max(ay, by) + hw) + one))
        ex, ey = bx - ax, by - ay
        Lq = ex * ex + ey * ey
        qx, qy = px - ax, py - ay
        t = np.fmin(np.fmax((qx * ex + qy * ey) / Lq, f(0)), f(1)) if Lq > 0 else np.zeros_like(px)
        rx, ry = qx - t * ex, qy - t * ey
        out.append((True, i, box & ((rx * rx + ry * ry) <= hw2)))
    return out


def draw_host(rgb, faces=None, verts3d=None, cam=None, normals=None, joints_px=None, status=None, depth_frame=None, M=None, frame_index=None,
              sample_offset=None, bones=MANO21_BONES, bone_color=MANO21_BONE_COLOR, joint_color=MANO21_JOINT_COLOR, mesh_color=MESH_COLOR, alpha=0.6,
              ambient=0.3, joint_radius=2.0, bone_half_width=0.75, occl_margin=10.0, mesh_on=None, skel_on=None):
    """Both launches in numpy float32, the yardstick and the documentation of the rule: FrameOverlay's arguments as arrays -> dict(image [F, H, W, 3]
    uint8, label [F, H, W] uint8, owner, prim [F, H, W] int32, depth [F, H, W] float32, project = project_host's dict or None).  rgb [F, H, W, 3] uint8;
    faces [Fc, 3]; frame_index [B] or None (then F == B); status [B] (a hand is drawn iff status == 0) or mesh_on / skel_on [B] separately."""
    f = np.float32
    rgb = np.ascontiguousarray(rgb, np.uint8)
    F, H, W = rgb.shape[:3]
    B = int((verts3d if verts3d is not None else joints_px).shape[0])
    fi = np.arange(B) if frame_index is None else np.clip(np.asarray(frame_index, np.int64), 0, F - 1)
    if status is not None:
        mesh_on = skel_on = (np.asarray(status) == 0)
    on_m = np.ones(B, bool) if mesh_on is None else np.asarray(mesh_on) != 0
    on_s = np.ones(B, bool) if skel_on is None else np.asarray(skel_on) != 0
    off = f((0.5 if M is not None else 0.0) if sample_offset is None else sample_offset)
    alpha, amb, margin, R, hw = f(alpha), f(ambient), f(occl_margin), f(joint_radius), f(bone_half_width)
    mc = np.broadcast_to(np.asarray(mesh_color, f), (B, 3))
    image, label = rgb.copy(), np.zeros((F, H, W), np.uint8)
    owner, prim = np.full((F, H, W), -1, np.int32), np.full((F, H, W), -1, np.int32)
    depth = np.zeros((F, H, W), f)
    p = None
    with np.errstate(all="ignore"):
        if verts3d is not None:
            p = project_host(verts3d, normals, cam, M, off, amb, H, W)
            fc = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
            keep = f(1) - alpha
            for fr in range(F):
                best, shade = np.full((H, W), np.inf, f), np.zeros((H, W), f)
                for b in range(B):
                    r = p["rect"][b]
                    if fi[b] == fr and on_m[b] and r[2] >= r[0] and r[3] >= r[1]:
                        _mesh_host(p, b, fc, H, W, best, owner[fr], prim[fr], shade)
                cov = owner[fr] >= 0
                depth[fr] = np.where(cov, best, f(0))
                hidden = np.zeros((H, W), bool)
                if depth_frame is not None:
                    o = np.asarray(depth_frame)[fr]
                    hidden = cov & (o != 0) & (o.astype(f) < best - margin)
                label[fr] = np.where(hidden, LABEL_HIDDEN, np.where(cov, LABEL_MESH, LABEL_NONE))
                draw = cov & ~hidden
                col = mc[np.where(cov, owner[fr], 0)]  # [H, W, 3]
                mixed = _byte_host(keep * rgb[fr].astype(f) + alpha * (col * shade[..., None]))
                image[fr] = np.where(draw[..., None], mixed, rgb[fr])
        if joints_px is not None:
            jp = np.ascontiguousarray(joints_px, f)
            bn = [(int(a), int(b)) for a, b in np.asarray(bones, np.int64).reshape(-1, 2)]
            bcol, jcol = np.asarray(bone_color, np.uint8).reshape(-1, 3), np.asarray(joint_color, np.uint8).reshape(-1, 3)
            for b in range(B):
                if not on_s[b]:
                    continue
                fr = fi[b]
                for is_bone, idx, covered in _skeleton_host(jp[b], bn, R, hw, H, W):
                    image[fr][covered] = (bcol if is_bone else jcol)[idx]
                    label[fr][covered] = LABEL_BONE if is_bone else LABEL_JOINT
                    owner[fr][covered] = b
                    prim[fr][covered] = idx
    return dict(image=image, label=label, owner=owner, prim=prim, depth=depth, project=p)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------------------------------------------------------------------
def depth_crop_u8(prep):
    """The demo's grey picture of the depth crop, [B, H, W, 3] uint8 on the device: (prep["img"] + 1) / 2 * 255 truncated, on three channels -- the frame
    FrameOverlay.draw(M=...) draws the crop form over."""
    g = ((prep["img"][:, 0].to(torch.float32) + 1.0) / 2.0 * 255.0).clamp(0.0, 255.0).to(torch.uint8)
    return g[..., None].expand(-1, -1, -1, 3).contiguous()


class FrameOverlay:
    """FrameOverlay(fitter_or_faces, device, frame_size, frames).draw(rgb, ...) -> the picture and its by-products, on the device.

    fitter_or_faces: a ManoFitter (its faces), the faces [Fc, 3] themselves, or None (a skeleton-only overlay).  frame_size = (H, W) of the target grid,
    frames = F stored frames; frame_index [B] ints (hand b belongs to stored frame frame_index[b]; None: F == B and hand b lies on frame b).  bones
    [NB, 2], bone_color [NB, 3], joint_color [J, 3] (0..255) are the skeleton's tables; mesh_color is one colour or [B, 3]."""

    def __init__(self, fitter_or_faces, device, frame_size, frames, frame_index=None, bones=MANO21_BONES, bone_color=MANO21_BONE_COLOR,
                 joint_color=MANO21_JOINT_COLOR, mesh_color=MESH_COLOR, alpha=0.6, ambient=0.3, joint_radius=2.0, bone_half_width=0.75, occl_margin=10.0):
        self.device = torch.device(device)
        faces = getattr(fitter_or_faces, "faces", fitter_or_faces)
        self.faces = None if faces is None else torch.as_tensor(np.asarray(faces.cpu() if torch.is_tensor(faces) else faces)).to(torch.int32).to(self.device).contiguous()
        if self.faces is not None and (self.faces.dim() != 2 or self.faces.shape[1] != 3 or not 1 <= self.faces.shape[0] <= 2048):
            raise ValueError("faces must be [Fc, 3] with 1 <= Fc <= 2048")
        self.H, self.W, self.F = int(frame_size[0]), int(frame_size[1]), int(frames)
        if self.H < 1 or self.W < 1 or self.F < 1:
            raise ValueError("frame_size and frames must be positive")
        self.frame_index = None if frame_index is None else torch.as_tensor(frame_index).to(torch.int32).to(self.device).contiguous()
        self._bones = np.ascontiguousarray(np.asarray(bones, np.int32).reshape(-1, 2))  # host tables: read by the entry before each launch
        self._bone_color = np.ascontiguousarray(np.asarray(bone_color, np.uint8).reshape(-1, 3))
        self._joint_color = np.ascontiguousarray(np.asarray(joint_color, np.uint8).reshape(-1, 3))
        if len(self._bone_color) != len(self._bones):
            raise ValueError("bone_color must hold one colour per bone")
        self.mesh_color = np.asarray(mesh_color, np.float32)
        self.alpha, self.ambient, self.joint_radius = float(alpha), float(ambient), float(joint_radius)
        self.bone_half_width, self.occl_margin = float(bone_half_width), float(occl_margin)
        e = lambda dt, *s: torch.empty(*s, device=self.device, dtype=dt)  # noqa: E731
        self._out = {"image": e(torch.uint8, self.F, self.H, self.W, 3), "label": e(torch.uint8, self.F, self.H, self.W),
                     "owner": e(torch.int32, self.F, self.H, self.W), "prim": e(torch.int32, self.F, self.H, self.W),
                     "depth": e(torch.float32, self.F, self.H, self.W)}
        self._bufs = {}

    def _buffers(self, B):
        """static per batch size: a captured graph keeps reading and writing where it was captured"""
        if B not in self._bufs:
            e = lambda dt, *s: torch.empty(*s, device=self.device, dtype=dt)  # noqa: E731
            mc = torch.tensor(np.broadcast_to(self.mesh_color, (B, 3)).tolist(), dtype=torch.float32, device=self.device)
            self._bufs[B] = {"sx": e(torch.float32, B, NV), "sy": e(torch.float32, B, NV), "iz": e(torch.float32, B, NV), "shade": e(torch.float32, B, NV),
                             "ok": e(torch.int32, B, NV), "rect": e(torch.int32, B, 4), "on": e(torch.bool, B), "mesh_color": mc}
        return self._bufs[B]

    def _check(self, t, shape, dtype, name):
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), self.device))

    def draw(self, rgb, verts3d=None, cam=None, normals=None, joints_px=None, status=None, depth_frame=None, M=None, sample_offset=None):
        """rgb [F, H, W, 3] uint8; verts3d [B, 778, 3] mm in the camera frame with cam [B, 4] = fx, fy, u0, v0 (None: only the skeleton), normals
        [B, 778, 3] (ManoFitter.normals; None: unshaded); joints_px [B, J, 3] = u, v, d in target-grid pixels (None: only the mesh); status [B] int32
        (a hand is drawn iff its status is 0: a lost track draws nothing); depth_frame [F, H, W] uint16 mm (int16 storage is taken by its bits), 0 = not
        observed: the mesh more than occl_margin behind it is hidden; M [B, 2, 3]: frame pixels -> target-grid coordinates, the crop form (F == B,
        frame_index None, rgb = the crops, e.g. depth_crop_u8(prep)).  sample_offset: None = 0.5 with M, 0 without (see the module's text).

        Returns the overlay's own tensors, overwritten by the next call: image [F, H, W, 3] uint8, label [F, H, W] uint8 (0 nothing, 1 mesh, 2 bone,
        3 joint, 4 mesh hidden by the scene), owner (the hand, -1 none) and prim (the face, bone or joint index) [F, H, W] int32, depth [F, H, W] float32
        (the model depth in mm, 0 where no mesh)."""
        if verts3d is None and joints_px is None:
            raise ValueError("draw needs verts3d, joints_px or both")
        B = int((verts3d if verts3d is not None else joints_px).shape[0])
        self._check(rgb, (self.F, self.H, self.W, 3), torch.uint8, "rgb")
        o = self._buffers(B)
        d = L.OverlayDrawDesc()
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if status is not None:
                self._check(status, (B,), torch.int32, "status")
                torch.eq(status, 0, out=o["on"])
                d.mesh_on = d.skel_on = o["on"].data_ptr()
            if verts3d is not None:
                if self.faces is None:
                    raise ValueError("this overlay was built without faces")
                self._check(verts3d, (B, NV, 3), torch.float32, "verts3d")
                self._check(cam, (B, 4), torch.float32, "cam")
                if normals is not None:
                    self._check(normals, (B, NV, 3), torch.float32, "normals")
                if M is not None:
                    self._check(M, (B, 2, 3), torch.float32, "M")
                off = (0.5 if M is not None else 0.0) if sample_offset is None else float(sample_offset)
                L.check(L.load().kpf_overlay_project_f32(verts3d.data_ptr(), ptr(normals), cam.data_ptr(), ptr(M), off, self.ambient, self.H, self.W,
                                                         o["sx"].data_ptr(), o["sy"].data_ptr(), o["iz"].data_ptr(), o["shade"].data_ptr(),
                                                         o["ok"].data_ptr(), o["rect"].data_ptr(), B, stream), "kpf_overlay_project_f32")
                for k in ("sx", "sy", "iz", "shade", "ok", "rect", "mesh_color"):
                    setattr(d, k, o[k].data_ptr())
                d.faces, d.Fc = self.faces.data_ptr(), int(self.faces.shape[0])
            if joints_px is not None:
                J = int(joints_px.shape[1])
                self._check(joints_px, (B, J, 3), torch.float32, "joints_px")
                if len(self._joint_color) != J:
                    raise ValueError("joint_color holds %d colours, joints_px %d joints" % (len(self._joint_color), J))
                d.joints_px, d.J, d.NB = joints_px.data_ptr(), J, len(self._bones)
                d.bones, d.bone_color, d.joint_color = self._bones.ctypes.data, self._bone_color.ctypes.data, self._joint_color.ctypes.data
            if depth_frame is not None:
                if depth_frame.dtype not in (torch.uint16, torch.int16):
                    raise ValueError("depth_frame must hold 16-bit integers")
                self._check(depth_frame, (self.F, self.H, self.W), depth_frame.dtype, "depth_frame")
            if self.frame_index is not None and tuple(self.frame_index.shape) != (B,):
                raise ValueError("frame_index holds %d hands, this call %d" % (self.frame_index.shape[0], B))
            d.frame_index, d.rgb, d.depth_frame = ptr(self.frame_index), rgb.data_ptr(), ptr(depth_frame)
            d.out, d.label, d.owner, d.prim, d.depth = (self._out[k].data_ptr() for k in ("image", "label", "owner", "prim", "depth"))
            d.B, d.F, d.H, d.W = B, self.F, self.H, self.W
            d.occl_margin, d.alpha, d.joint_radius, d.bone_half_width = self.occl_margin, self.alpha, self.joint_radius, self.bone_half_width
            L.check(L.load().kpf_overlay_draw_u8(L.C.byref(d), stream), "kpf_overlay_draw_u8")
        return dict(self._out)
