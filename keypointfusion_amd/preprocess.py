"""RGB-D crop preprocessing in front of the forward path: bounding box -> centre of mass -> metric crop ->
nearest-neighbour resize -> depth normalisation -> point-cloud sampling, and the un-crop of predicted joints.

Restates demo_RGBD.py:253-276 (get_center_from_bbx), :410-569 (Crop_Image_deep_pp[_RGB], comToBounds, getCrop), :378-385
(normalize_img), :345-376 (getpcl / depthToPCL), :300-343 (process_depth sampling), :192-212 (transformPoints2D) — the same
code lives in dataloader/loader.py:604-750, 843-893.  Host-side numpy like the reference's (the dataloader stays Python per
BASELINE.json north_star); OpenCV is not a dependency: cv2.resize(INTER_NEAREST) is restated (src = floor(dst * src/dst)).
Pinned by the reference's own committed crops (tests/test_preprocess.py).

prepare_annotated / uncrop_points_mirrored restate the DATASET items' test-time path instead (dataloader/loader.py:1113-1204 DexYCB, :1296-1416 HO3D): the
crop around an annotated 3-D centre, left hands mirrored, the labels, float32 up to the integer bounds.  Pinned to the reference's own items bit for bit
(tests/test_prep_annot_host.py, tests/golden/dataset_item.npz); DESIGN.md §4.9.

prepare_augmented / draw_augment restate the items' TRAINING path (dataloader/loader.py:1140-1156, :1325-1347, :363-593): the same crop, then one of the
reference's four augmentation modes and HO3D's colour scale.  Pinned to the reference's items bit for bit around the project's own nearest-neighbour warp rule
(warp_perspective_nearest / warp_affine_nearest: restated from OpenCV's algorithm, unpinned against a real OpenCV); tests/test_prep_augment_host.py,
tests/golden/augment_item.npz; DESIGN.md §4.10.
"""
import math

import numpy as np


def center_from_bbox(depth, bbox, upper=1500, lower=171):
    """demo_RGBD.py:253-276 — (u, v, d_mm) centre of mass of the valid depth inside an xywh box (x,y = top-left)."""
    c = np.array([0.0, 0.0, 300.0])
    x0, x1 = int(bbox[0]), int(bbox[0] + bbox[2])
    y0, y1 = int(bbox[1]), int(bbox[1] + bbox[3])
    img = depth[y0:y1, x0:x1]
    flag = np.logical_and(img <= upper, img >= lower)
    xv, yv = np.meshgrid(np.linspace(0, img.shape[1], img.shape[1]), np.linspace(0, img.shape[0], img.shape[0]))
    if flag.any():
        c[0], c[1], c[2] = np.mean(xv[flag]), np.mean(yv[flag]), np.mean(img[flag])
        if c[2] <= 0:
            c[2] = 300.0
    else:
        c[:] = (0.0, 0.0, 300.0)
    c[0] += bbox[0]
    c[1] += bbox[1]
    return c


def com_to_bounds(com, size, cam):
    """demo_RGBD.py:520-530 — pixel bounds of a metric cube of `size` mm around the centre of mass."""
    fx, fy, _, _ = cam
    zs, ze = com[2] - size[2] / 2.0, com[2] + size[2] / 2.0
    xs = int(np.floor((com[0] * com[2] / fx - size[0] / 2.0) / com[2] * fx + 0.5))
    xe = int(np.floor((com[0] * com[2] / fx + size[0] / 2.0) / com[2] * fx + 0.5))
    ys = int(np.floor((com[1] * com[2] / fy - size[1] / 2.0) / com[2] * fy + 0.5))
    ye = int(np.floor((com[1] * com[2] / fy + size[1] / 2.0) / com[2] * fy + 0.5))
    return xs, xe, ys, ye, zs, ze


def get_crop(img, xs, xe, ys, ye, zs, ze, thresh_z=True, background=0):
    """demo_RGBD.py:532-569 — crop with zero padding outside the image; depth values clamped to the cube in z."""
    H, W = img.shape[:2]
    c = img[max(ys, 0):min(ye, H), max(xs, 0):min(xe, W)].copy()
    pad = ((abs(ys) - max(ys, 0), abs(ye) - min(ye, H)), (abs(xs) - max(xs, 0), abs(xe) - min(xe, W)))
    if img.ndim == 3:
        pad = pad + ((0, 0),)
    c = np.pad(c, pad, mode="constant", constant_values=background)
    if thresh_z:
        m1 = np.logical_and(c < zs, c != 0)
        m2 = np.logical_and(c > ze, c != 0)
        c[m1] = zs
        c[m2] = 0.0
    return c


def resize_nearest(src, dsize):
    """cv2.resize(src, (w, h), interpolation=cv2.INTER_NEAREST): dst[y, x] = src[floor(y * sh/h), floor(x * sw/w)]."""
    w, h = dsize
    sh, sw = src.shape[:2]
    xi = np.minimum(np.floor(np.arange(w) * (sw / float(w))).astype(np.int64), sw - 1)
    yi = np.minimum(np.floor(np.arange(h) * (sh / float(h))).astype(np.int64), sh - 1)
    return src[yi][:, xi]


def crop_image(img, com, size, dsize, cam, thresh_z):
    """demo_RGBD.py:410-518 — returns (dsize crop, 3x3 image->crop affine)."""
    xs, xe, ys, ye, zs, ze = com_to_bounds(com, size, cam)
    cropped = get_crop(img, xs, xe, ys, ye, zs, ze, thresh_z=thresh_z)
    wb, hb = xe - xs, ye - ys
    sz = (dsize[0], int(hb * dsize[0] / wb)) if wb > hb else (int(wb * dsize[1] / hb), dsize[1])
    trans = np.eye(3)
    trans[0, 2], trans[1, 2] = -xs, -ys
    if cropped.shape[0] > cropped.shape[1]:
        scale = np.eye(3) * sz[1] / float(cropped.shape[0])
    else:
        scale = np.eye(3) * sz[0] / float(cropped.shape[1])
    scale[2, 2] = 1
    rz = resize_nearest(cropped, sz)
    shape = (dsize[1], dsize[0]) + ((img.shape[2],) if img.ndim == 3 else ())
    ret = np.zeros(shape, np.float32)
    x0 = int(np.floor(dsize[0] / 2.0 - rz.shape[1] / 2.0))
    y0 = int(np.floor(dsize[1] / 2.0 - rz.shape[0] / 2.0))
    ret[y0:y0 + rz.shape[0], x0:x0 + rz.shape[1]] = rz
    off = np.eye(3)
    off[0, 2], off[1, 2] = x0, y0
    return ret, np.dot(off, np.dot(scale, trans))


def normalize_depth(crop, com, cube):
    """demo_RGBD.py:378-385 — background / out-of-cube -> far plane, then (d - com_z) / (cube_z/2) in [-1, 1].
    All scalars are rounded to float32 first: the reference runs under NumPy 1.x value-based casting, where a float64 scalar
    combined with a float32 array computes in float32 (NumPy 2 would silently compute in float64 and round differently)."""
    d = crop.astype(np.float32, copy=True)
    far = np.float32(com[2] + cube[2] / 2.0)
    near = np.float32(com[2] - cube[2] / 2.0)
    premax = d.max()
    d[d == premax] = far
    d[d == 0] = far
    d[d >= far] = far
    d[d <= near] = near
    d -= np.float32(com[2])
    d /= np.float32(cube[2] / 2.0)
    return d


def image_to_3d(uvd, cam, flip=1):
    """demo_RGBD.py:387-408 jointImgTo3D."""
    fx, fy, fu, fv = cam
    uvd = np.asarray(uvd, np.float64)
    out = np.zeros_like(uvd, np.float32)
    out[..., 0] = (uvd[..., 0] - fu) * uvd[..., 2] / fx
    out[..., 1] = flip * (uvd[..., 1] - fv) * uvd[..., 2] / fy
    out[..., 2] = uvd[..., 2]
    return out


def depth_to_pcl(img_n, com3d, cube, M, cam, flip=1):
    """demo_RGBD.py:345-376 — normalised crop -> all foreground points, normalised to the cube."""
    fx, fy, fu, fv = cam
    mask = np.isclose(img_n, 1)
    dpt = img_n * cube[2] / 2.0 + com3d[2]
    dpt[mask] = 0
    valid = ~np.isclose(dpt, 0.0)
    pts = np.asarray(np.where(valid)).transpose()
    pts = np.concatenate([pts[:, [1, 0]] + 0.5, np.ones((pts.shape[0], 1), dtype="float32")], axis=1)
    pts = np.dot(np.linalg.inv(np.asarray(M)), pts.T).T
    pts = (pts[:, 0:2] / pts[:, 2][:, None]).reshape((pts.shape[0], 2))
    depth = dpt[valid]
    xyz = np.column_stack(((pts[:, 0] - fu) / fx * depth, flip * (pts[:, 1] - fv) / fy * depth, depth))
    return (xyz - com3d) / (np.asarray(cube) / 2.0)


def sample_points(pcl, n, rng):
    """demo_RGBD.py:319-332 — n points without replacement (tiling the cloud first when it is smaller than n), clamped to [-1,1].
    `rng` is a numpy RandomState (the reference uses the global np.random seeded with 0)."""
    num = pcl.shape[0]
    if num == 0:
        return np.zeros([n, 3], np.float32)
    idx = np.arange(num)
    if num < n:
        idx = np.append(idx.repeat(math.floor(n / num)), rng.choice(idx, size=divmod(n, num)[1], replace=False))
    sel = rng.choice(idx, n, replace=False)
    return np.clip(pcl[sel, :], -1, 1).astype(np.float32)


def prepare_rgbd(rgb, depth, bbox, cam, cube=(250.0, 250.0, 250.0), img_size=128, sample_num=1024, rng=None):
    """Everything demo_RGBD.py:72-108 does before the forward.  rgb H x W x 3 (any channel order, kept), depth H x W (mm),
    bbox xywh with x,y the top-left corner.  Returns numpy arrays ready to batch: img_rgb 3xSxS in [0,1], img 1xSxS in [-1,1],
    pcl Nx3, center (3,) mm, M 3x3, cube (3,), cam_para (4,)."""
    rng = np.random.RandomState(0) if rng is None else rng
    depth = np.asarray(depth)  # keep the sensor dtype (uint16 mm from cv2.imread(..., IMREAD_ANYDEPTH)): the reference's means and
    com = center_from_bbox(depth, bbox)  # z-clamps are computed on it (float64 mean, integer truncation of the near plane)
    crop_rgb, _ = crop_image(np.asarray(rgb), com, cube, (img_size, img_size), cam, thresh_z=False)
    crop_d, M = crop_image(depth, com, cube, (img_size, img_size), cam, thresh_z=True)
    img_n = normalize_depth(crop_d, com, cube)
    com3d = image_to_3d(com, cam)
    pcl = sample_points(depth_to_pcl(img_n, com3d, np.asarray(cube, np.float64), M, cam), sample_num, rng)
    return dict(img_rgb=(crop_rgb.astype(np.float32) / 255.0).transpose(2, 0, 1), img=img_n[None].astype(np.float32), pcl=pcl,
                center=com3d.astype(np.float32), M=M.astype(np.float32), cube=np.asarray(cube, np.float32),
                cam_para=np.asarray(cam, np.float32), crop_rgb=crop_rgb, com=com)


def _f32(v):
    return np.asarray(v, np.float32)


def _project_f32(xyz, cam):
    """loader.joint3DToImg (dataloader/loader.py:242-262, flip = 1) on float32 input: every operation rounded to float32."""
    fx, fy, fu, fv = (np.float32(c) for c in cam)
    xyz = _f32(xyz)
    out = np.zeros_like(xyz)
    out[..., 0] = xyz[..., 0] * fx / xyz[..., 2] + fu
    out[..., 1] = xyz[..., 1] * fy / xyz[..., 2] + fv
    out[..., 2] = xyz[..., 2]
    return out


def _backproject_f32(uvd, cam):
    """loader.jointImgTo3D (dataloader/loader.py:219-240, flip = 1) on float32 input, in float32."""
    fx, fy, fu, fv = (np.float32(c) for c in cam)
    uvd = _f32(uvd)
    out = np.zeros_like(uvd)
    out[..., 0] = (uvd[..., 0] - fu) * uvd[..., 2] / fx
    out[..., 1] = (uvd[..., 1] - fv) * uvd[..., 2] / fy
    out[..., 2] = uvd[..., 2]
    return out


def _mean_rows_f32(a):
    """np.mean(0) of a [J][3] float32 array: the rows added in order from zero, one float32 division by J."""
    acc = np.zeros(3, np.float32)
    for row in _f32(a):
        acc = acc + row
    return acc / np.float32(len(a))


def annotated_bounds(center_uvd, cube, cam):
    """loader.comToBounds (dataloader/loader.py:291-301) as the dataset items call it: the centre and the intrinsics are float32 and the cube a list of
    integers, so every operation is a float32 one.  Returns (xs, xe, ys, ye) as integers and (zs, ze) as float32."""
    u, v, d = (np.float32(c) for c in center_uvd)
    fx, fy = np.float32(cam[0]), np.float32(cam[1])
    hx, hy, hz = (np.float32(c / 2.0) for c in cube)
    half = np.float32(0.5)
    xs = int(np.floor((u * d / fx - hx) / d * fx + half))
    xe = int(np.floor((u * d / fx + hx) / d * fx + half))
    ys = int(np.floor((v * d / fy - hy) / d * fy + half))
    ye = int(np.floor((v * d / fy + hy) / d * fy + half))
    return xs, xe, ys, ye, d - hz, d + hz


def _crop_to_bounds(img, bounds, dsize, thresh_z):
    """crop_image from given bounds on: the same steps (get_crop, resize_nearest, letterbox, M in float64), restated because crop_image computes its
    bounds itself, in float64, and stays as it is."""
    xs, xe, ys, ye, zs, ze = bounds
    cropped = get_crop(img, xs, xe, ys, ye, zs, ze, thresh_z=thresh_z)
    wb, hb = xe - xs, ye - ys
    sz = (dsize[0], int(hb * dsize[0] / wb)) if wb > hb else (int(wb * dsize[1] / hb), dsize[1])
    trans = np.eye(3)
    trans[0, 2], trans[1, 2] = -xs, -ys
    if cropped.shape[0] > cropped.shape[1]:
        scale = np.eye(3) * sz[1] / float(cropped.shape[0])
    else:
        scale = np.eye(3) * sz[0] / float(cropped.shape[1])
    scale[2, 2] = 1
    rz = resize_nearest(cropped, sz)
    shape = (dsize[1], dsize[0]) + ((img.shape[2],) if img.ndim == 3 else ())
    ret = np.zeros(shape, np.float32)
    x0 = int(np.floor(dsize[0] / 2.0 - rz.shape[1] / 2.0))
    y0 = int(np.floor(dsize[1] / 2.0 - rz.shape[0] / 2.0))
    ret[y0:y0 + rz.shape[0], x0:x0 + rz.shape[1]] = rz
    off = np.eye(3)
    off[0, 2], off[1, 2] = x0, y0
    return ret, np.dot(off, np.dot(scale, trans))


def _annotated_base(where, rgb, depth, joints_mm, cam, mirror, center_xyz, cube, S):
    """What prepare_annotated and prepare_augmented (`where`, for the errors) do alike up to the two crops: the float32 intrinsics, the mirror, the joints'
    round trip through the image, the centre and its projection, the bounds and both crops.  Returns (cam, W, joint_xyz, center_xyz, center_uvd, crop_rgb,
    crop_d, M); joint_xyz is None without joints."""
    rgb, depth = np.asarray(rgb), np.asarray(depth)
    cam = tuple(np.float32(c) for c in cam)
    if len(cam) != 4 or len(cube) != 3:
        raise ValueError("%s: cam is (fx, fy, u0, v0) and cube three sizes in mm" % where)
    W = depth.shape[1]
    if mirror:
        rgb, depth = rgb[:, ::-1].copy(), depth[:, ::-1].copy()
    joint_xyz = None
    if joints_mm is not None:
        joints_mm = _f32(joints_mm)
        if joints_mm.ndim != 2 or joints_mm.shape[1] != 3:
            raise ValueError("%s: joints_mm must be [J][3] (got %s)" % (where, joints_mm.shape))
        joint_xyz = joints_mm
        if center_xyz is None or mirror:
            # DexYCB's item takes the joints through the image and back, mirrored or not (an ulp from the annotation at times); HO3D's item, the one with
            # a given centre, uses them as they are
            joint_uvd = _project_f32(joints_mm, cam)
            if mirror:
                joint_uvd[:, 0] = np.float32(W) - joint_uvd[:, 0] - np.float32(1)
            joint_xyz = _backproject_f32(joint_uvd, cam)
    if center_xyz is None:
        center_xyz = _mean_rows_f32(joint_xyz)
    else:
        center_xyz = _f32(center_xyz)
        if center_xyz.shape != (3,):
            raise ValueError("%s: center_xyz must be [3] (got %s)" % (where, center_xyz.shape))
    center_uvd = _project_f32(center_xyz, cam)
    bounds = annotated_bounds(center_uvd, cube, cam)
    crop_rgb, _ = _crop_to_bounds(rgb, bounds, (S, S), thresh_z=False)
    crop_d, M = _crop_to_bounds(depth, bounds, (S, S), thresh_z=True)
    return cam, W, joint_xyz, center_xyz, center_uvd, crop_rgb, crop_d, M


def _labels_to_image(lab64, hx, com3d, cam, M, S):
    """The labels' tail, joint_img from the labels normalised by the half cube (float64 [J][3]): curLabel * (cube[0] / 2.0) + com3D with an int64 or float64
    cube, so float64 from here to the stores into float32 arrays.  hx: cube[0] / 2.0."""
    p = lab64 * hx + com3d.astype(np.float64)
    fx, fy, fu, fv = (float(c) for c in cam)
    uvd = np.stack([p[:, 0] * fx / p[:, 2] + fu, p[:, 1] * fy / p[:, 2] + fv, p[:, 2]], 1).astype(np.float32)
    joint_img = uvd.copy()  # transformPoints2D: M . (u, v, 1) in float64, stored into the float32 array
    joint_img[:, 0] = M[0, 0] * uvd[:, 0].astype(np.float64) + M[0, 2]
    joint_img[:, 1] = M[1, 1] * uvd[:, 1].astype(np.float64) + M[1, 2]
    joint_img[:, 0:2] = joint_img[:, 0:2] / np.float32(S / 2) - np.float32(1)
    joint_img[:, 2] = (joint_img[:, 2] - com3d[2]).astype(np.float64) / hx
    return joint_img


def prepare_annotated(rgb, depth, joints_mm, cam, mirror=False, center_xyz=None, cube=(250, 250, 250), img_size=128, sample_num=1024, rng=None):
    """The reference's dataset items at test time (dataloader/loader.py:1113-1204 DexYCB, :1296-1416 HO3D; flip = 1): the crop around an ANNOTATED 3-D
    centre, left hands mirrored, and the labels.  joints_mm [J][3] float32 in camera space, mm, in the model's joint order (the caller applies
    DexYCB2MANO / HO3D2MANO); cam four float32 values; center_xyz None (the mean of the joints) or [3] float32 (HO3D's refined centre); joints_mm may be
    None when center_xyz is given (no ground truth: the labels are [21][3] zeros).  mirror: a left hand — the frame is flipped left to right and u -> W - u
    - 1.  With the joint-mean centre, or mirrored, the joints go through the image and back in float32 as in DexYCB's item; next to a given centre and
    unmirrored they are used as they are, as in HO3D's item.

    Returns the keys of prepare_rgbd plus joint [J][3] (normalised xyz: DeviceEvaluator.update's xyz_gt), joint_img [J][3] (normalised uvd), mirror and
    frame_w.  Precisions are the reference's under the NumPy it runs on here (2.x): everything up to the integer bounds is float32 (annotations and
    intrinsics are np.float32 there), M is float64, joint is float32, center is the float32 round trip of the centre through the image (an ulp from
    center_xyz at times), and joint_img goes through a float64 intermediate because the reference's cube is an integer array."""
    rng = np.random.RandomState(0) if rng is None else rng
    if joints_mm is None and center_xyz is None:
        raise ValueError("prepare_annotated: neither joints nor a centre: nothing to crop around")
    cam, W, joint_xyz, center_xyz, center_uvd, crop_rgb, crop_d, M = _annotated_base("prepare_annotated", rgb, depth, joints_mm, cam, mirror, center_xyz, cube,
                                                                                     img_size)
    img_n = normalize_depth(crop_d, center_uvd, cube)
    com3d = _backproject_f32(center_uvd, cam)
    half = np.float32(cube[2] / 2.0)
    if joint_xyz is None:
        J = 21
        joint, joint_img = np.zeros((J, 3), np.float32), np.zeros((J, 3), np.float32)
    else:
        joint = (joint_xyz - center_xyz) / half
        joint_img = _labels_to_image(joint.astype(np.float64), cube[0] / 2.0, com3d, cam, M, img_size)
    cube64 = np.asarray(cube, np.float64)
    cam64 = tuple(float(c) for c in cam)
    pcl = sample_points(depth_to_pcl(img_n, com3d, cube64, M, cam64), sample_num, rng)
    return dict(img_rgb=(crop_rgb.astype(np.float32) / 255.0).transpose(2, 0, 1), img=img_n[None].astype(np.float32), pcl=pcl, center=com3d,
                M=M.astype(np.float32), cube=np.asarray(cube, np.float32), cam_para=np.asarray(cam, np.float32), crop_rgb=crop_rgb,
                com=center_uvd.astype(np.float64), joint=joint.astype(np.float32), joint_img=joint_img, mirror=bool(mirror), frame_w=int(W))


AUG_MODES = ("rot", "com", "sc", "none")  # the reference's aug_modes order: aug["mode"] indexes it


def _invert_crop_matrix(M):
    """np.linalg.inv of a crop matrix [[s, 0, t], [0, s', u], [0, 0, 1]] as the LAPACK behind NumPy computes it (no pivoting happens, the triangular solve
    multiplies by the RECIPROCAL of the diagonal): entries 1 / s, 1 / s', (-t) * (1 / s), (-u) * (1 / s').  Checked against np.linalg.inv by
    tests/golden/gen_golden_augment.py on every case."""
    r0, r1 = 1.0 / M[0, 0], 1.0 / M[1, 1]
    return np.array([[r0, 0.0, -M[0, 2] * r0], [0.0, r1, -M[1, 2] * r1], [0.0, 0.0, 1.0]])


def _dot_crop_matrices(Mn, Mi):
    """np.dot(Mn, Mi) of two matrices of that form: every product and the one sum rounded separately."""
    return np.array([[Mn[0, 0] * Mi[0, 0], 0.0, Mn[0, 0] * Mi[0, 2] + Mn[0, 2]], [0.0, Mn[1, 1] * Mi[1, 1], Mn[1, 1] * Mi[1, 2] + Mn[1, 2]], [0.0, 0.0, 1.0]])


def _warp_take(src, X, Y, ok):
    S0, S1 = src.shape[:2]
    ok = ok & (X >= 0) & (X < S1) & (Y >= 0) & (Y < S0)
    xi, yi = np.where(ok, X, 0).astype(np.int64), np.where(ok, Y, 0).astype(np.int64)
    out = src[yi, xi]
    out[~ok] = 0
    return out


def warp_perspective_nearest(src, A):
    """cv2.warpPerspective(src, A, src.shape, flags=INTER_NEAREST, borderMode=BORDER_CONSTANT, borderValue=0), restated from OpenCV's algorithm (UNPINNED:
    no OpenCV on the build machines; a pixel on a rounding boundary may differ from a real OpenCV).  The rule, float64, every operation rounded once, in
    this order:
      det = a00 (a11 a22 - a12 a21) - a01 (a10 a22 - a12 a20) + a02 (a10 a21 - a11 a20);  d = 1 / det
      Ai = [[(a11 a22 - a12 a21) d, (a02 a21 - a01 a22) d, (a01 a12 - a02 a11) d],
            [(a12 a20 - a10 a22) d, (a00 a22 - a02 a20) d, (a02 a10 - a00 a12) d],
            [(a10 a21 - a11 a20) d, (a01 a20 - a00 a21) d, (a00 a11 - a01 a10) d]]
      per destination pixel (x, y):  W = (Ai20 x + Ai21 y) + Ai22;  W = 1 / W if W != 0 else 0
      X = rint((Ai00 x + (Ai01 y + Ai02)) W),  Y = rint((Ai10 x + (Ai11 y + Ai12)) W)       (half to even)
      dst[y, x] = src[Y, X] if 0 <= X < width and 0 <= Y < height (and both are finite) else 0"""
    a = np.asarray(A, np.float64)
    det = a[0, 0] * (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) - a[0, 1] * (a[1, 0] * a[2, 2] - a[1, 2] * a[2, 0]) + a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0])
    with np.errstate(all="ignore"):
        d = 1.0 / np.float64(det)
        Ai = np.array([[(a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) * d, (a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]) * d, (a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]) * d],
                       [(a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]) * d, (a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]) * d, (a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]) * d],
                       [(a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]) * d, (a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]) * d, (a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]) * d]])
        x = np.arange(src.shape[1], dtype=np.float64)[None, :]
        y = np.arange(src.shape[0], dtype=np.float64)[:, None]
        W = (Ai[2, 0] * x + Ai[2, 1] * y) + Ai[2, 2]
        W = np.where(W != 0, 1.0 / np.where(W != 0, W, 1.0), 0.0)
        X = np.rint((Ai[0, 0] * x + (Ai[0, 1] * y + Ai[0, 2])) * W)
        Y = np.rint((Ai[1, 0] * x + (Ai[1, 1] * y + Ai[1, 2])) * W)
    return _warp_take(src, X, Y, np.isfinite(X) & np.isfinite(Y))


def rotation_matrix_2d(cx, cy, c, s):
    """cv2.getRotationMatrix2D((cx, cy), -rot, 1) with (c, s) = (cos, sin) of rot: alpha = c, beta = -s,
    [[alpha, beta, (1 - alpha) cx - beta cy], [-beta, alpha, beta cx + (1 - alpha) cy]]."""
    cx, cy = float(cx), float(cy)
    al, be = float(c), -float(s)
    return np.array([[al, be, (1.0 - al) * cx - be * cy], [-be, al, be * cx + (1.0 - al) * cy]])


def warp_affine_nearest(src, M2):
    """cv2.warpAffine(src, M2, src.shape, flags=INTER_NEAREST, borderMode=BORDER_CONSTANT, borderValue=0), restated from OpenCV's algorithm (UNPINNED, as
    warp_perspective_nearest).  The rule, float64, every operation rounded once:
      D = m00 m11 - m01 m10;  D = 1 / D if D != 0 else 0
      i00 = m11 D, i11 = m00 D, i01 = m01 (-D), i10 = m10 (-D);  i02 = (-i00) m02 - i01 m12,  i12 = (-i10) m02 - i11 m12
      X = (rint((i01 y + i02) 1024) + 512 + rint((i00 x) 1024)) >> 10,  Y = (rint((i11 y + i12) 1024) + 512 + rint((i10 x) 1024)) >> 10   (half to even;
      OpenCV's 10-bit fixed point; a term that is not finite or reaches 2^40 makes the pixel a border pixel)
      dst[y, x] = src[Y, X] if 0 <= X < width and 0 <= Y < height else 0"""
    m = np.asarray(M2, np.float64)
    with np.errstate(all="ignore"):
        D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
        D = 1.0 / D if D != 0 else 0.0
        i00, i11, i01, i10 = m[1, 1] * D, m[0, 0] * D, m[0, 1] * -D, m[1, 0] * -D
        i02 = -i00 * m[0, 2] - i01 * m[1, 2]
        i12 = -i10 * m[0, 2] - i11 * m[1, 2]
        x = np.arange(src.shape[1], dtype=np.float64)[None, :]
        y = np.arange(src.shape[0], dtype=np.float64)[:, None]
        tx0, tx1 = np.rint((i01 * y + i02) * 1024.0), np.rint((i00 * x) * 1024.0)
        ty0, ty1 = np.rint((i11 * y + i12) * 1024.0), np.rint((i10 * x) * 1024.0)
        lim = 2.0 ** 40
        ok = (np.abs(tx0) < lim) & (np.abs(tx1) < lim) & (np.abs(ty0) < lim) & (np.abs(ty1) < lim)  # (NaN compares false)
        X = np.floor(((np.where(ok, tx0, 0.0) + 512.0) + np.where(ok, tx1, 0.0)) / 1024.0)  # exact integers below 2^42: floor(/1024) is >> 10
        Y = np.floor(((np.where(ok, ty0, 0.0) + 512.0) + np.where(ok, ty1, 0.0)) / 1024.0)
    return _warp_take(src, X, Y, ok)


def _aug_transform(com, size, S, cam):
    """loader.comToTransform (dataloader/loader.py:303-338): bounds in float32 (annotated_bounds), then float64; the letterbox offset comes from the UNTRUNCATED
    resize size (sz = hb * S / wb as a float), unlike the crop's own M.  None when the bounds are degenerate."""
    try:
        xs, xe, ys, ye, _, _ = annotated_bounds(com, size, cam)
    except (OverflowError, ValueError):  # a bound that is not finite (a centre moved to depth 0)
        return None
    wb, hb = xe - xs, ye - ys
    if wb <= 0 or hb <= 0 or max(abs(v) for v in (xs, xe, ys, ye)) >= 2 ** 28:  # (the device saturates its bounds there: refused on both sides)
        return None
    if wb > hb:
        scale, sz = float(S) / float(wb), (float(S), hb * float(S) / wb)
    else:
        scale, sz = float(S) / float(hb), (wb * float(S) / hb, float(S))
    x0, y0 = float(np.floor(S / 2.0 - sz[0] / 2.0)), float(np.floor(S / 2.0 - sz[1] / 2.0))
    return np.array([[scale, 0.0, scale * float(-xs) + x0], [0.0, scale, scale * float(-ys) + y0], [0.0, 0.0, 1.0]])


def _rot_cs(rot):
    a = np.mod(np.float64(rot), 360) * np.pi / 180.0
    return np.float64(np.cos(a)), np.float64(np.sin(a))


def prepare_augmented(rgb, depth, joints_mm, cam, aug, mirror=False, center_xyz=None, cube=(250, 250, 250), img_size=128, sample_num=1024, rng=None):
    """The reference's dataset items at TRAINING time (dataloader/loader.py:1140-1156 DexYCB, :1325-1347 HO3D): prepare_annotated up to the two crops, then
    augmentCrop / augmentCrop_RGB (moveCoM, rotateHand, scaleHand, recropHand, comToTransform), normalize_img with the pre-augmentation maximum, and the
    labels.  aug: dict with mode 0..3 (AUG_MODES: rot, com, sc, none), off [3] float64 mm, rot float64 degrees, sc float64, optional rot_cs = (cos, sin) of
    np.mod(rot, 360) * pi / 180 as float64 (absent: computed with NumPy; given: no trigonometric function is called) and optional color [3] float64 (HO3D's
    colour scale: clip(crop * color, 0, 255) in float64 before the float32 cast and the / 255).  joints_mm is required (a training item has labels).

    Returns prepare_annotated's keys (center, M, cube, com, joint, joint_img, img, img_rgb, pcl of the training item) plus M64, cube64 and aug_status (bit 0:
    the depth side was augmented; bit 1: the parameters were REFUSED — a non-finite value, sc <= 0, a centre moved to where it does not project, or degenerate new bounds — and the sample was prepared as
    mode none without colour).

    Precisions, the reference's under NumPy 2: the crop, the centre and every bound are prepare_annotated's (float32); the augmented centre is projected in
    float64 and stored as float32; Mnew, the inverse maps and the warps are float64; the z-threshold and normalize_img are float32; the labels are divided by
    the float64 half cube and stay FLOAT64 into joint_img (so mode none differs from the test item in joint_img), joint is their float32 rounding.  The
    early exits are the reference's: allclose(off, 0), allclose(rot, 0), allclose(sc, 1), an all-zero depth crop (depth and labels stay, RGB is warped all the
    same), and the com[2] guards.  The reference's `warped[warped < min - 1] = background` lines are left out: a nearest-neighbour warp with a zero border
    returns only values of the source crop or 0; the non-zero ones are >= min > min - 1, and a 0 is only rewritten to the background, which is 0.
    The two warps are warp_perspective_nearest and warp_affine_nearest: the project's own rule, unpinned against a real OpenCV."""
    rng = np.random.RandomState(0) if rng is None else rng
    if joints_mm is None:
        raise ValueError("prepare_augmented: joints_mm is required: a training item has labels")
    mode = int(aug["mode"])
    off = np.asarray(aug["off"], np.float64)
    rot, sc = np.float64(aug["rot"]), np.float64(aug["sc"])
    if not 0 <= mode <= 3 or off.shape != (3,):
        raise ValueError("prepare_augmented: aug['mode'] is 0..3 (%s) and aug['off'] three mm" % (AUG_MODES,))
    c, s = (np.float64(v) for v in aug["rot_cs"]) if aug.get("rot_cs") is not None else _rot_cs(rot) if np.isfinite(rot) else (np.float64("nan"),) * 2
    color = None if aug.get("color") is None else np.asarray(aug["color"], np.float64)
    if color is not None and color.shape != (3,):
        raise ValueError("prepare_augmented: aug['color'] is three factors")
    S = int(img_size)
    cam, W, joint_xyz, center_xyz, com, crop_rgb, crop_d, M = _annotated_base("prepare_augmented", rgb, depth, joints_mm, cam, mirror, center_xyz, cube, S)
    gt = joint_xyz - center_xyz  # gt3Dcrop, float32
    premax = crop_d.max()
    cube64 = np.asarray(cube, np.float64)  # cube[k] / 2.0 is a float64 in every mode (an int64 array, or the list of Python floats of scaleHand)

    # -- the geometry of the mode: Mnew / A for the perspective warp, or the 2 x 3 matrix of the rotation; None = an early exit
    status = 0
    finite = bool(np.isfinite(off).all() and np.isfinite(rot) and np.isfinite(sc) and np.isfinite(c) and np.isfinite(s) and sc > 0
                  and (color is None or np.isfinite(color).all()))
    new_com, new_cube, Mnew, A, R = com, cube64, M, None, None
    shift = False
    com3d_old = _backproject_f32(com, cam)
    with np.errstate(all="ignore"):
        if finite and mode == 1 and not np.allclose(off, 0.0):
            p = com3d_old.astype(np.float64) + off  # joint3DToImg of a float64 point: float64, stored as float32
            fx, fy, fu, fv = (np.float64(v) for v in cam)
            new_com = np.array([p[0] * fx / p[2] + fu, p[1] * fy / p[2] + fv, p[2]]).astype(np.float32)
            shift = True
            if not np.isfinite(new_com).all():  # the offset moved the centre into the camera plane: refused
                Mnew = None
            elif not (np.allclose(com[2], 0.0) or np.allclose(new_com[2], 0.0)):
                Mnew = _aug_transform(new_com, cube, S, cam)
        elif finite and mode == 2 and not np.allclose(sc, 1.0):
            new_cube = np.array([float(v) * float(sc) for v in cube])
            if not np.allclose(com[2], 0.0):
                Mnew = _aug_transform(com, new_cube, S, cam)
        elif finite and mode == 0 and not np.allclose(rot, 0.0):
            R = rotation_matrix_2d(S // 2, S // 2, c, s)
        if Mnew is not None and Mnew is not M:
            A = _dot_crop_matrices(Mnew, _invert_crop_matrix(M))
            if not (np.isfinite(A).all() and A[0, 0] != 0 and A[1, 1] != 0):
                Mnew = None
    if not finite or Mnew is None:  # refused: mode none, no colour
        status, mode, color = 2, 3, None
        new_com, new_cube, Mnew, A, R, shift = com, cube64, M, None, None, False

    # -- RGB: warped whatever the depth crop holds (augmentCrop_RGB has no all-zero test)
    crop_rgb_aug = crop_rgb
    if A is not None:
        crop_rgb_aug = warp_perspective_nearest(crop_rgb, A)
    elif R is not None:
        crop_rgb_aug = warp_affine_nearest(crop_rgb, R)
    if color is not None:
        crop_rgb_aug = np.clip(crop_rgb_aug * color[None, None, :], 0, 255)
    crop_rgb_aug = crop_rgb_aug.astype(np.float32)

    # -- depth and labels
    d = crop_d.astype(np.float32, copy=True)
    lab = gt
    if premax == 0:  # an all-zero crop: depth, labels, com, M and cube stay
        new_com, new_cube, Mnew = com, cube64, M
    else:
        if A is not None or R is not None or shift or new_cube is not cube64:
            status |= 1
        if A is not None:
            d = warp_perspective_nearest(d, A)
            zc = new_com if mode == 1 else com  # recropHand's z-threshold: the new centre with the OLD cube (also in mode sc)
            zs, ze = zc[2] - np.float32(cube[2] / 2.0), zc[2] + np.float32(cube[2] / 2.0)
            m1, m2 = np.logical_and(d < zs, d != 0), np.logical_and(d > ze, d != 0)
            d[m1] = zs
            d[m2] = 0.0
        elif R is not None:
            d = warp_affine_nearest(d, R)
        if shift:
            lab = gt + com3d_old - _backproject_f32(new_com, cam)
        elif R is not None:
            j2 = _project_f32(gt + com3d_old, cam)
            pp = j2[:, 0:2] - com[0:2]
            pr = np.zeros_like(j2)
            pr[:, 0] = pp[:, 0].astype(np.float64) * c - pp[:, 1].astype(np.float64) * s
            pr[:, 1] = pp[:, 0].astype(np.float64) * s + pp[:, 1].astype(np.float64) * c
            pr[:, 2] = j2[:, 2]
            pr[:, 0:2] += com[0:2]
            lab = _backproject_f32(pr, cam) - com3d_old
    # normalize_img(premax, imgD, com, cube): float32 scalars (a float32 centre and Python-float halves)
    hz = np.float32(new_cube[2] / 2.0)
    far, near = new_com[2] + hz, new_com[2] - hz
    d[d == premax] = far
    d[d == 0] = far
    d[d >= far] = far
    d[d <= near] = near
    d -= new_com[2]
    d /= hz
    com3d = _backproject_f32(new_com, cam)
    lab64 = lab.astype(np.float64) / (new_cube[2] / 2.0)
    with np.errstate(all="ignore"):
        joint_img = _labels_to_image(lab64, new_cube[0] / 2.0, com3d, cam, Mnew, S)
    cam64 = tuple(float(v) for v in cam)
    pcl = sample_points(depth_to_pcl(d, com3d, new_cube, Mnew, cam64), sample_num, rng)
    return dict(img_rgb=(crop_rgb_aug / np.float32(255.0)).transpose(2, 0, 1), img=d[None].astype(np.float32), pcl=pcl, center=com3d,
                M=Mnew.astype(np.float32), cube=new_cube.astype(np.float32), cam_para=np.asarray(cam, np.float32), crop_rgb=crop_rgb_aug,
                com=new_com.astype(np.float64), joint=lab64.astype(np.float32), joint_img=joint_img, mirror=bool(mirror), frame_w=int(W),
                M64=Mnew, cube64=new_cube, aug_status=int(status))


# ---- drawing the augmentation parameters: the counter hash of kpf_prep.hip (hash32 / prep_seed_base), vectorised over the seeds
AUG_SALT = 0xa4093822


def _hash32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    return x ^ (x >> np.uint64(16))


def draw_augment(seed, sigma_com=10.0, sigma_sc=0.2, rot_range=180.0, color_factor=0.0):
    """The host twin of kpf_prep_aug_draw: the reference's rand_augment (dataloader/loader.py:495-498) and HO3D's colour scale, drawn from seed [B] int64 by
    the sampler's counter hash.  Word k of sample b = hash32(base ^ hash32(k * 0x85ebca6b + AUG_SALT)), base = prep_seed_base(seed[b]); uniform i = ((word 2i
    << 21) | (word 2i+1 >> 11)) * 2^-53, mapped a + (b - a) * u like random.uniform.  mode = floor(4 u0); off = (-1 + 2 u1..3) * sigma_com; rot = -range + (2
    range) u4; sc = |1 + (-1 + 2 u5) * sigma_sc|; color = (1 - f) + ((1 + f) - (1 - f)) u6..8; rot_cs = (cos, sin)(mod(rot, 360) pi / 180) with NumPy.  Python's
    Mersenne-Twister stream (the reference's `random`) is NOT reproduced: the distribution is.  Returns dict(mode [B] int32, off [B][3], rot [B], sc [B],
    rot_cs [B][2], color [B][3]) of float64."""
    seed = np.atleast_1d(np.asarray(seed, np.int64)).view(np.uint64)
    lo, hi = seed & np.uint64(0xffffffff), seed >> np.uint64(32)
    base = _hash32(lo ^ _hash32((hi + np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)))
    k = np.arange(18, dtype=np.uint64)[None, :]
    w = _hash32(base[:, None] ^ _hash32((k * np.uint64(0x85ebca6b) + np.uint64(AUG_SALT)) & np.uint64(0xffffffff)))
    u = ((w[:, 0::2] << np.uint64(21)) | (w[:, 1::2] >> np.uint64(11))).astype(np.float64) * 2.0 ** -53
    sigma_com, sigma_sc, rot_range, f = float(sigma_com), float(sigma_sc), float(rot_range), float(color_factor)
    mode = np.floor(4.0 * u[:, 0]).astype(np.int32)
    off = (-1.0 + 2.0 * u[:, 1:4]) * sigma_com
    rot = -rot_range + (rot_range - -rot_range) * u[:, 4]
    sc = np.abs(1.0 + (-1.0 + 2.0 * u[:, 5]) * sigma_sc)
    color = (1.0 - f) + ((1.0 + f) - (1.0 - f)) * u[:, 6:9]
    a = np.mod(rot, 360) * np.pi / 180.0
    return dict(mode=mode, off=off, rot=rot, sc=sc, rot_cs=np.stack([np.cos(a), np.sin(a)], 1), color=color)


def uncrop_points_mirrored(uv, M, mirror, frame_w):
    """uncrop_points for a prepare_annotated sample: a mirrored sample's u goes back to the camera's own frame (u -> frame_w - 1 - u, float64).  The depth
    column, and the predicted xyz it came from, stay in the mirrored camera's space, as in the reference."""
    out = uncrop_points(uv, M)
    if mirror:
        out[:, 0] = (frame_w - 1) - out[:, 0]
    return out


def project_to_crop(xyz_nl, center, M, cube, cam, img_size=128, flip=1):
    """loader.xyz_nl2uvdnl_tensor (dataloader/loader.py:821-834; demo_RGBD.py:121-123): normalised xyz joints -> pixel coordinates in
    the crop (u, v in [0, img_size), d in mm): de-normalise, pinhole-project (points3DToImg), apply the crop matrix M."""
    xyz = np.asarray(xyz_nl, np.float64) * (np.asarray(cube, np.float64) / 2.0) + np.asarray(center, np.float64)
    fx, fy, u0, v0 = [float(c) for c in cam]
    u = xyz[:, 0] * fx / xyz[:, 2] + u0
    v = flip * xyz[:, 1] * fy / xyz[:, 2] + v0
    h = np.stack([u, v, np.ones_like(u)], 1) @ np.asarray(M, np.float64).T
    return np.stack([h[:, 0], h[:, 1], xyz[:, 2]], 1)


def uncrop_points(uv, M):
    """demo_RGBD.py:192-212 — crop pixel coordinates back to the original image (projective divide included)."""
    Mi = np.linalg.inv(np.asarray(M, np.float64))
    uv = np.asarray(uv, np.float64)
    h = np.concatenate([uv[:, :2], np.ones((uv.shape[0], 1))], 1) @ Mi.T
    out = uv.copy()
    out[:, :2] = h[:, :2] / h[:, 2:3]
    return out
