"""Inputs shared by tests/golden/gen_golden_dataset_item.py, tests/test_prep_annot_host.py and tests/test_prep_annot_gpu.py: synthetic RGB-D frames with
annotations that reach every branch of keypointfusion_amd/preprocess.py::prepare_annotated.  A frame is tests/prep_cases.py's disc of rippled depth; the
joints are scattered in a 120 mm box around a point on the ray through the disc's centre (at the disc's depth unless `jz` says otherwise)."""
import numpy as np

from keypointfusion_amd import preprocess as P

CAM = (600.0, 600.0, 320.0, 240.0)
CUBE = (250, 250, 250)
J = 21
# name: disc (cx, cy, z, r) in the TRUE frame, background depth, camera, hand (mirror = a left hand), jz (depth of the joints' box, default the disc's),
# given (offset in mm of a given centre from the joint mean: HO3D's refined centre), size (H, W)
CASES = {
    "right": dict(disc=(320, 240, 600, 60)),                                                  # 1. bounds inside the frame
    "left": dict(disc=(320, 240, 600, 60), mirror=True),                                      # 2. the same frame as a left hand
    "corner": dict(disc=(20, 15, 500, 50)),                                                   # 3. negative bounds, zero padding
    "left_edge": dict(disc=(622, 240, 500, 50), mirror=True),                                 # 4. a left hand at the right edge: mirror + padding
    "fx_ne_fy": dict(disc=(300, 200, 700, 45), cam=(615.0, 580.0, 310.5, 245.25)),            # 5. letterboxed crop
    "near": dict(disc=(320, 240, 200, 200)),                                                  # 6. bounds exceed the frame on all sides
    "far": dict(disc=(400, 300, 1400, 9)),                                                    # 7. a small source patch, scaled up
    "wall": dict(disc=(320, 240, 600, 60), bg=1200, jz=850),                                  # 8. wall behind the hand: zero candidates by the premax rule
    "given": dict(disc=(320, 240, 600, 60), given=(30.0, 0.0, 0.0)),                          # 9. HO3D: a given centre 30 mm off the joint mean
    "empty": dict(disc=(320, 240, 3000, 60), jz=600),                                         # 10. joint mean over empty depth: an empty cloud
    "hd_left": dict(disc=(1500, 480, 650, 70), mirror=True, cam=(1400.0, 1400.0, 960.0, 540.0), size=(1080, 1920)),  # the window test
}
SMALL = [n for n in CASES if n != "hd_left"]
HD_WINDOW = ((1270, 250), (460, 500))  # (x0, y0), (Hs, Ws): the part of hd_left's TRUE frame that holds the hand and its cube


def synth(name, seed=1, metres=False):
    """(rgb uint8 [H][W][3], depth uint16 [H][W], joints_mm float32 [J][3], cam float32 [4], mirror, center_xyz float32 [3] or None) of a case.  The
    joints are float32 METRES times 1000, which is how the reference's items get them (metres=True: the metres themselves)."""
    c = CASES[name]
    H, W = c.get("size", (480, 640))
    cx, cy, z, r = c["disc"]
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.full((H, W), c.get("bg", 0), np.uint16)
    m = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    depth[m] = (z + 30 * np.sin(xx[m] / 7.0) + g.randint(-5, 6, m.sum())).astype(np.uint16)
    # (a pattern in which neighbouring pixels differ, not noise: the reference's RGB crops of these frames are committed and have to compress)
    rgb = np.stack([(xx * (k + 1) + yy * (k + 3) + 40 * k) & 255 for k in range(3)], 2).astype(np.uint8)
    cam = np.asarray(c.get("cam", CAM), np.float32)
    jz = float(c.get("jz", z))
    mid = np.array([(cx - cam[2]) * jz / cam[0], (cy - cam[3]) * jz / cam[1], jz])
    jm = joints_m(mid, g)
    joints_mm = jm * 1000
    center = None
    if "given" in c:
        center = (joints_mm.astype(np.float64).mean(0) + np.asarray(c["given"])).astype(np.float32)
    return rgb, depth, jm if metres else joints_mm, cam, bool(c.get("mirror", False)), center


def joints_m(mid_mm, g):
    """[J][3] float32 metres scattered in a 120 mm box around mid_mm."""
    return ((np.asarray(mid_mm) + g.uniform(-60.0, 60.0, (J, 3))) / 1000.0).astype(np.float32)


def host_record(rgb, depth, joints_mm, cam, mirror, center, img_size=128, sample_num=1024):
    """prepare_annotated plus the integer record the device path reports: bounds, sz, M64 and all candidate points (as prep_cases.host_record)."""
    out = P.prepare_annotated(rgb, depth, joints_mm, cam, mirror, center, CUBE, img_size, sample_num)
    xs, xe, ys, ye, _, _ = P.annotated_bounds(out["com"], CUBE, cam)
    wb, hb = xe - xs, ye - ys
    sz = (img_size, int(hb * img_size / wb)) if wb > hb else (int(wb * img_size / hb), img_size)
    d = np.asarray(depth)[:, ::-1] if mirror else np.asarray(depth)
    _, M64 = P._crop_to_bounds(d, P.annotated_bounds(out["com"], CUBE, cam), (img_size, img_size), True)
    cand = P.depth_to_pcl(out["img"][0], out["center"], np.asarray(CUBE, np.float64), M64, tuple(float(c) for c in cam))
    out.update(bounds=np.array([xs, xe, ys, ye], np.int32), sz=np.array(sz, np.int32), M64=M64,
               candidates=np.clip(cand, -1, 1).astype(np.float32).reshape(-1, 3))
    return out


def flipped(rgb, depth, joints_mm, cam):
    """The mirror identity's other side: (rgb, depth, joints, centre) of the frame flipped left to right with the annotations moved with it (u -> W - 1 - u
    in float32, as the loader does), to be prepared with mirror=False.  The centre (the joints' mean) is GIVEN: joints next to a given centre are used as
    they are, while a second trip through the image could move them by an ulp."""
    W = depth.shape[1]
    uvd = P._project_f32(joints_mm, cam)
    uvd[:, 0] = np.float32(W) - uvd[:, 0] - np.float32(1)
    xyz = P._backproject_f32(uvd, cam)
    return np.ascontiguousarray(rgb[:, ::-1]), np.ascontiguousarray(depth[:, ::-1]), xyz, P._mean_rows_f32(xyz)


def random_hand(g):
    """A seeded random case for the comparison with the live reference: (rgb, depth, joints in METRES, cam, mirror, centre or None) on a 480 x 640 frame
    — discs anywhere (also partly outside), 250 .. 1300 mm, both hand types, two cameras, one in ten over empty depth, one in five with a given centre (right hands: HO3D)."""
    H, W = 480, 640
    cam = np.asarray(CAM if g.rand() < 0.5 else (615.0 + g.uniform(-20, 20), 580.0 + g.uniform(-20, 20), 310.5 + g.uniform(-9, 9), 245.25), np.float32)
    z = g.uniform(250, 1300)
    cx, cy, r = g.uniform(-20, W + 20), g.uniform(-20, H + 20), 36000.0 / z
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.full((H, W), 0 if g.rand() < 0.7 else int(z + g.uniform(60, 400)), np.uint16)
    m = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    zd = z if g.rand() < 0.9 else 3000.0  # one in ten: nothing but far depth under the joints, an empty cloud
    depth[m] = (zd + 30 * np.sin(xx[m] / 7.0) + g.randint(-5, 6, m.sum())).astype(np.uint16)
    rgb = np.stack([(xx * (k + 1) + yy * (k + 3) + 40 * k) & 255 for k in range(3)], 2).astype(np.uint8)
    jm = joints_m(np.array([(cx - cam[2]) * z / cam[0], (cy - cam[3]) * z / cam[1], z + g.uniform(-40, 40)]), g)
    given = g.rand() < 0.2
    mirror = bool(g.rand() < 0.5) and not given
    center = ((jm * 1000).astype(np.float64).mean(0) + g.uniform(-30, 30, 3)).astype(np.float32) if given else None
    return rgb, depth, jm, cam, mirror, center
