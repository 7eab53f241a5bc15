"""Inputs shared by tests/test_prep_host.py and tests/test_preprocess_gpu.py: the demo frame (whole and as a window) and synthetic 480 x 640 RGB-D frames
that reach every branch of keypointfusion_amd/preprocess.py (a disc of depth with a sinusoidal ripple and +-5 mm noise)."""
import os

import numpy as np

from conftest import GOLDEN
from keypointfusion_amd import preprocess as P

CAM = (600.0, 600.0, 320.0, 240.0)
CUBE = (250.0, 250.0, 250.0)
# name: disc (cx, cy, z, r), background depth, box, camera
CASES = {
    "centre": dict(disc=(320, 240, 600, 60), bg=0, bbox=[250, 170, 140, 140], cam=CAM),           # N = 2969, bounds inside the frame
    "corner": dict(disc=(20, 15, 500, 50), bg=0, bbox=[0, 0, 80, 70], cam=CAM),                    # zero padding; N = 733 < 1024: tiling
    "far_small": dict(disc=(400, 300, 1400, 9), bg=0, bbox=[385, 285, 30, 30], cam=CAM),           # N = 357: tiling, quotient 2, remainder 310
    "near_big": dict(disc=(320, 240, 200, 200), bg=0, bbox=[100, 20, 440, 440], cam=CAM),          # bounds exceed the frame; N = 16384
    "background_wall": dict(disc=(320, 240, 600, 60), bg=1200, bbox=[250, 170, 140, 140], cam=CAM),  # N = 0 through the premax rule
    "empty": dict(disc=(320, 240, 3000, 60), bg=0, bbox=[250, 170, 140, 140], cam=CAM),            # no valid depth: com = box corner at 300 mm
    "full_wall": dict(disc=(320, 240, 600, 2000), bg=0, bbox=[250, 170, 140, 140], cam=CAM),     # the whole crop is foreground: the largest sort
    "fx_ne_fy": dict(disc=(300, 200, 700, 45), bg=0, bbox=[240, 140, 120, 120], cam=(615.0, 580.0, 310.5, 245.25)),  # 219 x 207 crop -> 128 x 120
}


def synth_frame(name, seed=1, H=480, W=640):
    c = CASES[name]
    cx, cy, z, r = c["disc"]
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.full((H, W), c["bg"], np.uint16)
    m = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    depth[m] = (z + 30 * np.sin(xx[m] / 7.0) + g.randint(-5, 6, m.sum())).astype(np.uint16)
    rgb = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    return rgb, depth, [float(v) for v in c["bbox"]], c["cam"]


def demo_window():
    """(rgb window, depth window, bbox, cam, (x0, y0), (H, W)) of the reference's sample frame (tests/test_preprocess.py::_frame embeds it in zeros)."""
    from PIL import Image
    meta = {}
    for line in open(os.path.join(GOLDEN, "demo_box_window.txt")):
        k, *v = line.split()
        meta[k] = [float(x) for x in v]
    y0, x0 = int(meta["window_y0"][0]), int(meta["window_x0"][0])
    H, W = int(meta["frame_h"][0]), int(meta["frame_w"][0])
    rgbw = np.array(Image.open(os.path.join(GOLDEN, "demo_box_rgb_window.png")))
    dw = np.array(Image.open(os.path.join(GOLDEN, "demo_box_depth_window.png")))
    cx, cy, w, h = meta["bbox_norm"]
    bbox = [cx * W, cy * H, w * W, h * H]
    bbox[0] -= bbox[2] / 2
    bbox[1] -= bbox[3] / 2
    return np.ascontiguousarray(rgbw), np.ascontiguousarray(dw), bbox, tuple(meta["cam"]), (x0, y0), (H, W)


def embed(rgbw, dw, origin, frame_size):
    (x0, y0), (H, W) = origin, frame_size
    rgb = np.zeros((H, W, 3), np.uint8)
    depth = np.zeros((H, W), np.uint16)
    rgb[y0:y0 + rgbw.shape[0], x0:x0 + rgbw.shape[1]] = rgbw
    depth[y0:y0 + dw.shape[0], x0:x0 + dw.shape[1]] = dw
    return rgb, depth


def host_record(rgb, depth, bbox, cam, cube=CUBE, img_size=128):
    """prepare_rgbd plus the integer record the device path reports: bounds (xs, xe, ys, ye), sz (w, h), the float64 M and all candidate points."""
    out = P.prepare_rgbd(rgb, depth, bbox, cam, cube, img_size)
    com = out["com"]
    xs, xe, ys, ye, zs, ze = P.com_to_bounds(com, cube, cam)
    wb, hb = xe - xs, ye - ys
    sz = (img_size, int(hb * img_size / wb)) if wb > hb else (int(wb * img_size / hb), img_size)
    _, M64 = P.crop_image(np.asarray(depth), com, cube, (img_size, img_size), cam, thresh_z=True)
    cand = P.depth_to_pcl(out["img"][0], P.image_to_3d(com, cam), np.asarray(cube, np.float64), M64, cam)
    out.update(bounds=np.array([xs, xe, ys, ye], np.int32), sz=np.array(sz, np.int32), M64=M64,
               candidates=np.clip(cand, -1, 1).astype(np.float32).reshape(-1, 3))
    return out


def floor_margin(com, cam, cube=CUBE):
    """Distance of com_to_bounds' four floor(x + 0.5) arguments from an integer (the device's centre of mass differs from the host's by its float64
    summation order, a few 1e-13 relative: a case is usable when this margin is >= 1e-6)."""
    fx, fy = cam[0], cam[1]
    a = [(com[0] * com[2] / fx - cube[0] / 2.0) / com[2] * fx + 0.5, (com[0] * com[2] / fx + cube[0] / 2.0) / com[2] * fx + 0.5,
         (com[1] * com[2] / fy - cube[1] / 2.0) / com[2] * fy + 0.5, (com[1] * com[2] / fy + cube[1] / 2.0) / com[2] * fy + 0.5]
    return min(min(v - np.floor(v), np.ceil(v) - v) for v in a)
