"""The analytic video shared by tests/test_tracking_host.py and tests/test_tracking_gpu.py: two discs of depth moving through ONE 640 x 480 camera frame
(each built as tests/prep_cases.py builds its disc: sinusoidal ripple, +-5 mm noise, no background), and an analytic "forward" that puts 21 joints on a ring
of 0.8 r around a disc's current centre.  Camera and cube are prep_cases' (600, 600, 320, 240) and 250 mm."""
import numpy as np

import prep_cases as PC

H, W, J, FRAMES = 480, 640, 21, 10
CAM, CUBE = PC.CAM, PC.CUBE
# (centre x, y at frame 0, z mm, radius px), velocity px per frame
DISCS = (((200.0, 240.0, 600.0, 60.0), (6.0, 4.0)), ((450.0, 200.0, 700.0, 45.0), (5.0, -3.0)))
FIRST_BOX = [[d[0] - 70.0, d[1] - 70.0, 140.0, 140.0] for d, _ in DISCS]  # the 140-px square centred on each disc's start position
_ANGLE = 2.0 * np.pi * np.arange(J) / J
RING = np.stack([np.cos(_ANGLE), np.sin(_ANGLE)], 1)  # [J][2] float64 unit offsets


def centre(track, t):
    (cx, cy, _, _), (vx, vy) = DISCS[track]
    return np.array([cx + vx * t, cy + vy * t], np.float64)


def frame(t):
    """(rgb [H][W][3] uint8, depth [H][W] uint16) of frame t: both discs."""
    g = np.random.RandomState(100 + t)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.zeros((H, W), np.uint16)
    for k, ((_, _, z, r), _) in enumerate(DISCS):
        cx, cy = centre(k, t)
        m = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
        depth[m] = (z + 30 * np.sin(xx[m] / 7.0) + g.randint(-5, 6, m.sum())).astype(np.uint16)
    rgb = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    return rgb, depth


def ring_px(track, t):
    """[J][2] float32 frame pixels: the analytic forward's joints of `track` at frame t."""
    return (centre(track, t) + 0.8 * DISCS[track][0][3] * RING).astype(np.float32)
