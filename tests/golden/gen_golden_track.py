"""Known answers of the reference loader's box rule (dataloader/loader.py:1250-1251: `get_bbox(joints, expansion_factor=1.5)` followed by
`process_bbox(bbox, width, height, expansion_factor=1.0)`, :1432-1480) for keypointfusion_amd/tracking.py::next_bbox and kpf_track_step_f32.  Run in the
build container only (imports the reference); writes tests/golden/track_bbox.npz = 512 joint sets [21][2] float32 + their frame sizes + the reference's
boxes as float64 + a `valid` byte (0: the reference returned None).

Cases (seeded): hands inside a 640 x 480 and a 1920 x 1080 frame, hands partly outside on every side, wholly outside (left / above: the rule clips them to a
box at the border; right / below: None), coincident joints, a vertical and a horizontal line of joints (zero width or height: None)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

N, J, EXPANSION = 512, 21, 1.5
FRAMES = ((640, 480), (1920, 1080))  # (width, height)


def cases():
    g = np.random.RandomState(20240)
    joints, size, kind = np.zeros((N, J, 2), np.float32), np.zeros((N, 2), np.int32), []
    for i in range(N):
        W, H = FRAMES[i % 2]
        r = g.rand()
        spread = g.uniform(8.0, 0.2 * H, 2)
        if r < 0.62:
            k, c = "inside", np.array([g.uniform(0.25 * W, 0.75 * W), g.uniform(0.25 * H, 0.75 * H)])
        elif r < 0.78:
            k = "partly_outside"
            c = np.array([g.choice([0.0, W - 1.0]), g.uniform(0, H)]) if g.rand() < 0.5 else np.array([g.uniform(0, W), g.choice([0.0, H - 1.0])])
            c = c + g.uniform(-0.5, 0.5, 2) * spread
        elif r < 0.90:
            k = "outside"
            side = g.randint(4)
            c = np.array([g.uniform(0, W), g.uniform(0, H)])
            c[side % 2] = (-2.5 * spread[side % 2] - g.uniform(0, 200)) if side < 2 else ((W, H)[side % 2] + 2.5 * spread[side % 2] + g.uniform(0, 200))
        elif r < 0.94:
            k, c, spread = "coincident", np.array([g.uniform(0, W), g.uniform(0, H)]), np.zeros(2)
        elif r < 0.97:
            k, c, spread = "vertical_line", np.array([g.uniform(0, W), g.uniform(0.25 * H, 0.75 * H)]), spread * np.array([0.0, 1.0])
        else:
            k, c, spread = "horizontal_line", np.array([g.uniform(0.25 * W, 0.75 * W), g.uniform(0, H)]), spread * np.array([1.0, 0.0])
        joints[i] = (c + g.uniform(-1.0, 1.0, (J, 2)) * spread).astype(np.float32)
        size[i] = (W, H)
        kind.append(k)
    return joints, size, kind


def main():
    if not ref_import.reference_available():
        sys.exit("reference tree not found; golden vectors can only be generated in the build container")
    ref_import.load_reference()
    from dataloader.loader import HO3D  # neither method touches self
    joints, size, kind = cases()
    bbox, valid = np.zeros((N, 4), np.float64), np.zeros(N, np.uint8)
    for i in range(N):
        b = HO3D.process_bbox(None, HO3D.get_bbox(None, joints[i], EXPANSION), int(size[i, 0]), int(size[i, 1]), 1.0)
        if b is not None:
            assert b.dtype == np.float64 and b.shape == (4,)
            bbox[i], valid[i] = b, 1
    none = 1.0 - valid.mean()
    for k in sorted(set(kind)):
        sel = np.array([x == k for x in kind])
        print("%-16s %3d cases, %3d None" % (k, sel.sum(), int((valid[sel] == 0).sum())))
    print("None: %.1f %%" % (100 * none))
    assert 0.05 <= none <= 0.20, none
    path = os.path.join(HERE, "track_bbox.npz")
    np.savez_compressed(path, joints=joints, size=size, bbox=bbox, valid=valid, expansion=np.float64(EXPANSION))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
