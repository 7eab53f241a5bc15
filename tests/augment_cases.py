"""Shared by tests/test_prep_augment_host.py and tests/test_prep_augment_gpu.py: augmentation draws for the frames of tests/annot_cases.py and the host
record (preprocess.prepare_augmented plus the integer record and all candidate points) that the device path is compared with."""
import numpy as np

import annot_cases as AC
from keypointfusion_amd import preprocess as P


def draw(g, mode, color=False):
    """One augmentation record in the reference's ranges (sigma_com 10 mm, sigma_sc 0.2, +-180 degrees) from RandomState g, with the mode given."""
    rot = float(g.uniform(-180, 180))
    aug = dict(mode=int(mode), off=g.uniform(-1, 1, 3) * 10.0, rot=rot, sc=float(abs(1.0 + g.uniform(-1, 1) * 0.2)), rot_cs=P._rot_cs(rot))
    if color:
        aug["color"] = g.uniform(0.8, 1.2, 3)
    return aug


def host_record(ins, aug, img_size=128, sample_num=1024):
    """ins: annot_cases.synth()'s tuple.  prepare_augmented plus bounds / sz of the BASE crop and every candidate point of the augmented one."""
    rgb, depth, joints_mm, cam, mirror, center = ins
    out = P.prepare_augmented(rgb, depth, joints_mm, cam, aug, mirror, center, AC.CUBE, img_size, sample_num)
    base = AC.host_record(rgb, depth, joints_mm, cam, mirror, center, img_size, sample_num)
    cand = P.depth_to_pcl(out["img"][0], out["center"], out["cube64"], out["M64"], tuple(float(c) for c in cam))
    out.update(bounds=base["bounds"], sz=base["sz"], candidates=np.clip(cand, -1, 1).astype(np.float32).reshape(-1, 3), base=base)
    return out


def stack(augs):
    """A list of records -> the arrays of a batch (color: ones where a record has none; None when no record has one)."""
    out = dict(mode=np.array([a["mode"] for a in augs], np.int32), off=np.stack([np.asarray(a["off"], np.float64) for a in augs]),
               sc=np.array([a["sc"] for a in augs], np.float64), rot=np.array([a["rot"] for a in augs], np.float64),
               rot_cs=np.array([a["rot_cs"] for a in augs], np.float64))
    if any(a.get("color") is not None for a in augs):
        out["color"] = np.stack([np.ones(3) if a.get("color") is None else np.asarray(a["color"], np.float64) for a in augs])
    return out
