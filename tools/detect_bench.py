"""Timing of the on-device hand detector (keypointfusion_amd/detect.py::HandDetector.detect and .assign: the six launches of kpf_detect_hands_u16 and the one
of kpf_detect_assign_f64), eager and replayed from a captured graph, on one 480 x 640 and one 1080 x 1920 registered depth frame, beside
TrackedStream.step of the same build at B = 2 (graphed), without and with the detector inside the captured step -- the comparison: what finding the hands
adds to a tracked frame.  Prints one JSON line and writes it to profiles/detect_bench.json (--out).

    python tools/detect_bench.py
    python tools/detect_bench.py --reps 50 --detect-reps 500

The frame is a wall at 1.2 m that fills the picture (one component of every pixel, refused by the area gate: the labelling's and the statistics' full
load), with two hands of ripple and noise in front of it and a scatter of single-pixel speckle; the 1080 x 1920 frame is the same scene at 2.25 times the
focal length.  Times are host clocks around `reps` calls that end in one device synchronise, after a warm-up, tools/align_bench.py's discipline.  No figure
here is a pass bar."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # (as bench.py: keypointfusion_amd/graphs.py)


def _timed(fn, reps, torch):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def scene(size, np):
    """(depth [1][H][W] uint16, cam [1][4] float32): a wall, two hands, speckle"""
    H, W = size
    s = H / 480.0
    g = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (1200 + 4 * np.sin(xx / (9.0 * s))).astype(np.int64)
    for cx, cy, z, r in ((200.0, 240.0, 600.0, 60.0), (450.0, 200.0, 700.0, 45.0)):
        m = (xx - cx * s) ** 2 + (yy - cy * s) ** 2 < (r * s) ** 2
        depth[m] = (z + 30 * np.sin(xx[m] / (7.0 * s)) + g.randint(-5, 6, int(m.sum()))).astype(np.int64)
    speck = g.rand(H, W) < 0.002
    depth[speck] = 300
    return depth.astype(np.uint16)[None], np.array([[600.0 * s, 600.0 * s, W / 2.0, H / 2.0]], np.float32)


def _detect_records(rec, dev, reps, torch, np):
    from keypointfusion_amd.detect import STAT_NAMES, HandDetector
    from keypointfusion_amd.preprocess_gpu import make_frame_index

    for size in ((480, 640), (1080, 1920)):
        depth_h, cam = scene(size, np)
        depth = torch.from_numpy(depth_h).to(dev)
        det = HandDetector(cam, size, dev)
        fi = make_frame_index([0, 0], 1, dev)
        bbox, lost = torch.zeros(2, 4, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        seeded, reseeded = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        tag = "%dx%d" % size
        for name, run in (("detect", lambda: det.detect(depth)), ("assign", lambda: det.assign(fi, bbox, lost, seeded, reseeded, 3))):
            rec["%s_eager_ms_%s" % (name, tag)] = _timed(run, reps, torch)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run()
            rec["%s_graph_ms_%s" % (name, tag)] = _timed(g.replay, reps, torch)
            torch.cuda.synchronize()
        rec["stats_" + tag] = dict(zip(STAT_NAMES, det.stats.cpu().numpy()[0].tolist()))
        rec["scratch_MiB_" + tag] = round((det._ws32.numel() * 4 + det._ws64.numel() * 8) / 2.0 ** 20, 1)


def _tracked_records(rec, dev, reps, torch, np):
    import prep_cases as PC
    from conftest import synthetic_sd
    from keypointfusion_amd.detect import HandDetector
    from keypointfusion_amd.model.model import KPFusion
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    from keypointfusion_amd.tracking import TrackedStream

    net = "KPFusion-convnext-tiny"
    m = KPFusion(net, "", 21, "dexycb", "")
    m.load_state_dict(synthetic_sd(net))
    m = m.to(dev).eval()
    rgb1, depth1, bbox1, cam1 = PC.synth_frame("centre")
    rgb, depth = torch.from_numpy(rgb1[None].copy()).to(dev), torch.from_numpy(depth1[None].copy()).to(dev)
    bbox = torch.tensor([bbox1] * 2, dtype=torch.float64, device=dev)
    cam = torch.tensor([cam1] * 2, dtype=torch.float64, device=dev)
    for tag, detector in (("tracked_graph_ms_B2_480x640", None),
                          ("tracked_detect_graph_ms_B2_480x640", HandDetector(np.asarray([cam1], np.float32), (480, 640), dev))):
        ts = TrackedStream(m, DevicePreprocessor(), cam, frame_size=(480, 640), frames=1, frame_index=[0, 0], graph=True, detector=detector)
        ts.reseed(bbox)
        for _ in range(3):  # the two eager frames and the capture
            ts.step(rgb, depth)
        rec[tag] = _timed(lambda: ts.step(rgb, depth), reps, torch)
    rec["net"] = net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--detect-reps", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    dev = torch.device("cuda:0")
    rec = {"tool": "detect_bench", "frames": 1, "reps": args.reps, "detect_reps": args.detect_reps}
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(stream):
        _detect_records(rec, dev, args.detect_reps, torch, np)
        _tracked_records(rec, dev, args.reps, torch, np)
    torch.cuda.synchronize()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
