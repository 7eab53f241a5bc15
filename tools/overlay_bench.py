"""Timing of the on-device overlay (keypointfusion_amd/overlay.py::FrameOverlay.draw: kpf_overlay_project_f32 + kpf_overlay_draw_u8), eager
and replayed from a captured graph, at 480 x 640 and at 1080 x 1920 with B = 2 hands on ONE stored frame, beside TrackedStream.step of the same build at
B = 2 (graphed) -- the comparison: what drawing the result adds to a tracked frame.  Prints one JSON line and writes it to profiles/overlay_bench.json (--out).

    python tools/overlay_bench.py
    python tools/overlay_bench.py --reps 50

The hands are the surface model's first two poses (tests/mano_raster_cases.py), the second shifted so that the two overlap in the picture; the camera is
scaled with the frame so that a hand covers the same share of it; the 21 "joints" are every 37th vertex projected by the camera (the skeleton's load, not
its anatomy); the depth frame is a constant 2 m, behind both hands, so that the occlusion test runs and hides nothing.  Times are host clocks around `reps`
calls that end in one device synchronise, after a warm-up, tools/track_bench.py's discipline.  No figure here is a pass bar."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # (as bench.py: keypointfusion_amd/graphs.py)

import numpy as np  # noqa: E402


def _timed(fn, reps, torch):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _overlay_records(rec, dev, reps, torch):
    import mano_raster_cases as R
    import mano_surface_cases as S
    from keypointfusion_amd.mano_fit import ManoFitter
    from keypointfusion_amd.overlay import FrameOverlay

    fitter = ManoFitter(S.surface_sd(), dev)
    verts = R.hands()[:2].copy()
    verts[1] += np.asarray([40.0, 25.0, -50.0], np.float32)
    rng = np.random.Generator(np.random.PCG64(7))
    for H, W in ((480, 640), (1080, 1920)):
        k = H / 480.0
        cam = np.tile(np.asarray([475.0 * k, 475.0 * k, W / 2.0, H / 2.0], np.float32), (2, 1))
        picked = verts[:, ::37][:, :21]
        jp = np.stack([picked[..., 0] * cam[:, None, 0] / picked[..., 2] + cam[:, None, 2], picked[..., 1] * cam[:, None, 1] / picked[..., 2] + cam[:, None, 3],
                       picked[..., 2]], -1).astype(np.float32)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        rgb, depth = d(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)), d(np.full((1, H, W), 2000, np.uint16))
        vd, cd, jd, status = d(verts), d(cam), d(jp), torch.zeros(2, dtype=torch.int32, device=dev)
        nd = fitter.normals(vd).clone()
        ov = FrameOverlay(fitter, dev, (H, W), 1, frame_index=[0, 0])
        run = lambda: ov.draw(rgb, vd, cd, nd, jd, status, depth)  # noqa: E731
        tag = "%dx%d" % (H, W)
        rec["draw_eager_ms_" + tag] = _timed(run, reps, torch)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run()
        rec["draw_graph_ms_" + tag] = _timed(g.replay, reps, torch)
        torch.cuda.synchronize()
        label = out["label"].cpu().numpy()
        rec["pixels_" + tag] = {"mesh": int((label == 1).sum()), "bone": int((label == 2).sum()), "joint": int((label == 3).sum()), "hidden": int((label == 4).sum())}


def _tracked_record(rec, dev, reps, torch):
    import prep_cases as PC
    from conftest import synthetic_sd
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
    ts = TrackedStream(m, DevicePreprocessor(), cam, frame_size=(480, 640), frames=1, frame_index=[0, 0], graph=True)
    ts.reseed(bbox)
    for _ in range(3):  # the two eager frames and the capture
        ts.step(rgb, depth)
    rec["tracked_graph_ms_B2_480x640"] = _timed(lambda: ts.step(rgb, depth), reps, torch)
    rec["net"] = net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.json"))
    args = ap.parse_args()

    import torch

    dev = torch.device("cuda:0")
    rec = {"tool": "overlay_bench", "hands": 2, "frames": 1, "reps": args.reps}
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(stream):
        _overlay_records(rec, dev, args.reps, torch)
        _tracked_record(rec, dev, args.reps, torch)
    torch.cuda.synchronize()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
