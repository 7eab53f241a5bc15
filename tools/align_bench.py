"""Timing of the on-device depth registration (keypointfusion_amd/sensor.py::DepthAligner.align: the three launches of kpf_align_depth_u16),
eager and replayed from a captured graph, with one 480 x 640 raw frame registered to a 480 x 640 and to a 1080 x 1920 colour grid, beside TrackedStream.step
of the same build at B = 2 (graphed), without and with the aligner inside the captured step -- the comparison: what registering the depth adds to a tracked
frame.  Prints one JSON line and writes it to profiles/align_bench.json (--out).

    python tools/align_bench.py
    python tools/align_bench.py --reps 50 --align-reps 2000

The raw frame is a tilted plane with a near block and holes (tests/align_cases.py), every pixel but the holes measured, which is the scatter launch's
full load; the depth camera is turned by 0.01 and 0.005 rad and stands 15 mm beside the colour camera.  Times are host clocks around `reps` calls that
end in one device synchronise, after a warm-up, tools/track_bench.py's discipline; an align call is tens of microseconds, so it is repeated --align-reps
times (default 5000) for a window of a tenth of a second or more.  No figure here is a pass bar."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # (as bench.py: keypointfusion_amd/graphs.py)


RAW = (480, 640)


def _timed(fn, reps, torch):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _calib(out_size):
    import align_cases as AC
    from keypointfusion_amd.sensor import make_calib
    Kd = AC.intrinsics(RAW)
    return make_calib(Kd, AC.scaled(Kd, out_size[0] / RAW[0]), AC.rot(0.01, 0.005), AC.T_MM)


def _align_records(rec, dev, reps, torch):
    import align_cases as AC
    from keypointfusion_amd.sensor import DepthAligner

    raw = torch.from_numpy(AC.scene("block", RAW)[None].copy()).to(dev)
    for out_size in ((480, 640), (1080, 1920)):
        al = DepthAligner(_calib(out_size), RAW, out_size, dev)
        run = lambda: al.align(raw)  # noqa: E731
        tag = "%dx%d" % out_size
        rec["align_eager_ms_" + tag] = _timed(run, reps, torch)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run()
        rec["align_graph_ms_" + tag] = _timed(g.replay, reps, torch)
        torch.cuda.synchronize()
        rec["stats_" + tag] = dict(zip(("valid", "skipped", "too_large", "covered", "filled"), out["stats"].cpu().numpy()[0].tolist()))


def _tracked_records(rec, dev, reps, torch):
    import prep_cases as PC
    from conftest import synthetic_sd
    from keypointfusion_amd.model.model import KPFusion
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    from keypointfusion_amd.sensor import DepthAligner, make_calib
    from keypointfusion_amd.tracking import TrackedStream

    net = "KPFusion-convnext-tiny"
    m = KPFusion(net, "", 21, "dexycb", "")
    m.load_state_dict(synthetic_sd(net))
    m = m.to(dev).eval()
    rgb1, depth1, bbox1, cam1 = PC.synth_frame("centre")
    rgb, depth = torch.from_numpy(rgb1[None].copy()).to(dev), torch.from_numpy(depth1[None].copy()).to(dev)
    bbox = torch.tensor([bbox1] * 2, dtype=torch.float64, device=dev)
    cam = torch.tensor([cam1] * 2, dtype=torch.float64, device=dev)
    for tag, aligner in (("tracked_graph_ms_B2_480x640", None),  # the same camera on both sides: the disc stays under the box
                         ("tracked_aligned_graph_ms_B2_480x640", DepthAligner(make_calib(cam1, cam1), RAW, RAW, dev))):
        ts = TrackedStream(m, DevicePreprocessor(), cam, frame_size=RAW, frames=1, frame_index=[0, 0], graph=True, aligner=aligner)
        ts.reseed(bbox)
        for _ in range(3):  # the two eager frames and the capture
            ts.step(rgb, depth)
        rec[tag] = _timed(lambda: ts.step(rgb, depth), reps, torch)
    rec["net"] = net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--align-reps", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    args = ap.parse_args()

    import torch

    dev = torch.device("cuda:0")
    rec = {"tool": "align_bench", "raw": "%dx%d" % RAW, "frames": 1, "reps": args.reps, "align_reps": args.align_reps}
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(stream):
        _align_records(rec, dev, args.align_reps, torch)
        _tracked_records(rec, dev, args.reps, torch)
    torch.cuda.synchronize()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
