"""Timing of the tracked video loop (keypointfusion_amd/tracking.py::TrackedStream: prepare -> forward -> kpf_track_step_f32, the next box staying on the
device) at B = 1 and B = 32 tracks, graphed and eager, beside the existing UNTRACKED prepare + forward + uncrop graph of the same build (the boxes of every
frame given from outside: tests/test_preprocess_gpu.py::test_prepare_and_forward_in_one_graph) — the comparison: what the tracking step adds to a frame.
Prints one JSON line and writes it to profiles/track_bench.json (--out).

    python tools/track_bench.py                 # fp32 ConvNeXt-T, synthetic weights, 640 x 480 frames
    python tools/track_bench.py --reps 50

Every track has its own stored frame (F = B) so that both loops read the same bytes.  Times are host clocks around `reps` frames that end in one device
synchronise, after a warm-up; a tracked frame includes the copy of the frames into the stream's static buffers.  No figure here is a pass bar."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    args = ap.parse_args()

    import torch
    import prep_cases as PC
    from conftest import synthetic_sd
    from keypointfusion_amd.model.model import KPFusion
    from keypointfusion_amd.preprocess_gpu import MODEL_INPUTS, DevicePreprocessor
    from keypointfusion_amd.tracking import TrackedStream

    dev = torch.device("cuda:0")
    net = "KPFusion-convnext-tiny"
    m = KPFusion(net, "", 21, "dexycb", "")
    m.load_state_dict(synthetic_sd(net))
    m = m.to(dev).eval()
    plan = m._plan(dev)
    rgb1, depth1, bbox1, cam1 = PC.synth_frame("centre")
    rec = {"tool": "track_bench", "net": net, "precision": "fp32", "frame": [480, 640], "reps": args.reps}
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(stream):
        for B in (1, 32):
            rgb = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(rgb1, (B,) + rgb1.shape))).to(dev)
            depth = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(depth1, (B,) + depth1.shape))).to(dev)
            bbox = torch.tensor([bbox1] * B, dtype=torch.float64, device=dev)
            cam = torch.tensor([cam1] * B, dtype=torch.float64, device=dev)
            for graph in (True, False):
                ts = TrackedStream(m, DevicePreprocessor(), cam, frame_size=(480, 640), frames=B, graph=graph)
                ts.reseed(bbox)
                for _ in range(3):  # the two eager frames and the capture
                    ts.step(rgb, depth)
                rec["tracked_%s_ms_B%d" % ("graph" if graph else "eager", B)] = _timed(lambda: ts.step(rgb, depth), args.reps, torch)
                torch.cuda.synchronize()
                rec["tracked_lost_max_B%d" % B] = int(ts.lost.max())  # (untrained weights: whether the box survives says nothing about the kernel)
            # the untracked loop: boxes from outside, prepare + forward + uncrop in one graph, frames copied into its static inputs every frame
            pre = DevicePreprocessor()
            seed = torch.arange(B, dtype=torch.int64, device=dev)
            static = [rgb.clone(), depth.clone(), bbox.clone(), cam.clone(), seed.clone()]

            def run():
                prep = pre.prepare(*static)
                res, _, _ = plan.forward(*[prep[k] for k in MODEL_INPUTS], 0.8, 128, 1)
                return pre.uncrop(res[5], prep)

            rec["untracked_eager_ms_B%d" % B] = _timed(run, args.reps, torch)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run()

            def replay():
                static[0].copy_(rgb)
                static[1].copy_(depth)
                g.replay()

            rec["untracked_graph_ms_B%d" % B] = _timed(replay, args.reps, torch)
            rec["tracking_adds_ms_graph_B%d" % B] = rec["tracked_graph_ms_B%d" % B] - rec["untracked_graph_ms_B%d" % B]
    torch.cuda.synchronize()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
