"""Timing of the preprocessing stage in front of the forward: host `preprocess.prepare_rgbd` (one core, and a pool of 16 processes) against the device
`preprocess_gpu.DevicePreprocessor.prepare` of a B = 32 batch (640 x 480 frames, and a 512 x 512 window of a 1920 x 1080 frame), beside the B = 32 bf16
forward of the same build.  Prints one JSON line.

    python tools/prep_bench.py                      # everything
    python tools/prep_bench.py --device-only --reps 50   # only the three kpf_prep_* kernels (the form to run under rocprofv3 --kernel-trace --stats)
    python tools/prep_bench.py --annotated          # only: prepare_annotated (the dataset protocol) beside prepare on the same B = 32 frames;
                                                    # writes profiles/prep_annot_bench.json (--out: elsewhere)
    python tools/prep_bench.py --augmented          # only: prepare_augmented with parameters drawn on the device (training augmentation) beside
                                                    # prepare_annotated on the same B = 32 frames; writes profiles/prep_augment_bench.json (--out: elsewhere)

Times are host clocks around work that ends in a device synchronise (enqueue of `reps` batches, one synchronise), after a warm-up of every shape."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # (as bench.py: keypointfusion_amd/graphs.py)

import numpy as np  # noqa: E402

B = 32


def _frames():
    import prep_cases as PC
    names = list(PC.CASES)
    return [PC.synth_frame(names[i % len(names)], seed=1 + i) for i in range(B)]


def _host_one(k):
    from keypointfusion_amd import preprocess as P
    frames = _frames()[:8]
    t0 = time.perf_counter()
    for i in range(k):
        rgb, depth, bbox, cam = frames[i % len(frames)]
        P.prepare_rgbd(rgb, depth, bbox, cam)
    return time.perf_counter() - t0


def host_times(per_proc=40, procs=16):
    _host_one(4)  # warm-up (imports, page faults)
    single = _host_one(per_proc) / per_proc
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_host_one, [4] * procs)
        wall = max(pool.map(_host_one, [per_proc] * procs))  # the workers time their own loops (frame generation excluded); they run side by side
    return single, wall / (per_proc * procs)


def _timed(fn, reps, torch):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def annotated(args):
    """prepare_annotated beside prepare: the frames of tests/annot_cases.py (mixed, a third of them left hands), each also given the box of its joints
    (the rule of tracking.next_bbox's get_bbox, 1.5 x) for prepare, eagerly and replayed from a graph."""
    import torch
    import annot_cases as AC
    from keypointfusion_amd import preprocess as P
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    dev = torch.device("cuda:0")
    items = [AC.synth(AC.SMALL[i % len(AC.SMALL)], seed=1 + i) for i in range(B)]
    bbox = []
    for rgb, depth, joints_mm, cam, mirror, center in items:
        uv = P._project_f32(joints_mm, cam)[:, :2].astype(np.float64)
        lo, hi = uv.min(0), uv.max(0)
        c, w = (lo + hi) / 2, (hi - lo) * 1.5
        bbox.append([c[0] - w[0] / 2, c[1] - w[1] / 2, w[0], w[1]])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rgb, depth = t(np.stack([i[0] for i in items])), t(np.stack([i[1] for i in items]))
    joints, cam32 = t(np.stack([i[2] for i in items])), t(np.stack([i[3] for i in items]))
    mirror = t(np.array([i[4] for i in items], np.uint8))
    seed = torch.arange(B, dtype=torch.int64, device=dev)
    box_in = (rgb, depth, t(np.array(bbox, np.float64)), cam32.double(), seed)
    pre = DevicePreprocessor(cube=AC.CUBE)
    rec = {"tool": "prep_bench --annotated", "B": B, "reps": args.reps, "frames": "640x480", "left_hands": int(mirror.sum())}
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(stream):
        run_a = lambda: pre.prepare_annotated(rgb, depth, joints, cam32, seed, mirror=mirror)
        run_b = lambda: pre.prepare(*box_in)
        graphs = []
        for fn in (run_b, run_a):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            graphs.append(graph)
        # the two forms alternate, three rounds each, so that a drift of the box shows as spread and not as a difference
        names = ("prepare_ms", "prepare_annotated_ms", "prepare_graph_ms", "prepare_annotated_graph_ms")
        rounds = {k: [] for k in names}
        for _ in range(3):
            for k, fn in zip(names, (run_b, run_a, graphs[0].replay, graphs[1].replay)):
                rounds[k].append(_timed(fn, args.reps, torch) * 1e3)
        for k in names:
            rec[k], rec[k + "_rounds"] = float(np.median(rounds[k])), rounds[k]
        rec["pcl_count_mean_prepare"] = float(run_b()["pcl_count"].float().mean())
        rec["pcl_count_mean_annotated"] = float(run_a()["pcl_count"].float().mean())
    torch.cuda.synchronize()
    rec["annotated_no_slower_than_prepare"] = bool(rec["prepare_annotated_graph_ms"] <= rec["prepare_graph_ms"])
    line = json.dumps(rec)
    print(line, flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "prep_annot_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


def augmented(args):
    """prepare_augmented (draw + crop + sample, the parameters drawn on the device, so every replay sees a fresh mix of the four modes) beside
    prepare_annotated on the frames of tests/annot_cases.py, eagerly and replayed from a graph, alternating as annotated() does."""
    import torch
    import annot_cases as AC
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    dev = torch.device("cuda:0")
    items = [AC.synth(AC.SMALL[i % len(AC.SMALL)], seed=1 + i) for i in range(B)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rgb, depth = t(np.stack([i[0] for i in items])), t(np.stack([i[1] for i in items]))
    joints, cam32 = t(np.stack([i[2] for i in items])), t(np.stack([i[3] for i in items]))
    mirror = t(np.array([i[4] for i in items], np.uint8))
    seed, seed_aug = torch.arange(B, dtype=torch.int64, device=dev), torch.arange(B, dtype=torch.int64, device=dev)
    pre = DevicePreprocessor(cube=AC.CUBE)
    rec = {"tool": "prep_bench --augmented", "B": B, "reps": args.reps, "frames": "640x480", "left_hands": int(mirror.sum()), "color_factor": 0.2}
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(stream):
        run_a = lambda: pre.prepare_annotated(rgb, depth, joints, cam32, seed, mirror=mirror)
        run_g = lambda: pre.prepare_augmented(rgb, depth, joints, cam32, seed_aug, mirror=mirror, color_factor=0.2)
        graphs = []
        for fn in (run_a, run_g):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            graphs.append(graph)
        names = ("prepare_annotated_ms", "prepare_augmented_ms", "prepare_annotated_graph_ms", "prepare_augmented_graph_ms")
        rounds = {k: [] for k in names}
        for _ in range(3):
            for k, fn in zip(names, (run_a, run_g, graphs[0].replay, graphs[1].replay)):
                rounds[k].append(_timed(fn, args.reps, torch) * 1e3)
        for k in names:
            rec[k], rec[k + "_rounds"] = float(np.median(rounds[k])), rounds[k]
        out = run_g()
        rec["pcl_count_mean_augmented"] = float(out["pcl_count"].float().mean())
        rec["modes_of_the_last_batch"] = torch.bincount(out["aug"]["mode"].long(), minlength=4).tolist()
        rec["refused"] = int((out["aug_status"] & 2).ne(0).sum())
    torch.cuda.synchronize()
    rec["augmented_over_annotated_graph"] = rec["prepare_augmented_graph_ms"] / rec["prepare_annotated_graph_ms"]
    line = json.dumps(rec)
    print(line, flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "prep_augment_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--device-only", action="store_true", help="skip the host path and the model: only prepare() and uncrop() of the two input forms")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    ap.add_argument("--annotated", action="store_true", help="only: prepare_annotated beside prepare on the same frames; writes profiles/prep_annot_bench.json")
    ap.add_argument("--augmented", action="store_true", help="only: prepare_augmented (drawn parameters) beside prepare_annotated; writes profiles/prep_augment_bench.json")
    args = ap.parse_args()
    if args.annotated:
        return annotated(args)
    if args.augmented:
        return augmented(args)
    rec = {"tool": "prep_bench", "B": B, "reps": args.reps}
    if not args.device_only:  # before the GPU is initialised: the pool forks
        single, pooled = host_times()
        rec.update(host_ms_per_image_1core=single * 1e3, host_ms_per_image_16proc=pooled * 1e3, host_img_per_s_16proc=1.0 / pooled)

    import torch
    from keypointfusion_amd.preprocess_gpu import MODEL_INPUTS, DevicePreprocessor
    dev = torch.device("cuda:0")
    fr = _frames()
    rgb, depth = np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])
    bbox, cam = np.array([f[2] for f in fr], np.float64), np.array([f[3] for f in fr], np.float64)
    # the same content as a 512 x 512 window of a 1920 x 1080 frame: the frame's left 512 columns at (704, 284), boxes shifted with it
    x0, y0 = 704, 284
    rgbw, depthw = np.zeros((B, 512, 512, 3), np.uint8), np.zeros((B, 512, 512), np.uint16)
    rgbw[:, :480], depthw[:, :480] = rgb[:, :, :512], depth[:, :, :512]
    bboxw, camw = bbox + np.array([x0, y0, 0, 0], np.float64), cam + np.array([0, 0, x0, y0], np.float64)
    t = lambda a: torch.from_numpy(a).to(dev)
    seed = torch.arange(B, dtype=torch.int64, device=dev)
    full_in, win_in = (t(rgb), t(depth), t(bbox), t(cam), seed), (t(rgbw), t(depthw), t(bboxw), t(camw), seed)
    pre = DevicePreprocessor()
    joints = torch.zeros(B, 21, 3, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(stream):
        rec["device_prepare_ms_640x480"] = _timed(lambda: pre.prepare(*full_in), args.reps, torch) * 1e3
        rec["device_prepare_ms_window512_of_1920x1080"] = _timed(lambda: pre.prepare(*win_in, origin=(x0, y0), frame_size=(1080, 1920)), args.reps, torch) * 1e3
        prep = pre.prepare(*full_in)
        rec["device_uncrop_ms"] = _timed(lambda: pre.uncrop(joints, prep), args.reps, torch) * 1e3
        rec["pcl_count_mean"] = float(prep["pcl_count"].float().mean())
        # the same launches replayed from a captured graph (what a server that captures prepare + forward pays)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pre.prepare(*full_in)
        rec["device_prepare_graph_ms_640x480"] = _timed(graph.replay, args.reps, torch) * 1e3
        rec["device_prepare_us_per_image_640x480"] = rec["device_prepare_graph_ms_640x480"] * 1e3 / B
        if not args.device_only:
            from conftest import synthetic_sd
            from keypointfusion_amd.model.model import KPFusion
            from keypointfusion_amd.serving import PipelinedEval
            net = "KPFusion-convnext-tiny"
            m = KPFusion(net, "", 21, "dexycb", "")
            m.load_state_dict(synthetic_sd(net))
            m.precision = "bf16"
            m = m.to(dev).eval()
            plan = m._plan(dev)
            ins = [prep[k].clone() for k in MODEL_INPUTS]
            rec["forward_bf16_ms_one_in_flight"] = _timed(lambda: plan.forward_graphed(*ins, 0.8, 128, 1), 30, torch) * 1e3
            pe = PipelinedEval(m, depth=2)
            rec["forward_bf16_ms_two_in_flight"] = _timed(lambda: pe.submit(*ins[:3], None, *ins[3:]), 30, torch) * 1e3
            rec["prepare_plus_forward_ms_two_in_flight"] = _timed(lambda: pe.submit_frames(pre, *full_in), 30, torch) * 1e3
            rec["forward_img_per_s_two_in_flight"] = B / (rec["forward_bf16_ms_two_in_flight"] * 1e-3)
            fastest_forward = min(rec["forward_bf16_ms_one_in_flight"], rec["forward_bf16_ms_two_in_flight"])
            rec["prepare_faster_than_forward"] = bool(rec["device_prepare_ms_640x480"] < fastest_forward)
            rec["prepare_faster_than_host_pool"] = bool(rec["device_prepare_ms_640x480"] / B < rec["host_ms_per_image_16proc"])
    torch.cuda.synchronize()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
