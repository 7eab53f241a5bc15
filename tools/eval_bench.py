"""What the metrics of the test loop cost beside the forward: `evaluation.evaluate_batch` (six host round trips per batch) against
`evaluation_gpu.DeviceEvaluator.update` (no synchronisation, one transfer at the end), B = 32 at 128 x 128 on the bf16 full model.  Prints one JSON line.

    python tools/eval_bench.py --out profiles/eval_bench.json
    python tools/eval_bench.py --update-only --reps 50      # only update() on synthetic results (the form to run under rocprofv3 --kernel-trace --stats:
                                                            # the launch count of one update is the kernels' call counts / (reps + 5 warm-up calls))

(a) one batch of already-collected results: stream time between two HIP events and host wall time per call, medians over `--runs` runs of `--reps` calls
    (evaluate_batch ends in a host wait by itself; update's wall time is the time to enqueue it, its stream time is taken over back-to-back calls).
(b) batches per second of the `PipelinedEval(depth=2)` loop on `feed_stream`, frames in (`submit_frames`): no metrics / evaluate_batch per batch / update per
    batch and one summary() at the end; host clock around `--batches` batches ending in a device synchronise, the three forms alternating, medians."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # (as bench.py: keypointfusion_amd/graphs.py)

import numpy as np  # noqa: E402

B = 32


def _median_times(fn, reps, runs, torch):
    """(median stream ms per call between two events, median host ms per call) over `runs` runs of `reps` calls; the host time excludes the final wait."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    dev_ms, host_ms = [], []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        host_ms.append((time.perf_counter() - t0) / reps * 1e3)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(dev_ms), statistics.median(host_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--batches", type=int, default=200, help="batches per timed loop of (b)")
    ap.add_argument("--update-only", action="store_true", help="skip the model: update() on synthetic results, reps calls after 5 warm-up calls")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    from keypointfusion_amd import evaluation as EV
    from keypointfusion_amd.evaluation_gpu import DeviceEvaluator
    from keypointfusion_amd.weights import synthetic_batch
    dev = torch.device("cuda:0")
    rec = {"tool": "eval_bench", "B": B, "reps": args.reps, "runs": args.runs}
    g = torch.Generator().manual_seed(0)
    gt = (0.3 * torch.randn(B, 21, 3, generator=g)).to(dev)
    ev = DeviceEvaluator()
    stream = torch.cuda.Stream(device=dev)

    if args.update_only:
        sb = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_batch(B, 128, seed=1).items()}
        res = [torch.randn(B, 105, 32, 32, generator=g).to(dev) for _ in range(2)] + [(gt.cpu() + 0.05 * torch.randn(B, 21, 3, generator=g)).to(dev) for _ in range(4)]
        with torch.no_grad(), torch.cuda.stream(stream):
            d, h = _median_times(lambda: ev.update(res, sb["img"], gt, sb["center"], sb["M"], sb["cube"], sb["cam_para"]), args.reps, 1, torch)
            rec.update(update_stream_ms=d, update_enqueue_ms=h, samples=ev.summary()[0]["samples"])
    else:
        import prep_cases as PC
        from conftest import synthetic_sd
        from keypointfusion_amd.model.model import KPFusion
        from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
        from keypointfusion_amd.serving import PipelinedEval
        names = list(PC.CASES)
        fr = [PC.synth_frame(names[i % len(names)], seed=1 + i) for i in range(B)]
        t = lambda a: torch.from_numpy(a).to(dev)
        frames = (t(np.stack([f[0] for f in fr])), t(np.stack([f[1] for f in fr])), t(np.array([f[2] for f in fr], np.float64)),
                  t(np.array([f[3] for f in fr], np.float64)), torch.arange(B, dtype=torch.int64, device=dev))
        net = "KPFusion-convnext-tiny"
        m = KPFusion(net, "", 21, "dexycb", "")
        m.load_state_dict(synthetic_sd(net))
        m.precision = "bf16"
        m = m.to(dev).eval()
        pre = DevicePreprocessor()
        pe = PipelinedEval(m, depth=2)

        def loop(metrics, n):
            """n batches, two in flight; metrics(results, prep) after every collect.  Returns batches per second."""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pending = []
            for i in range(n + 1):
                if i < n:
                    pending.append(pe.submit_frames(pre, *frames))
                if len(pending) == 2 or i == n:
                    ticket, prep = pending.pop(0)
                    res, _, _ = pe.collect(ticket)
                    if metrics is not None:
                        metrics(res, prep)
            if metrics is update:
                ev.summary()
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        def host_metrics(res, p):
            EV.evaluate_batch(res, p["img"], gt, p["center"], p["M"], p["cube"], p["cam_para"])

        def update(res, p):
            ev.update(res, p["img"], gt, p["center"], p["M"], p["cube"], p["cam_para"])

        with torch.no_grad(), torch.cuda.stream(pe.feed_stream(dev)):
            for f in (None, host_metrics, update):  # warm-up of every form: graphs captured, buffers allocated, solver loaded
                loop(f, 6)
            # (a) on one collected batch
            ticket, p = pe.submit_frames(pre, *frames)
            res, _, _ = pe.collect(ticket)
            torch.cuda.synchronize()
            d, h = _median_times(lambda: host_metrics(res, p), args.reps, args.runs, torch)
            rec.update(evaluate_batch_stream_ms=d, evaluate_batch_wall_ms=h)
            d, h = _median_times(lambda: update(res, p), args.reps, args.runs, torch)
            rec.update(update_stream_ms=d, update_enqueue_ms=h)
            # (b) the pipelined loop, forms alternating
            ev.reset()
            rates = {"none": [], "evaluate_batch": [], "update": []}
            for _ in range(args.runs):
                for name, f in (("none", None), ("evaluate_batch", host_metrics), ("update", update)):
                    if f is update:
                        ev.reset()
                    rates[name].append(loop(f, args.batches))
            for name, r in rates.items():
                rec["loop_batches_per_s_" + name] = statistics.median(r)
                rec["loop_batches_per_s_" + name + "_min_max"] = [min(r), max(r)]
            rec["loop_ms_per_batch"] = {k: 1e3 / statistics.median(r) for k, r in rates.items()}
            rec["loop_update_vs_none"] = rec["loop_batches_per_s_update"] / rec["loop_batches_per_s_none"]
            rec["loop_evaluate_batch_vs_none"] = rec["loop_batches_per_s_evaluate_batch"] / rec["loop_batches_per_s_none"]
            s = ev.summary()
            rec.update(batches=args.batches, summary_samples=s[0]["samples"], summary_final_mean_error_mm=s[5]["mean_error"])
    torch.cuda.synchronize()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
