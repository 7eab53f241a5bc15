"""Timing of the MANO layer in HIP: the MANO head's train step (forward + backward to the features and the MLP's parameters) at B = 32 with the
hand model as torch ops under autograd (layer="torch") against heads_train.ManoLayerHip (layer="hip"), and the joint fit mano_fit.ManoFitter at B = 1 and 32
with iters = 10 and 50; the Gauss-Newton fit fit_gn at B = 1 and 32 -- ms per call at its default 8 iterations, at 1 and 0, ms per
iteration = (8 - 1) / 7, the residual and history after, Adam's 10 / 50-iteration figures of the same run beside them (records fit_gn_B1, fit_gn_B32); and the fit with a vertex term, the association of 1024 points and the chain fit_cloud (3 rounds) at B = 1 and 32
with iters = 50; the Gauss-Newton mesh fit fit_mesh_gn at 0, 1, 2 and 8 iterations and the chain with six Gauss-Newton rounds of two
iterations, Adam's figures of the same run beside them (records fit_mesh_gn_B1 / _B32, fit_cloud_gn_B1 / _B32); the vertex normals, the
association over the camera-facing vertices and the chain with point-to-plane rounds (records normals_B1 / _B32, assoc_vis_B1 / _B32,
fit_cloud_plane_B1 / _B32, beside fit_cloud_gn_* of the same run); the z-buffer render at 128 x 128 and 32 x 32, with and without an
observed depth crop, and the chain with the render's mask on the association (records raster_B1 / _B32, fit_cloud_zbuf_B1 / _B32, beside
fit_cloud_plane_* of the same run); the silhouette of an observed crop, the free-space term and the plane chain with it (records
silhouette_B1 / _B32, free_space_B1 / _B32, fit_cloud_free_B1 / _B32, beside fit_cloud_plane_* of the same run); the mesh evaluation evaluation_mesh_gpu.DeviceMeshEvaluator.update at V = 778 and beside it the same
figures as torch ops on the device with one .cpu() per batch (records mesh_eval_B1 / _B32).  Prints one JSON line and writes it to profiles/mano_bench.json (--out).

    python tools/mano_bench.py
    python tools/mano_bench.py --reps 50

Synthetic hand model and weights.  Times are host clocks around `reps` calls that end in one device synchronise, after a warm-up.  No figure here is a pass bar."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mano_bench.json"))
    args = ap.parse_args()

    import torch
    from keypointfusion_amd.heads_train import mano_head_train_forward
    from keypointfusion_amd.mano_fit import ManoFitter
    from keypointfusion_amd.model.mano_head import mano_regHead

    dev = torch.device("cuda:0")
    rec = {"tool": "mano_bench", "reps": args.reps}
    m = mano_regHead().to(dev).train()
    gen = torch.Generator().manual_seed(0)
    feats = torch.randn(32, 1024, generator=gen).to(dev)
    keys = ("verts3d", "joints3d", "mano_shape", "mano_pose", "mano_pose_aa")
    for layer in ("torch", "hip"):
        def step():
            x = feats.clone().requires_grad_(True)
            out = mano_head_train_forward(m, x, layer=layer)
            sum(out[k].sum() for k in keys).backward()
            m.zero_grad(set_to_none=True)

        rec["head_train_step_ms_B32_%s" % layer] = _timed(step, args.reps, torch)

    # the fit: targets are the synthetic hand's own joints at a random pose, moved half a metre in front of the camera
    with torch.no_grad():
        pose = m.eval()(feats)
    target = (pose["joints3d"] + torch.tensor([30.0, -20.0, 600.0], device=dev)).contiguous()
    for B in (1, 32):
        for iters in (10, 50):
            fitter = ManoFitter(m, dev, iters=iters)
            y = target[:B].contiguous()
            rec["fit_ms_B%d_iters%d" % (B, iters)] = _timed(lambda: fitter.fit(y), args.reps, torch)
            out = fitter.fit(y)
            rec["fit_residual_mm_B%d_iters%d" % (B, iters)] = [float(v) for v in out["residual"].mean(0)]
    # the Gauss-Newton fit on the same targets: its default 8 iterations, 1 and 0 iterations for the cost of one, and Adam's figures of this run
    for B in (1, 32):
        fitter = ManoFitter(m, dev)
        y = target[:B].contiguous()
        ms = {n: _timed(lambda: fitter.fit_gn(y, iters=n), args.reps, torch) for n in (0, 1, 8)}
        out = fitter.fit_gn(y)
        rec["fit_gn_B%d" % B] = {"ms_iters8": ms[8], "ms_iters1": ms[1], "ms_iters0": ms[0], "ms_per_iteration": (ms[8] - ms[1]) / 7,
                                 "residual_mm": [float(v) for v in out["residual"].mean(0)], "history_mm": [float(v) for v in out["history"].mean(0)],
                                 "status": sorted(set(int(v) for v in out["status"])),
                                 "adam_ms_iters10": rec["fit_ms_B%d_iters10" % B], "adam_ms_iters50": rec["fit_ms_B%d_iters50" % B],
                                 "adam_residual_mm_iters10": rec["fit_residual_mm_B%d_iters10" % B][1],
                                 "adam_residual_mm_iters50": rec["fit_residual_mm_B%d_iters50" % B][1]}
    # the mesh fit: the vertex targets are the hand's own vertices; the cloud is 1024 of them with 0.5 mm of noise
    verts = (pose["verts3d"] + torch.tensor([30.0, -20.0, 600.0], device=dev)).contiguous()
    pick = torch.randint(0, 778, (1024,), generator=gen).to(dev)
    points = (verts[:, pick] + 0.5 * torch.randn(32, 1024, 3, generator=gen).to(dev)).contiguous()
    ones = torch.ones(32, 778, device=dev)
    for B in (1, 32):
        fitter = ManoFitter(m, dev, iters=50)
        y, vt, u, pts = target[:B].contiguous(), verts[:B].contiguous(), ones[:B].contiguous(), points[:B].contiguous()
        rec["fit_mesh_ms_B%d_iters50" % B] = _timed(lambda: fitter.fit_mesh(y, None, vt, u), args.reps, torch)
        rec["fit_mesh_residual_mm_B%d_iters50" % B] = [float(v) for v in fitter.fit_mesh(y, None, vt, u)["residual"].mean(0)]
        rec["associate_ms_B%d_N1024" % B] = _timed(lambda: fitter.associate(pts, vt), args.reps, torch)
        rec["fit_cloud_ms_B%d_iters50_rounds3" % B] = _timed(lambda: fitter.fit_cloud(y, pts), args.reps, torch)
        out = fitter.fit_cloud(y, pts)
        rec["fit_cloud_mm_B%d_iters50_rounds3" % B] = [float(out["cloud_before"][:, 1].mean()), float(out["cloud_after"][:, 1].mean())]
        # the Gauss-Newton mesh fit on the same targets, and the chain with Gauss-Newton rounds (6 rounds of 2 iterations) beside Adam's
        ms = {n: _timed(lambda: fitter.fit_mesh_gn(y, None, vt, u, iters=n), args.reps, torch) for n in (0, 1, 2, 8)}
        out = fitter.fit_mesh_gn(y, None, vt, u)
        rec["fit_mesh_gn_B%d" % B] = {"ms_iters0": ms[0], "ms_iters1": ms[1], "ms_iters2": ms[2], "ms_iters8": ms[8], "ms_per_iteration": (ms[8] - ms[1]) / 7,
                                      "residual_mm": [float(v) for v in out["residual"].mean(0)],
                                      "history_mm": [[float(v) for v in row] for row in out["history"].mean(0)],
                                      "status": sorted(set(int(v) for v in out["status"])),
                                      "adam_ms_iters50": rec["fit_mesh_ms_B%d_iters50" % B],
                                      "adam_residual_mm_iters50": rec["fit_mesh_residual_mm_B%d_iters50" % B]}
        gn = dict(rounds=6, iters_cloud=2, cloud_solver="gn")
        cloud_ms = _timed(lambda: fitter.fit_cloud(y, pts, **gn), args.reps, torch)
        out = fitter.fit_cloud(y, pts, **gn)
        rec["fit_cloud_gn_B%d" % B] = {"ms_rounds6_iters2": cloud_ms, "cloud_mm": [float(out["cloud_before"][:, 1].mean()), float(out["cloud_after"][:, 1].mean())],
                                       "status": sorted(set(int(v) for v in out["status"])),
                                       "adam_ms_rounds3_iters50": rec["fit_cloud_ms_B%d_iters50_rounds3" % B],
                                       "adam_cloud_mm_rounds3_iters50": rec["fit_cloud_mm_B%d_iters50_rounds3" % B]}
        # the surface entries: the normals, the association over the camera-facing vertices, and the chain with point-to-plane rounds beside
        # the point-to-vertex chain of this run.  The synthetic hand's faces are random, so the figures that mean something here are the times.
        nrm = fitter.normals(vt)
        rec["normals_B%d" % B] = {"ms": _timed(lambda: fitter.normals(vt), args.reps, torch), "faces": int(fitter.faces.shape[0])}
        vis = fitter.associate(pts, vt, normals=nrm)
        rec["assoc_vis_B%d" % B] = {"ms_N1024": _timed(lambda: fitter.associate(pts, vt, normals=nrm), args.reps, torch),
                                    "visible": float(vis["stats"][:, 3].mean()), "matched": float(vis["stats"][:, 0].mean()),
                                    "associate_ms_N1024": rec["associate_ms_B%d_N1024" % B]}
        pl_ms = {n: _timed(lambda: fitter.fit_mesh_gn(y, None, vt, u, iters=n, vert_normal=nrm), args.reps, torch) for n in (1, 8)}
        plane = dict(gn, metric="plane")
        plane_ms = _timed(lambda: fitter.fit_cloud(y, pts, **plane), args.reps, torch)
        out = fitter.fit_cloud(y, pts, **plane)
        rec["fit_cloud_plane_B%d" % B] = {"ms_rounds6_iters2": plane_ms, "cloud_mm": [[float(v) for v in out[k].mean(0)] for k in ("cloud_before", "cloud_after")],
                                          "status": sorted(set(int(v) for v in out["status"])),
                                          "fit_mesh_gn_plane_ms_iters1": pl_ms[1], "fit_mesh_gn_plane_ms_iters8": pl_ms[8],
                                          "fit_mesh_gn_plane_ms_per_iteration": (pl_ms[8] - pl_ms[1]) / 7,
                                          "point_ms_rounds6_iters2": cloud_ms, "point_ms_per_iteration": rec["fit_mesh_gn_B%d" % B]["ms_per_iteration"]}
        # the z-buffer render: camera (475, 475, 320, 240) and the map that puts a 250 mm square around the mesh's mean onto the window; the
        # observed crop is the render of the neighbouring hand.  Random faces span the whole hand, so every pixel is contested: an upper figure; ms_128_local_faces is the time with faces of a real mesh's size.
        fx, u0, v0 = 475.0, 320.0, 240.0
        mean = vt.mean(1)
        cam = torch.tensor([fx, fx, u0, v0], device=dev).repeat(B, 1).contiguous()

        def crop_map(size):
            sc = size / (250.0 * fx / mean[:, 2])
            Mx = torch.zeros(B, 2, 3, device=dev)
            Mx[:, 0, 0], Mx[:, 1, 1] = sc, sc
            Mx[:, 0, 2] = size / 2.0 - sc * (mean[:, 0] * fx / mean[:, 2] + u0)
            Mx[:, 1, 2] = size / 2.0 - sc * (mean[:, 1] * fx / mean[:, 2] + v0)
            return Mx.contiguous()

        M128, M32 = crop_map(128), crop_map(32)
        # mesh-like faces: each vertex of hand 0 with its two nearest neighbours, and with its second and third -- 1556 faces a few pixels wide.  The skin
        # is random, so another hand's neighbours are others: the batch for this figure is hand 0, B times.
        near = torch.cdist(vt[0], vt[0]).topk(4, largest=False).indices.to(torch.int32)
        local = ManoFitter(m, dev)
        local.faces = torch.cat([near[:, [0, 1, 2]], near[:, [0, 2, 3]]]).contiguous()
        v0, M0 = vt[:1].repeat(B, 1, 1).contiguous(), M128[:1].repeat(B, 1, 1).contiguous()
        ren_local = local.render_depth(v0, cam, M0)
        ren = fitter.render_depth(vt, cam, M128)
        obs = torch.roll(ren["depth"], 1, 0).clone()
        rec["raster_B%d" % B] = {"ms_128": _timed(lambda: fitter.render_depth(vt, cam, M128), args.reps, torch),
                                 "ms_128_obs": _timed(lambda: fitter.render_depth(vt, cam, M128, depth_obs=obs), args.reps, torch),
                                 "ms_32": _timed(lambda: fitter.render_depth(vt, cam, M32, size=(32, 32)), args.reps, torch),
                                 "ms_128_local_faces": _timed(lambda: local.render_depth(v0, cam, M0), args.reps, torch),
                                 "covered_128_local_faces": float(ren_local["stats"][:, 0].mean()),
                                 "covered_128": float(ren["stats"][:, 0].mean()), "occluded": float(ren["occluded"].sum(1).float().mean()),
                                 "faces": int(fitter.faces.shape[0]), "normals_ms": rec["normals_B%d" % B]["ms"],
                                 "assoc_vis_ms_N1024": rec["assoc_vis_B%d" % B]["ms_N1024"]}
        zbuf = dict(plane, occlusion="zbuffer", camera=(cam, M128), depth_obs=obs)
        zbuf_ms = _timed(lambda: fitter.fit_cloud(y, pts, **zbuf), args.reps, torch)
        out = fitter.fit_cloud(y, pts, **zbuf)
        rec["fit_cloud_zbuf_B%d" % B] = {"ms_rounds6_iters2": zbuf_ms, "cloud_mm": [[float(v) for v in out[k].mean(0)] for k in ("cloud_before", "cloud_after")],
                                         "status": sorted(set(int(v) for v in out["status"])), "depth_stats": [float(v) for v in out["depth_stats"].mean(0)],
                                         "iou": float(out["iou"].mean()), "plane_ms_rounds6_iters2": plane_ms}
        # the free-space term: the silhouette of the observed crop (the neighbouring hand's render, so vertices of both kinds exist), the
        # term on the mesh with and without the association's outputs, and the plane chain with it beside the plane chain of this run
        obs32 = torch.roll(fitter.render_depth(vt, cam, M32, size=(32, 32))["depth"], 1, 0).clone()
        sil = {k: t.clone() for k, t in fitter.silhouette(obs).items()}
        rec["silhouette_B%d" % B] = {"ms_128": _timed(lambda: fitter.silhouette(obs), args.reps, torch),
                                     "ms_32": _timed(lambda: fitter.silhouette(obs32), args.reps, torch),
                                     "observed_128": float(sil["count"].float().mean())}
        fs = fitter.free_space(vt, cam, M128, sil)
        rec["free_space_B%d" % B] = {"ms": _timed(lambda: fitter.free_space(vt, cam, M128, sil), args.reps, torch),
                                     "ms_with_inputs": _timed(lambda: fitter.free_space(vt, cam, M128, sil, vert_target=vis["vert_target"],
                                                                                        vert_weight=vis["vert_weight"], vert_normal=nrm), args.reps, torch),
                                     "stats": [float(v) for v in fs["stats"].mean(0)]}
        free = dict(plane, camera=(cam, M128), depth_obs=obs, free_space="silhouette")
        free_ms = _timed(lambda: fitter.fit_cloud(y, pts, **free), args.reps, torch)
        out = fitter.fit_cloud(y, pts, **free)
        rec["fit_cloud_free_B%d" % B] = {"ms_rounds6_iters2": free_ms, "cloud_mm": [[float(v) for v in out[k].mean(0)] for k in ("cloud_before", "cloud_after")],
                                         "status": sorted(set(int(v) for v in out["status"])),
                                         "free_stats": [[float(v) for v in out[k].mean(0)] for k in ("free_before", "free_after")],
                                         "plane_ms_rounds6_iters2": plane_ms}
    # the mesh evaluation: the fitted hands scored against the hands 2 mm away; beside it the same figures as torch ops
    from keypointfusion_amd.evaluation import similarity_align
    from keypointfusion_amd.evaluation_mesh_gpu import DeviceMeshEvaluator
    gt_all = (verts + 2.0 * torch.randn(32, 778, 3, generator=gen).to(dev)).contiguous()
    for B in (1, 32):
        ev = DeviceMeshEvaluator()
        pv, gv = verts[:B].contiguous(), gt_all[:B].contiguous()
        th, taus = torch.from_numpy(ev.thresholds).to(dev), ev.f_thresholds

        def torch_figures():
            out = []
            for a in (pv.double(), similarity_align(pv.double(), gv.double())):
                d = torch.cdist(a, gv.double())
                e = (a - gv.double()).norm(dim=-1)
                d_pg, d_gp = d.min(2).values, d.min(1).values
                f = [((d_pg <= t).double().mean(1), (d_gp <= t).double().mean(1)) for t in taus]
                out += [e.mean(1), (e[..., None] <= th).sum((0, 1)).double()] + [2 * p * r / (p + r).clamp_min(1e-300) for p, r in f]
            return torch.cat([o.reshape(-1) for o in out]).cpu()

        ms = _timed(lambda: ev.update(pv, gv), args.reps, torch)
        ev.reset()
        ev.update(pv, gv)
        summ, ref = ev.summary(), torch_figures()
        rec["mesh_eval_B%d" % B] = {"ms_update": ms, "ms_torch_ops": _timed(torch_figures, args.reps, torch), "verts": 778,
                                    "mean_error_mm": summ["mean_error"], "pa_mean_error_mm": summ["pa_mean_error"],
                                    "f_score": {str(t): summ["f_score"][t] for t in taus}, "pa_f_score": {str(t): summ["pa_f_score"][t] for t in taus},
                                    "auc": summ["auc"], "torch_mean_error_mm": float(ref[:B].mean()), "fit_gn_ms_iters8": rec["fit_gn_B%d" % B]["ms_iters8"]}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
