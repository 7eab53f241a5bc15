"""Mesh evaluation on the host, in numpy float64: the yardstick of `evaluation_mesh_gpu.DeviceMeshEvaluator` (tests/test_evaluation_mesh_gpu.py judges the
device against these functions).

The figures are those the HO3D / FreiHAND challenge servers report for a predicted hand mesh against a ground-truth mesh with the same vertices: the mean
per-vertex error, the same after the similarity (Procrustes) alignment of the prediction onto the ground truth, the F-score at given thresholds on
nearest-vertex distances in both directions, raw and aligned, and the PCK curve / AUC of the vertex errors pooled over all vertices.  The alignment is
`evaluation.rigid_align` (LAPACK's SVD; tests/test_evaluation.py pins it to the reference's own code through tests/golden/metrics.npz).  The F-score is
vertex to vertex, written from its definition; point-to-surface distances are not computed.

Units are the inputs' (mm).  Nothing here touches a device.
"""
import numpy as np

from . import evaluation as EV


def _sets(pred, gt, pred_origin, gt_origin):
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    if p.ndim != 3 or p.shape[2] != 3 or p.shape != g.shape or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError("evaluation_mesh: pred and gt must both be [B][V][3] (got %s and %s)" % (p.shape, g.shape))
    if (pred_origin is None) != (gt_origin is None):
        raise ValueError("evaluation_mesh: pred_origin and gt_origin are given together or not at all")
    if pred_origin is not None:
        po, go = np.asarray(pred_origin, np.float64), np.asarray(gt_origin, np.float64)
        if po.shape != (p.shape[0], 3) or go.shape != po.shape:
            raise ValueError("evaluation_mesh: origins must be [B][3] (got %s and %s)" % (po.shape, go.shape))
        p, g = p - po[:, None, :], g - go[:, None, :]
    return p, g


def _norm(d):
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def aligned_sets(pred, gt, pred_origin=None, gt_origin=None):
    """(pred - origin, aligned prediction, gt - origin), float64 [B][V][3]: what the errors and the nearest-vertex distances are taken on."""
    p, g = _sets(pred, gt, pred_origin, gt_origin)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p, EV.rigid_align(p, g), g


def mesh_errors(pred, gt, pred_origin=None, gt_origin=None):
    """(plain [B][V], aligned [B][V]) float64: the distance of every predicted vertex from its ground-truth vertex, as given and after the similarity
    alignment of each sample's prediction onto its ground truth.  Origins [B][3] are subtracted from their set first (the root-relative figures of the HO3D
    protocol).  A sample whose predicted vertices all coincide has no alignment: its aligned errors are NaN."""
    p, a, g = aligned_sets(pred, gt, pred_origin, gt_origin)
    return _norm(p - g), _norm(a - g)


def nearest_vertex(a, b):
    """(dist [B][V] float64, idx [B][V] int64): for every vertex of `a` [B][V][3] the nearest vertex of `b` [B][Vb][3], the lowest index on a tie.
    d2 = (dx*dx + dy*dy) + dz*dz, then sqrt.  A NaN distance never wins; a vertex for which nothing wins has idx -1 and dist +inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim != 3 or b.ndim != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError("nearest_vertex: a and b must be [B][V][3] with the same B (got %s and %s)" % (a.shape, b.shape))
    dist, idx = np.empty(a.shape[:2]), np.empty(a.shape[:2], np.int64)
    for s in range(a.shape[0]):  # one [V][Vb] matrix at a time
        with np.errstate(invalid="ignore"):
            dx, dy, dz = (a[s, :, None, k] - b[s, None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(d2 < np.inf, d2, np.inf)  # NaN and +inf never win
        i = np.argmin(d2, -1)  # the first occurrence of the minimum
        best = d2[np.arange(d2.shape[0]), i]
        dist[s], idx[s] = np.sqrt(best), np.where(best < np.inf, i, -1)
    return dist, idx


def f_score(d_pred_to_gt, d_gt_to_pred, tau):
    """(F, P, R) per sample, [B] float64: P = the share of predicted vertices within tau of the ground truth (d <= tau), R = the share of ground-truth
    vertices within tau of the prediction, F = 2 P R / (P + R), and 0 where P + R == 0."""
    dp, dg = np.asarray(d_pred_to_gt, np.float64), np.asarray(d_gt_to_pred, np.float64)
    with np.errstate(invalid="ignore"):
        P = (dp <= float(tau)).sum(-1) / float(dp.shape[-1])
        R = (dg <= float(tau)).sum(-1) / float(dg.shape[-1])
    F = np.zeros_like(P)
    pos = P + R > 0
    F[pos] = 2.0 * P[pos] * R[pos] / (P[pos] + R[pos])
    return F, P, R


def mesh_pck_auc_from_counts(counts, n_vertices_total, thresholds):
    """(curve [T], auc): counts [T] = how many of the n_vertices_total pooled vertex errors are <= thresholds[t]; auc = trapz(curve, th) / (th[-1] - th[0])."""
    th = np.asarray(thresholds, np.float64)
    counts = np.asarray(counts)
    if counts.shape != th.shape or th.ndim != 1 or th.shape[0] < 2:
        raise ValueError("mesh_pck_auc_from_counts: counts must be [%d] like the thresholds (got %s)" % (th.shape[0] if th.ndim == 1 else -1, counts.shape))
    curve = counts.astype(np.float64) / float(n_vertices_total)
    return curve, EV._trapz(curve, th) / float(th[-1] - th[0])


def threshold_table(thresholds):
    """(val_min, val_max, steps) -> np.linspace, the bits the device compares against; an array is taken as it is."""
    if isinstance(thresholds, tuple) and len(thresholds) == 3 and float(thresholds[2]) == int(thresholds[2]) and int(thresholds[2]) >= 2 \
            and float(thresholds[0]) < float(thresholds[1]):
        return np.linspace(float(thresholds[0]), float(thresholds[1]), int(thresholds[2]))
    return np.asarray(thresholds, np.float64)


def evaluate_meshes(pred, gt, thresholds, f_thresholds, valid=None, pred_origin=None, gt_origin=None, logged=None):
    """Everything `DeviceMeshEvaluator.summary()` returns, for one batch: samples, batches, mean_error (the mean over samples of the per-sample mean vertex
    error), per_vertex_mean [V], pck_curve [T], auc, f_score / precision / recall {threshold: mean over samples}, and the pa_ twins after the alignment.
    thresholds: [T] mm (or (val_min, val_max, steps)); f_thresholds: the F-score thresholds; valid: None or [B], false drops a sample.

    Every error and distance is rounded once to float32 before it is summed or compared, as the device logs them.  logged = (err [2][B][V], nn [2][2][B][V])
    scores those values in place of the ones computed here from pred and gt (an evaluator's own log: the aggregation alone is then restated)."""
    th, fth = threshold_table(thresholds), [float(t) for t in f_thresholds]
    if logged is None:
        p, a, g = aligned_sets(pred, gt, pred_origin, gt_origin)
        err = np.stack([_norm(p - g), _norm(a - g)])
        nn = np.stack([np.stack([nearest_vertex(x, g)[0], nearest_vertex(g, x)[0]]) for x in (p, a)])
    else:
        err, nn = np.asarray(logged[0]), np.asarray(logged[1])
    err, nn = err.astype(np.float32).astype(np.float64), nn.astype(np.float32).astype(np.float64)
    B, V = err.shape[1:]
    keep = np.ones(B, bool) if valid is None else np.asarray(valid).astype(bool)
    n = int(keep.sum())
    if n == 0:
        raise ValueError("evaluate_meshes: no valid sample")
    out = {"samples": n, "batches": 1}
    for a_, pre in ((0, ""), (1, "pa_")):
        e = err[a_][keep]
        out[pre + "mean_error"] = float(e.mean(1).mean())
        out[pre + "per_vertex_mean"] = e.mean(0)
        with np.errstate(invalid="ignore"):
            counts = (e[:, :, None] <= th[None, None, :]).sum((0, 1))
        out[pre + "pck_curve"], out[pre + "auc"] = mesh_pck_auc_from_counts(counts, n * V, th)
        out[pre + "f_score"], out[pre + "precision"], out[pre + "recall"] = {}, {}, {}
        for tau in fth:
            F, P, R = f_score(nn[a_][0][keep], nn[a_][1][keep], tau)
            out[pre + "f_score"][tau], out[pre + "precision"][tau], out[pre + "recall"][tau] = float(F.mean()), float(P.mean()), float(R.mean())
    return out
