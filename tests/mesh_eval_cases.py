"""Inputs, restatement and yardstick calls of the mesh evaluation tests (tests/test_evaluation_mesh_host.py, tests/test_evaluation_mesh_gpu.py).

Inputs: the surface model's three hands (mano_surface_cases.surface_poses: V = 778, about 600 mm in front of the camera) as ground truth and predictions of
nine kinds, and small batches of random points at the V that straddle the kernel's lane (64), wave (64 -> 65), thread-stride (256 -> 257) and LDS (1024)
boundaries.  `restate` is kpf_eval_mesh_f32 in numpy float64, operation for operation in the order include/kpf.h states (the sums over vertices by the
kernel's tree, the 3 x 3 rotation by its Jacobi sweeps): the plain outputs are expected bit for bit, the aligned ones within the tolerance the float64
yardstick (keypointfusion_amd/evaluation_mesh.py, LAPACK's SVD) is held to.  `yardstick` is that module on the same inputs, rounded once to float32."""
import functools
import math

import numpy as np

import mano_surface_cases as S
from keypointfusion_amd import evaluation_mesh as EM

KINDS = ("noisy2", "noisy8", "similarity", "mirrored", "permuted", "shifted", "equal", "coincident", "duplicate")
BATCHES = (KINDS[:5], KINDS[5:])  # B = 5 and B = 4
SMALL_V = (1, 3, 63, 65, 256, 257, 1024)
DUP = (100, 101)  # `duplicate`: ground-truth vertex 101 is a copy of vertex 100
TH_PLAIN = (0.0, 50.0, 100)  # the evaluator's default table: threshold 0.0 meets the error 0.0 of `equal`
TH_DECIDED = (0.5, 50.0, 100)  # the table of the comparisons with the yardstick: no distance of any case lies within DECIDED_MM of one of these
F_TH = (5.0, 15.0)
DECIDED_MM = 1e-6  # a count / an index is compared where the yardstick's distances differ by more than this from the threshold / from each other
ORIGIN_VERTEX = 0  # the origins of the root-relative runs: each set's own vertex 0


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))  # proper: det = +1


def predict(kind, g32, rng):
    """The prediction of one kind for the ground truth g32 [V][3] float32 -> (pred float32, gt float32; `duplicate` changes the ground truth)."""
    g32 = g32.copy()
    g = g32.astype(np.float64)
    V = g.shape[0]
    if kind in ("noisy2", "noisy8"):
        p = g + float(kind[5:]) * rng.normal(size=(V, 3))
    elif kind == "similarity":  # an exact similarity copy up to its float32 rounding: the aligned error is rounding residue
        p = 1.1 * (g - g.mean(0)) @ _rotation(rng).T + g.mean(0) + np.array([12.0, -7.0, 25.0])
    elif kind == "mirrored":  # mirrored through the plane z = centroid: the reflection branch of the alignment
        p = g + 2.0 * rng.normal(size=(V, 3))
        p[:, 2] = 2.0 * g[:, 2].mean() - p[:, 2]
    elif kind == "permuted":  # the same point set with the vertices shuffled: large err, nn == 0, F == 1
        return g32[rng.permutation(V)].copy(), g32
    elif kind == "shifted":
        p = g + np.array([3.0, -2.0, 4.0])
    elif kind == "equal":
        return g32.copy(), g32  # bit for bit
    elif kind == "coincident":  # no alignment exists: var == 0
        p = np.repeat(g.mean(0, keepdims=True), V, 0)
    elif kind == "duplicate":  # two identical candidates: the lowest index must win
        g32[DUP[1]] = g32[DUP[0]]
        p = g32.astype(np.float64) + 2.0 * rng.normal(size=(V, 3))
    else:
        raise ValueError(kind)
    return p.astype(np.float32), g32


@functools.lru_cache(maxsize=None)
def kind_batch(i):
    """(pred, gt [B][778][3] float32, kinds) of BATCHES[i]; sample b's ground truth is hand b % 3."""
    hands = S.surface_poses().numpy()
    rng = np.random.default_rng(1000 + i)
    pairs = [predict(k, hands[b % 3], rng) for b, k in enumerate(BATCHES[i])]
    return np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs]), BATCHES[i]


@functools.lru_cache(maxsize=None)
def small_batch(V, B=2):
    """(pred, gt [B][V][3] float32): random points in a 160 mm box half a metre in front of the camera, predicted with 3 mm of noise."""
    rng = np.random.default_rng(2000 + V)
    gt = (rng.uniform(-80.0, 80.0, size=(B, V, 3)) + np.array([10.0, -30.0, 500.0])).astype(np.float32)
    pred = (gt.astype(np.float64) + 3.0 * rng.normal(size=(B, V, 3))).astype(np.float32)
    return pred, gt


def origins(pred, gt):
    return np.ascontiguousarray(pred[:, ORIGIN_VERTEX]), np.ascontiguousarray(gt[:, ORIGIN_VERTEX])


def ulp32(x):
    """The spacing of float32 at |x| (numpy's: towards larger magnitude)."""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def within_tolerance(got32, want32):
    """|got - want| <= max(1 ulp32, 1e-7 mm) elementwise, NaN and +inf matching themselves; -> (ok [..] bool, the differences where both are finite)."""
    got, want = np.asarray(got32, np.float64), np.asarray(want32, np.float64)
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & (got == want))
    fin = np.isfinite(got) & np.isfinite(want)
    with np.errstate(invalid="ignore"):
        diff = np.where(fin, np.abs(got - want), 0.0)
        ok = same | (fin & (diff <= np.maximum(ulp32(np.where(fin, want, 0.0)), 1e-7)))
    return ok, diff


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the restatement of kpf_eval_mesh_f32 (include/kpf.h)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def tree_sum(x):
    """x [V] or [V][K] float64 -> the kernel's sum over vertices: thread t adds its vertices t, t + 256, ... in ascending order onto +0.0, the 64-lane xor
    butterfly of each of the four waves, then ((w0 + w1) + w2) + w3."""
    x = np.asarray(x, np.float64)
    part = np.zeros((256,) + x.shape[1:])
    for lo in range(0, x.shape[0], 256):
        chunk = x[lo:lo + 256]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    waves = part.reshape((4, 64) + x.shape[1:])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lane ^ o]
    assert all(np.array_equal(waves[:, 0], waves[:, k], equal_nan=True) for k in (1, 31, 63))  # every lane ends with the same bits
    w = waves[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def _jacobi_rotate(a, v, p, q):
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    r = 3 - p - q
    arp, arq = a[r][p], a[r][q]
    a[p][p] -= t * apq
    a[q][q] += t * apq
    a[p][q] = a[q][p] = 0.0
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for k in range(3):
        vp, vq = v[k][p], v[k][q]
        v[k][p] = c * vp - s * vq
        v[k][q] = s * vp + c * vq


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def _cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def _matvec(H, x):
    return [H[i][0] * x[0] + H[i][1] * x[1] + H[i][2] * x[2] for i in range(3)]


def umeyama_rotation(H):
    """eval_umeyama_rotation of csrc/kpf_eval.hip in Python floats (IEEE double, one rounding per operation) -> (R [3][3], tr)."""
    H = [[float(H[i][k]) for k in range(3)] for i in range(3)]
    a = [[H[0][i] * H[0][k] + H[1][i] * H[1][k] + H[2][i] * H[2][k] for k in range(3)] for i in range(3)]
    v = [[1.0 if i == k else 0.0 for k in range(3)] for i in range(3)]
    for i in range(3):
        for k in range(i):
            a[i][k] = a[k][i]
    for _ in range(8):
        _jacobi_rotate(a, v, 0, 1)
        _jacobi_rotate(a, v, 0, 2)
        _jacobi_rotate(a, v, 1, 2)
    lam = [a[0][0], a[1][1], a[2][2]]
    for i, k in ((0, 1), (1, 2), (0, 1)):  # descending
        if lam[i] < lam[k]:
            lam[i], lam[k] = lam[k], lam[i]
            for r in range(3):
                v[r][i], v[r][k] = v[r][k], v[r][i]
    v1, v2 = [v[k][0] for k in range(3)], [v[k][1] for k in range(3)]
    v3 = _cross(v1, v2)
    u1 = _matvec(H, v1)
    s1 = math.sqrt(_dot(u1, u1))
    u1 = [x / s1 for x in u1] if s1 > 0.0 else [1.0, 0.0, 0.0]
    w = _matvec(H, v2)
    p = _dot(u1, w)
    u2 = [w[k] - p * u1[k] for k in range(3)]
    n2 = math.sqrt(_dot(u2, u2))
    if n2 > 0.0:
        u2 = [x / n2 for x in u2]
    else:  # rank 1: a unit vector orthogonal to u1, along the axis u1 leans on least
        f = [abs(x) for x in u1]
        k = (0 if f[0] <= f[2] else 2) if f[0] <= f[1] else (1 if f[1] <= f[2] else 2)
        u2 = [(1.0 if i == k else 0.0) - u1[k] * u1[i] for i in range(3)]
        n = math.sqrt(_dot(u2, u2))
        u2 = [x / n for x in u2]
    u3 = _cross(u1, u2)
    s3 = _dot(u3, _matvec(H, v3))
    s2 = _dot(u2, _matvec(H, v2))
    R = [[v1[i] * u1[k] + v2[i] * u2[k] + v3[i] * u3[k] for k in range(3)] for i in range(3)]
    return R, s1 + s2 + s3


def _nearest(q, s):
    """The kernel's scan: candidates j = 0 .. in ascending order, strict <, from +inf -> (nn float32 [V], idx int32 [V])."""
    best, idx = np.full(q.shape[0], np.inf), np.full(q.shape[0], -1, np.int32)
    with np.errstate(invalid="ignore"):
        for j in range(s.shape[0]):
            dx, dy, dz = q[:, 0] - s[j, 0], q[:, 1] - s[j, 1], q[:, 2] - s[j, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            win = d2 < best
            best[win], idx[win] = d2[win], j
    return np.sqrt(best).astype(np.float32), idx


def restate(pred, gt, pred_origin=None, gt_origin=None, thresholds=TH_PLAIN, f_thresholds=F_TH):
    """kpf_eval_mesh_f32 in numpy float64 -> dict(err [2][B][V] f32, nn [2][2][B][V] f32, nn_idx [2][2][B][V] i32, mean_err [2][B] f64,
    pck_cnt [2][B][T] i32, f_cnt [2][B][Tf][2] i32)."""
    th, fth = EM.threshold_table(thresholds), np.asarray(f_thresholds, np.float64)
    B, V = pred.shape[:2]
    out = dict(err=np.zeros((2, B, V), np.float32), nn=np.zeros((2, 2, B, V), np.float32), nn_idx=np.zeros((2, 2, B, V), np.int32),
               mean_err=np.zeros((2, B)), pck_cnt=np.zeros((2, B, len(th)), np.int32), f_cnt=np.zeros((2, B, len(fth), 2), np.int32))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            a, g = pred[b].astype(np.float64), gt[b].astype(np.float64)
            if pred_origin is not None:
                a, g = a - pred_origin[b].astype(np.float64), g - gt_origin[b].astype(np.float64)
            for ps in range(2):
                if ps == 1:
                    n = float(V)
                    ca, cb = tree_sum(a) / n, tree_sum(g) / n
                    a0, b0 = a - ca, g - cb
                    H = tree_sum((a0[:, :, None] * b0[:, None, :]).reshape(V, 9)).reshape(3, 3) / n
                    var = tree_sum(a0[:, 0] * a0[:, 0] + a0[:, 1] * a0[:, 1] + a0[:, 2] * a0[:, 2]) / n
                    R, tr = umeyama_rotation(H)
                    scale = np.float64(tr) / var
                    a = np.stack([scale * (R[k][0] * a0[:, 0] + R[k][1] * a0[:, 1] + R[k][2] * a0[:, 2]) + cb[k] for k in range(3)], -1)
                d = a - g
                e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32)
                out["err"][ps, b] = e
                out["mean_err"][ps, b] = tree_sum(e.astype(np.float64)) / float(V)
                out["pck_cnt"][ps, b] = (e.astype(np.float64)[:, None] <= th[None, :]).sum(0)
                for dr, (q, s) in enumerate(((a, g), (g, a))):
                    out["nn"][ps, dr, b], out["nn_idx"][ps, dr, b] = _nearest(q, s)
                    out["f_cnt"][ps, b, :, dr] = (out["nn"][ps, dr, b].astype(np.float64)[:, None] <= fth[None, :]).sum(0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the yardstick (keypointfusion_amd/evaluation_mesh.py), rounded once to float32, and how well it decides indices and counts
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _gap(q, s):
    """second-nearest minus nearest distance of every vertex of q [V][3] among s [Vs][3], float64 (+inf when there is no second candidate or a NaN)"""
    with np.errstate(invalid="ignore"):
        d = np.sqrt(((q[:, None, :] - s[None, :, :]) ** 2).sum(-1))
    if s.shape[0] < 2 or np.isnan(d).any():
        return np.full(q.shape[0], np.inf)
    two = np.partition(d, 1, axis=1)[:, :2]
    return two[:, 1] - two[:, 0]


def yardstick(pred, gt, pred_origin=None, gt_origin=None, thresholds=TH_DECIDED, f_thresholds=F_TH):
    """evaluation_mesh on one batch -> dict(err, nn float32 like the device's log; nn_idx int64; gap [2][2][B][V] float64; pck_cnt, f_cnt; margin = the
    smallest |distance - threshold| over everything counted, per pass [2]; conditioning [B])."""
    th, fth = EM.threshold_table(thresholds), np.asarray(f_thresholds, np.float64)
    p, al, g = EM.aligned_sets(pred, gt, pred_origin, gt_origin)
    plain, aligned = EM.mesh_errors(pred, gt, pred_origin, gt_origin)
    B, V = plain.shape
    out = dict(err=np.stack([plain, aligned]).astype(np.float32), nn=np.zeros((2, 2, B, V), np.float32), nn_idx=np.zeros((2, 2, B, V), np.int64),
               gap=np.zeros((2, 2, B, V)), margin=np.full(2, np.inf))
    for ps, x in enumerate((p, al)):
        for dr, (q, s) in enumerate(((x, g), (g, x))):
            dist, idx = EM.nearest_vertex(q, s)
            out["nn"][ps, dr], out["nn_idx"][ps, dr] = dist.astype(np.float32), idx
            out["gap"][ps, dr] = np.stack([_gap(q[b], s[b]) for b in range(B)])
            fin = dist[np.isfinite(dist)]
            if fin.size:
                out["margin"][ps] = min(out["margin"][ps], np.abs(fin[:, None] - fth[None, :]).min())
        e64 = (plain, aligned)[ps]
        fin = e64[np.isfinite(e64)]
        if fin.size:
            out["margin"][ps] = min(out["margin"][ps], np.abs(fin[:, None] - th[None, :]).min())
    with np.errstate(invalid="ignore"):
        out["pck_cnt"] = (out["err"].astype(np.float64)[..., None] <= th).sum(2).astype(np.int32)  # [2][B][T]
        out["f_cnt"] = np.moveaxis((out["nn"].astype(np.float64)[..., None] <= fth).sum(3), 1, 3).astype(np.int32)  # [2][2][B][Tf] -> [2][B][Tf][2]
    out["conditioning"] = conditioning(p, g)
    return out


def conditioning(pred, gt):
    """(sigma2 + d sigma3) / sigma1 of every sample's cross-covariance, float64 (tests/eval_cases.py): two correct SVDs agree on the aligned set up to
    rounding / this number.  NaN for a sample without variance."""
    A, Bm = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    A0, B0 = A - A.mean(1, keepdims=True), Bm - Bm.mean(1, keepdims=True)
    H = np.einsum("bji,bjk->bik", A0, B0) / A.shape[1]
    U, Sv, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (Sv[:, 1] + d * Sv[:, 2]) / Sv[:, 0]


_YARD, _RESTATED = {}, {}


def cases():
    """[(name, pred, gt)]: the two batches of kinds and the small-V batches."""
    out = [("kinds%d" % i,) + kind_batch(i)[:2] for i in range(len(BATCHES))]
    return out + [("V%d" % V,) + small_batch(V) for V in SMALL_V]


def case(name):
    return {n: (p, g) for n, p, g in cases()}[name]


def case_names():
    return ["kinds%d" % i for i in range(len(BATCHES))] + ["V%d" % V for V in SMALL_V]


def yardstick_of(name, with_origins):
    """computed once per (case, origins) and shared"""
    key = (name, bool(with_origins))
    if key not in _YARD:
        pred, gt = case(name)
        _YARD[key] = yardstick(pred, gt, *(origins(pred, gt) if with_origins else (None, None)))
    return _YARD[key]


def restated_of(name, with_origins, thresholds=TH_PLAIN):
    key = (name, bool(with_origins), thresholds)
    if key not in _RESTATED:
        pred, gt = case(name)
        _RESTATED[key] = restate(pred, gt, *(origins(pred, gt) if with_origins else (None, None)), thresholds=thresholds)
    return _RESTATED[key]
