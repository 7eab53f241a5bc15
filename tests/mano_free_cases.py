"""Inputs and the host restatements for the free-space term of the cloud fit (kpf_depth_silhouette_f32, kpf_mano_free_space_f32).  No GPU.

silhouette_brute is the definition (argmin over all observed pixels, first minimum in linear index), silhouette_host the separable algorithm the kernel
follows; both give integers and exact minima.  free_space_host restates the second kernel in numpy operation by operation: float32 is held to the
kernel's bits, float64 is what its geometry is judged in.  fit_cloud_free_reference extends mano_raster_cases.fit_cloud_curl_reference by the term."""
import functools

import numpy as np
import torch

import mano_raster_cases as R
import mano_surface_cases as S

NV = 778
DEFAULTS = dict(slack2=1, margin=5.0, step=20.0, lambda_free=1.0)
SIL_SIZES = ((1, 1), (3, 5), (16, 64), (32, 32), (1, 16384))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the silhouette
# ----------------------------------------------------------------------------------------------------------------------------------------
def observed(depth):
    """the raster's rule: finite and > 0"""
    d = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def front_host(depth):
    """[B, H, W] -> the minimum of the observed depths of each pixel's 3 x 3 neighbourhood clipped to the window, 0 where none is observed"""
    d = np.asarray(depth, np.float32)
    B, H, W = d.shape
    pad = np.full((B, H + 2, W + 2), np.inf, np.float32)
    pad[:, 1:-1, 1:-1] = np.where(observed(d), d, np.float32(np.inf))
    f = np.full((B, H, W), np.inf, np.float32)
    for i in range(3):
        for j in range(3):
            f = np.minimum(f, pad[:, i:i + H, j:j + W])
    return np.where(np.isfinite(f), f, np.float32(0))


def _maps(fn, depth):
    d = np.asarray(depth, np.float32)
    seen = observed(d)
    near, dist = (np.full(d.shape, -1, np.int32) for _ in range(2))
    for b in range(d.shape[0]):
        if seen[b].any():
            near[b], dist[b] = fn(seen[b])
    return near, dist, front_host(d), seen.sum((1, 2)).astype(np.int32)


def _brute_one(seen):
    H, W = seen.shape
    rr, cc = np.nonzero(seen)  # ascending linear index: argmin's first minimum is the lowest one
    near, dist = np.zeros(H * W, np.int32), np.zeros(H * W, np.int32)
    step = max(1, (1 << 22) // len(rr))
    for p0 in range(0, H * W, step):
        p = np.arange(p0, min(p0 + step, H * W))
        d2 = (p[:, None] // W - rr[None]) ** 2 + (p[:, None] % W - cc[None]) ** 2
        k = d2.argmin(1)
        near[p], dist[p] = rr[k] * W + cc[k], d2[np.arange(len(p)), k]
    return near.reshape(H, W), dist.reshape(H, W)


def _separable_one(seen):
    H, W = seen.shape
    col = np.arange(W)
    big = 1 << 20
    left = np.maximum.accumulate(np.where(seen, col, -2 * big), 1)              # the nearest observed column at or left of c
    right = np.minimum.accumulate(np.where(seen, col, big)[:, ::-1], 1)[:, ::-1]  # ... at or right of it
    pick = np.where(col - left <= right - col, left, right)                  # the lower column on a tie
    has = seen.any(1)
    near, dist = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    rows = np.nonzero(has)[0]
    chunk = max(1, (1 << 22) // (len(rows) * W))
    for r0 in range(0, H, chunk):
        r = np.arange(r0, min(r0 + chunk, H))
        d2 = (r[:, None, None] - rows[None, :, None]) ** 2 + (col[None, None] - pick[rows][None]) ** 2  # [r, r', c]
        k = d2.argmin(1)                                                     # ascending r', strict <
        near[r] = rows[k] * W + pick[rows[k], col[None]]
        dist[r] = np.take_along_axis(d2, k[:, None], 1)[:, 0]
    return near, dist


def silhouette_brute(depth):
    """the definition of kpf_depth_silhouette_f32: depth [B, H, W] -> nearest, dist2 (int32), front (float32), count (int32)"""
    return _maps(_brute_one, depth)


def silhouette_host(depth):
    """the separable algorithm: per row the nearest observed column (the lower one on a tie), then the minimum over the rows in ascending order"""
    return _maps(_separable_one, depth)


def mask_cases(H, W):
    """name -> depth [1, H, W] float32: the masks the silhouette is tested on"""
    full = np.full((1, H, W), 400.0, np.float32) + np.arange(H * W, dtype=np.float32).reshape(1, H, W) % 7
    out = {"empty": np.zeros((1, H, W), np.float32), "full": full}
    for name, (r, c) in (("corner00", (0, 0)), ("corner01", (0, W - 1)), ("corner10", (H - 1, 0)), ("corner11", (H - 1, W - 1))):
        d = np.zeros((1, H, W), np.float32)
        d[0, r, c] = 500.0
        out[name] = d
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out["checker"] = np.where((rr + cc) % 2 == 0, full, np.float32(0))
    d = np.zeros((1, H, W), np.float32)  # two pixels equidistant from the one between them, along a row and along a column
    d[0, 0, 0] = 450.0
    d[0, 0, min(2, W - 1)] = 460.0
    d[0, min(2, H - 1), 0] = 470.0
    out["equidistant"] = d
    out["pattern"] = R.observed_from(np.concatenate([full, full]))[:1]  # NaN, 0 and -5 among the depths
    return out


@functools.lru_cache(maxsize=None)
def render_obs(size):
    """the float32 render of hands() in the crop_for window of `size`: the observed crop of the self cases -> depth [5, H, W]"""
    return R.rendered(size)[0]


# ----------------------------------------------------------------------------------------------------------------------------------------
# the free-space term
# ----------------------------------------------------------------------------------------------------------------------------------------
def _tree(vals, dtype):
    """the kernel's sum of 778 values: thread t adds t, t + 256, ... in ascending order onto +0, a 64-lane butterfly per wave, the waves in order"""
    v = np.zeros(1024, dtype)
    v[:NV] = vals
    v = v.reshape(4, 256)
    part = np.zeros(256, dtype)
    for k in range(4):
        part = part + v[k]
    w = part.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def free_space_host(verts, cam, M, sil, slack2=1, margin=5.0, step=20.0, lambda_free=1.0, vert_target=None, vert_weight=None, vert_normal=None,
                    dtype=np.float32):
    """kpf_mano_free_space_f32 in numpy: verts [B, 778, 3], cam [B, 4], M [B, 2, 3] or None, sil = (nearest, dist2, front[, count]) [B, H, W] ->
    vert_target [B, 778, 3], vert_weight [B, 778], vert_normal [B, 778, 3] in `dtype`, kind [B, 778] int32, stats [B, 4] in `dtype`.  Every product,
    difference, sum, quotient and root is one operation of `dtype`."""
    Vb = np.ascontiguousarray(verts, dtype)
    B = Vb.shape[0]
    near, dist, front = (np.asarray(a) for a in sil[:3])
    H, W = front.shape[1:]
    half, zero = dtype(0.5), dtype(0)
    vt = np.zeros((B, NV, 3), dtype) if vert_target is None else np.array(vert_target, dtype)
    vw = np.zeros((B, NV), dtype) if vert_weight is None else np.array(vert_weight, dtype)
    vn = np.zeros((B, NV, 3), dtype) if vert_normal is None else np.array(vert_normal, dtype)
    kind, stats = np.zeros((B, NV), np.int32), np.zeros((B, 4), dtype)
    margin, step, lam = dtype(margin), dtype(step), dtype(lambda_free)
    with np.errstate(all="ignore"):
        for b in range(B):
            c = np.ascontiguousarray(np.asarray(cam)[b], dtype)
            m = np.asarray([[1, 0, 0], [0, 1, 0]], dtype) if M is None else np.ascontiguousarray(np.asarray(M)[b], dtype)
            sx, sy, _, ok = R.project_host(Vb[b], c, m, dtype)
            det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
            ok = ok & ~np.isnan(sx) & ~np.isnan(sy) & bool(det != 0 and np.isfinite(det))
            x, y, z = Vb[b][:, 0], Vb[b][:, 1], Vb[b][:, 2]
            cf = np.fmin(np.fmax(np.floor(sx + half), zero), dtype(W - 1))  # fmax / fmin as C's: a NaN loses
            rf = np.fmin(np.fmax(np.floor(sy + half), zero), dtype(H - 1))
            ci, ri = np.where(ok, cf, 0).astype(np.int64), np.where(ok, rf, 0).astype(np.int64)
            d2, n, f = dist[b][ri, ci].astype(np.int64), near[b][ri, ci].astype(np.int64), front[b][ri, ci].astype(dtype)
            # kind 1: the centre of the nearest observed pixel, at the vertex's depth
            k1 = ok & (d2 > slack2)
            rs, cs = n // W, n - (n // W) * W
            a_, b_ = (cs.astype(dtype) + half) - m[0, 2], (rs.astype(dtype) + half) - m[1, 2]
            u = (m[1, 1] * a_ - m[0, 1] * b_) / det
            v = (m[0, 0] * b_ - m[1, 0] * a_) / det
            t1 = np.stack([((u - c[2]) / c[0]) * z, ((v - c[3]) / c[1]) * z, z], -1)
            # kind 2: along the vertex's own ray to front - margin
            zt = f - margin
            k2 = ok & ~k1 & (d2 == 0) & (f > 0) & (z < zt)
            s = zt / z
            t2 = np.stack([x * s, y * s, zt], -1)
            k = np.where(k1, 1, np.where(k2, 2, 0))
            t = np.where(k1[:, None], t1, t2)
            d = t - Vb[b]
            ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            k = np.where((ln > 0) & np.isfinite(ln), k, 0)
            q = step / ln
            t = np.where((ln > step)[:, None], Vb[b] + d * q[:, None], t)
            on = k != 0
            vt[b] = np.where(on[:, None], t, vt[b])
            vn[b] = np.where(on[:, None], d / ln[:, None], vn[b])
            vw[b] = np.where(on, lam, vw[b])
            kind[b] = k
            n1, n2 = int((k == 1).sum()), int((k == 2).sum())
            s1 = _tree(np.where(k == 1, np.sqrt(d2.astype(dtype)), zero), dtype)
            s2 = _tree(np.where(k == 2, f - z, zero), dtype)
            stats[b] = [n1, s1 / dtype(n1) if n1 else zero, n2, s2 / dtype(n2) if n2 else zero]
    return vt, vw, vn, kind, stats


def project64(points, cam, M):
    """float64: points [n, 3], cam [4], M [2, 3] or None -> (sx, sy) with pixel (c, r) sampled at sx = c, sy = r (the raster's convention)"""
    p, c = np.asarray(points, np.float64), np.asarray(cam, np.float64)
    m = np.asarray([[1, 0, 0], [0, 1, 0]], np.float64) if M is None else np.asarray(M, np.float64)
    U, V = p[:, 0] * c[0] / p[:, 2] + c[2], p[:, 1] * c[1] / p[:, 2] + c[3]
    return m[0, 0] * U + m[0, 1] * V + m[0, 2] - 0.5, m[1, 0] * U + m[1, 1] * V + m[1, 2] - 0.5


def fold_crop(cam, M):
    """the crop map folded into the camera (M is a scale and a shift), for the cases without M: the same hand in the same window"""
    cam, M = np.asarray(cam, np.float32), np.asarray(M, np.float32)
    return np.stack([M[:, 0, 0] * cam[:, 0], M[:, 1, 1] * cam[:, 1], M[:, 0, 0] * cam[:, 2] + M[:, 0, 2], M[:, 1, 1] * cam[:, 3] + M[:, 1, 2]], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def crossed(size=(128, 128), with_M=True):
    """mesh b of hands() against the observation and the crop of hand (b + 1) % 5: hundreds of vertices of both kinds -> (verts [5, 778, 3], cam, M or
    None, silhouette_host of the other hand's render)"""
    v = R.hands()
    cam, M = R.crop_for(v, size)
    cam, M, obs = np.roll(cam, -1, 0), np.roll(M, -1, 0), np.roll(render_obs(size), -1, 0)
    if not with_M:
        cam, M = fold_crop(cam, M), None
    return v, cam, M, silhouette_host(obs)


@functools.lru_cache(maxsize=None)
def selfcase(size=(128, 128), with_M=True):
    """each of hands() against its own float32 render -> (verts, cam, M or None, silhouette_host of the render)"""
    v = R.hands()
    cam, M = R.crop_for(v, size)
    obs = render_obs(size)
    if not with_M:
        cam = fold_crop(cam, M)
        M = None
        obs = R.raster_host(v, R.surface_faces(), cam, None, size[0], size[1], 10.0)[0]
    return v, cam, M, silhouette_host(obs)


@functools.lru_cache(maxsize=None)
def assoc_inputs():
    """what associate and normals hand to free_space for hands(): (vert_target [5, 778, 3], vert_weight [5, 778], vert_normal [5, 778, 3]) float32, with
    a NaN, an infinity and a -0 among them (a pass-through is bit for bit)"""
    v = R.hands()
    nrm = S.normals_host(v, R.surface_faces())
    rng = np.random.Generator(np.random.PCG64(71))
    vt = (v + rng.standard_normal(v.shape)).astype(np.float32)
    vw = rng.integers(0, 4, v.shape[:2]).astype(np.float32)
    vt[:, 5, 0], vt[:, 6, 1], vw[:, 7], nrm[:, 8, 2] = np.nan, np.inf, -0.0, -0.0
    return vt, vw, nrm


# ----------------------------------------------------------------------------------------------------------------------------------------
# constructed scenes: camera UNIT and the identity map, so that vertex mano_raster_cases._at(c, r, z) lies exactly on pixel (c, r)
# ----------------------------------------------------------------------------------------------------------------------------------------
def scene_obs(H=16, W=16):
    """an observed plate over pixels 4..11 x 4..11 at 512 mm; everything else background"""
    d = np.zeros((1, H, W), np.float32)
    d[0, 4:12, 4:12] = 512.0
    return d


def scene_verts():
    """vertex -> what the defaults (slack2 1, margin 5, step 20) must say, on scene_obs():
      0 on the plate at its depth: 0            1 one pixel left of it (d2 = 1 = slack2): 0       2 two pixels left (d2 = 4): 1
      3 diagonal to its corner (d2 = 2): 1      4 on the plate at z = 507 = front - margin: 0     5 at the next float below 507: 2
      6 far in front (z = 300): 2, clamped      7 outside the window, left of row 6: 1            8 outside the window, below column 8: 1
      9 NaN: 0                                  10 z = 0: 0                                        11 behind the plate (z = 600): 0
    the rest are parked behind the camera: 0"""
    v = R._blank()
    v[0], v[1], v[2], v[3] = R._at(8, 8, 512.0), R._at(3, 6, 512.0), R._at(2, 6, 512.0), R._at(3, 3, 512.0)
    v[4], v[5] = R._at(8, 8, 507.0), R._at(8, 8, float(np.nextafter(np.float32(507.0), np.float32(0))))
    v[6], v[7], v[8] = R._at(6, 9, 300.0), R._at(-9, 6, 512.0), R._at(8, 20, 400.0)
    v[9], v[10], v[11] = (np.nan, 1.0, 500.0), (10.0, 10.0, 0.0), R._at(8, 8, 600.0)
    return v[None]


SCENE_KINDS = [0, 0, 1, 1, 0, 2, 2, 1, 1, 0, 0, 0]


# ----------------------------------------------------------------------------------------------------------------------------------------
# what float64 says about the term
# ----------------------------------------------------------------------------------------------------------------------------------------
def perturbed_start(scale=0.3, seed=5):
    """curl_inputs().near with scale * randn added to the pose (float64, then cast to float)"""
    c = R.curl_inputs()
    pose = c.near[0].double() + scale * torch.randn(2, 48, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (pose.float(), c.near[1], c.near[2])


def wrist_weights(n=7):
    """[2, 21]: 1 for the n joint targets nearest the wrist (target 0) of curl_inputs(), 0 for the others"""
    c = R.curl_inputs()
    d = (c.target - c.target[:, :1]).norm(dim=-1)
    w = torch.zeros(2, 21)
    w.scatter_(1, d.argsort(1)[:, :n], 1.0)
    return w


def fit_cloud_free_reference(free, start=None, weight=None, rounds=6, iters=50, iters_cloud=2, max_dist=20.0, size=(128, 128), **rule):
    """mano_raster_cases.fit_cloud_curl_reference(masked=False) with (free) or without the free-space term between the association and the solve: the
    Adam joint fit in float64 from `start` (None: curl_inputs().near) under `weight` (None: all 21 joints), then rounds x (normals_host, the association,
    free_space_host with `rule` over DEFAULTS, all on the float32 vertices, and the float64 Gauss-Newton plane fit).  The observed crop is the float32
    render of the true mesh.  -> (outside [2]: the vertices of kind 1 on the final mesh, in_front [2]: of kind 2, error [2]: the mean error of all 778
    vertices in mm)"""
    c, sd, faces = R.curl_inputs(), S.surface_sd(), R.surface_faces()
    pts, cam, M = c.cloud.numpy(), c.cam.numpy(), c.M.numpy()
    rule = dict(DEFAULTS, **rule)
    sil = silhouette_host(render_obs(size)[3:])
    w = c.weight if weight is None else weight
    state = S.adam_joint_fit(torch.float64, sd, c.target, w, c.near if start is None else start, iters)
    verts = S.layer(sd, torch.float64, *state)[0]
    for _ in range(rounds):
        v32 = verts.float().numpy()
        nrm = S.normals_host(v32, faces)
        a = R.associate_vis_mask_host(pts, None, v32, nrm, None, max_dist * max_dist)
        vt, vw, vn = a[1], a[2], nrm
        if free:
            vt, vw, vn, _, _ = free_space_host(v32, cam, M, sil, vert_target=vt, vert_weight=vw, vert_normal=vn, **rule)
        out = S.fit_mesh_gn_plane_reference(torch.float64, c.target, w, torch.from_numpy(vt), torch.from_numpy(vw), torch.from_numpy(vn), state,
                                            iters_cloud, init_trans=False, sd=sd)
        state, verts = (out["pose_aa"], out["betas"], out["trans"]), out["verts"]
    kind = free_space_host(verts.float().numpy(), cam, M, sil, **rule)[3]
    return (kind == 1).sum(1), (kind == 2).sum(1), (verts.double() - c.verts.double()).norm(dim=-1).mean(1).numpy()
