"""Inputs and the host restatement for the z-buffer render (kpf_mano_raster_f32, kpf_mano_assoc_vis_mask_f32).  No GPU.

raster_host restates the kernel in numpy operation by operation: float32 is held to the kernel's bits, float64 is what its decisions are judged against.
curl_poses are the two curled hands of the surface model on which self-occlusion shows, crop_for a camera and a crop map that put a mesh into a window of
`size` pixels, and the scenes are meshes of a few hand-placed vertices (the rest parked behind the camera) whose render is known by construction."""
import functools

import numpy as np
import torch

import mano_surface_cases as S

NV = 778
CAM = (475.0, 475.0, 320.0, 240.0)
PARKED = (0.0, 0.0, -1000.0)  # behind the camera: z <= 0, so a face that lists such a vertex is skipped and the vertex is never occluded


# ----------------------------------------------------------------------------------------------------------------------------------------
# the render
# ----------------------------------------------------------------------------------------------------------------------------------------
def project_host(verts, cam, M, dtype=np.float32):
    """verts [778, 3], cam [4], M [2, 3] or None -> (sx, sy, iz, ok), each [778]: the crop coordinates with pixel (c, r) sampled at sx = c, sy = r"""
    V, c = np.ascontiguousarray(verts, dtype), np.ascontiguousarray(cam, dtype)
    m = np.asarray([[1, 0, 0], [0, 1, 0]], dtype) if M is None else np.ascontiguousarray(M, dtype)
    half, one = dtype(0.5), dtype(1)
    with np.errstate(all="ignore"):
        x, y, z = V[:, 0], V[:, 1], V[:, 2]
        U, Vv = (x * c[0]) / z + c[2], (y * c[1]) / z + c[3]
        sx = ((m[0, 0] * U + m[0, 1] * Vv) + m[0, 2]) - half
        sy = ((m[1, 0] * U + m[1, 1] * Vv) + m[1, 2]) - half
        iz = one / z
        ok = np.isfinite(V).all(1) & (z > 0)
    return sx, sy, iz, ok


def _edge(sx, sy, a, b, px, py):
    """the edge function of the directed edge a -> b at (px, py), evaluated from the lower vertex index and negated if a > b"""
    lo, hi = (a, b) if a < b else (b, a)
    e = (sx[hi] - sx[lo]) * (py - sy[lo]) - (sy[hi] - sy[lo]) * (px - sx[lo])
    return -e if a > b else e


def raster_host(verts, faces, cam, M, H, W, margin, depth_obs=None, dtype=np.float32, with_margins=False):
    """kpf_mano_raster_f32 in numpy: verts [B, 778, 3], faces [F, 3], cam [B, 4], M [B, 2, 3] or None, depth_obs [B, H, W] or None ->
    depth [B, H, W] in `dtype`, face [B, H, W] int32, occluded [B, 778] int32, stats [B, 4] in `dtype`.  Every product, difference, sum and quotient is
    one operation of `dtype`; the faces are taken in ascending order and a candidate replaces the pixel's only if it is strictly nearer, which is "the
    smallest d, among equal d the lowest face".

    with_margins: also edge [B, H, W], per pixel the smallest |w_i| / |area| over every face whose pixel box grown by one pixel holds it (how far the
    pixel is from changing sides of an edge; inf where no face is near), and gap [B, H, W], (second nearest d - nearest d) / nearest d over the faces
    that cover the pixel (inf with fewer than two)."""
    Vb, f = np.ascontiguousarray(verts, dtype), np.asarray(faces, np.int64).reshape(-1, 3)
    B = Vb.shape[0]
    one, zero = dtype(1), dtype(0)
    depth, face = np.zeros((B, H, W), dtype), np.full((B, H, W), -1, np.int32)
    occ, stats = np.zeros((B, NV), np.int32), np.zeros((B, 4), dtype)
    edge, gap = np.full((B, H, W), np.inf), np.full((B, H, W), np.inf)
    grow = 1 if with_margins else 0
    with np.errstate(all="ignore"):
        for b in range(B):
            sx, sy, iz, ok = project_host(Vb[b], np.asarray(cam)[b], None if M is None else np.asarray(M)[b], dtype)
            best, second, owner = np.full((H, W), np.inf, dtype), np.full((H, W), np.inf, dtype), np.full((H, W), -1, np.int32)
            for k, (i0, i1, i2) in enumerate(f.tolist()):
                if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= NV or i0 == i1 or i1 == i2 or i0 == i2 or not (ok[i0] and ok[i1] and ok[i2]):
                    continue
                area = _edge(sx, sy, i0, i1, sx[i2], sy[i2])
                if area == 0 or not np.isfinite(area):
                    continue
                xs, ys = sx[[i0, i1, i2]], sy[[i0, i1, i2]]
                x0, x1 = max(np.ceil(xs.min()) - grow, 0.0), min(np.floor(xs.max()) + grow, float(W - 1))  # clamped as floats, then converted
                y0, y1 = max(np.ceil(ys.min()) - grow, 0.0), min(np.floor(ys.max()) + grow, float(H - 1))
                if not (x0 <= x1 and y0 <= y1):
                    continue
                x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
                py, px = np.meshgrid(np.arange(y0, y1 + 1).astype(dtype), np.arange(x0, x1 + 1).astype(dtype), indexing="ij")
                w0, w1, w2 = _edge(sx, sy, i1, i2, px, py), _edge(sx, sy, i2, i0, px, py), _edge(sx, sy, i0, i1, px, py)
                inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) if area > 0 else ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
                tot = (w0 + w1) + w2
                izp = ((w0 / tot) * iz[i0] + (w1 / tot) * iz[i1]) + (w2 / tot) * iz[i2]
                d = one / izp
                cand = inside & np.isfinite(d) & (d > 0)
                win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
                if with_margins:
                    near = np.minimum(np.minimum(np.abs(w0), np.abs(w1)), np.abs(w2)) / abs(area)
                    edge[b][win] = np.minimum(edge[b][win], near)
                    dc = np.where(cand, d, np.inf)
                    second[win] = np.where(dc < best[win], best[win], np.minimum(second[win], dc))
                upd = cand & (d < best[win])
                best[win] = np.where(upd, d, best[win])
                owner[win] = np.where(upd, np.int32(k), owner[win])
            cov = owner >= 0
            depth[b], face[b] = np.where(cov, best, zero), owner
            gap[b] = np.where(np.isfinite(second), (second.astype(np.float64) - best) / np.where(cov, best, 1), np.inf)
            occ[b] = _occluded(sx, sy, ok, Vb[b][:, 2], depth[b], cov, margin, dtype)
            stats[b] = _stats(depth[b], cov, None if depth_obs is None else np.ascontiguousarray(depth_obs, dtype)[b], dtype)
    return (depth, face, occ, stats, edge, gap) if with_margins else (depth, face, occ, stats)


def _occluded(sx, sy, ok, z, depth, cov, margin, dtype):
    """the vertices more than `margin` behind the surface that owns their nearest pixel (floor(sx + 0.5), floor(sy + 0.5)), the window tested in float"""
    H, W = depth.shape
    with np.errstate(all="ignore"):
        c, r = np.floor(sx + dtype(0.5)), np.floor(sy + dtype(0.5))
        inwin = ok & (c >= 0) & (c <= dtype(W - 1)) & (r >= 0) & (r <= dtype(H - 1))
        ci, ri = np.where(inwin, c, 0).astype(np.int64), np.where(inwin, r, 0).astype(np.int64)
        return (inwin & cov[ri, ci] & (depth[ri, ci] < z - dtype(margin))).astype(np.int32)


def _stats(depth, cov, obs, dtype):
    """covered, observed (finite and > 0), both, the mean |d - d_obs| over both: summed per row in ascending column order, then over the rows"""
    zero = dtype(0)
    if obs is None:
        return np.asarray([cov.sum(), 0, 0, 0], dtype)
    with np.errstate(all="ignore"):
        seen = np.isfinite(obs) & (obs > 0)
        both = seen & cov
        total = zero
        for rr in range(depth.shape[0]):
            s = zero
            for cc in np.nonzero(both[rr])[0]:  # ascending columns
                s = dtype(s + np.abs(depth[rr, cc] - obs[rr, cc]))
            total = dtype(total + s)
        n = int(both.sum())
        return np.asarray([cov.sum(), seen.sum(), n, total / dtype(n) if n else zero], dtype)


def stats_host(depth, face, depth_obs, dtype=np.float32):
    """raster_host's `stats` [B, 4] for another depth_obs (or None), from its depth and face"""
    return np.stack([_stats(np.asarray(depth[b], dtype), np.asarray(face[b]) >= 0, None if depth_obs is None else np.ascontiguousarray(depth_obs, dtype)[b],
                            dtype) for b in range(len(depth))])


def occluded_host(verts, cam, M, depth, face, margin, dtype=np.float32):
    """raster_host's `occluded` [B, 778] for another margin, from its depth and face (the render does not depend on the margin)"""
    Vb = np.ascontiguousarray(verts, dtype)
    out = np.zeros(Vb.shape[:2], np.int32)
    for b in range(Vb.shape[0]):
        sx, sy, _, ok = project_host(Vb[b], np.asarray(cam)[b], None if M is None else np.asarray(M)[b], dtype)
        out[b] = _occluded(sx, sy, ok, Vb[b][:, 2], np.asarray(depth[b], dtype), np.asarray(face[b]) >= 0, margin, dtype)
    return out


def backproject_host(depth, cam, M):
    """preprocess.depth_to_pcl's rule in float64 for ONE hand: depth [H, W], cam [4], M [2, 3] or None -> xyz [H, W, 3]: crop pixel (c, r) is taken at
    (c + 0.5, r + 0.5, 1), mapped through inv(M) (3 x 3, last row 0 0 1), divided by its third entry, then x = (u - u0) / fx * d, y = (v - v0) / fy * d"""
    d = np.asarray(depth, np.float64)
    H, W = d.shape
    M3 = np.eye(3)
    if M is not None:
        M3[:2] = np.asarray(M, np.float64)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pts = np.stack([c + 0.5, r + 0.5, np.ones_like(c, np.float64)], -1).reshape(-1, 3)
    pts = np.dot(np.linalg.inv(M3), pts.T).T
    pts = pts[:, :2] / pts[:, 2:]
    fx, fy, u0, v0 = (float(x) for x in cam)
    dd = d.reshape(-1)
    return np.column_stack(((pts[:, 0] - u0) / fx * dd, (pts[:, 1] - v0) / fy * dd, dd)).reshape(H, W, 3)


# ----------------------------------------------------------------------------------------------------------------------------------------
# poses and crops
# ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def curl_poses():
    """float32 [2, 778, 3]: the surface model curled towards and away from the camera -- every chain's first joint at +0.6 (-0.6) rad about x, its second
    and third at +1.0 (-1.0) rad, zero shape, translation (30, -20, 600) mm"""
    aa = torch.zeros(2, 48, dtype=torch.float64)
    for i, sgn in enumerate((1.0, -1.0)):
        for chain in range(5):
            for s, ang in enumerate((0.6, 1.0, 1.0)):
                aa[i, (1 + chain * 3 + s) * 3] = sgn * ang
    tr = torch.tensor([30.0, -20.0, 600.0]).repeat(2, 1)
    return S.layer(S.surface_sd(), torch.float64, aa, torch.zeros(2, 10, dtype=torch.float64), tr)[0].float().contiguous()


def crop_for(verts, size, cube=250.0):
    """verts [B, 778, 3], size (H, W) -> (cam [B, 4], M [B, 2, 3]) float32: the camera (475, 475, 320, 240) and the map that puts a `cube` mm square,
    centred on the mesh's mean and at the mean's depth, onto the H x W window (the crop the preprocessing takes around the centre of mass)"""
    V = np.asarray(verts, np.float64)
    H, W = size
    fx, fy, u0, v0 = CAM
    mean = V.mean(1)
    uc, vc = mean[:, 0] * fx / mean[:, 2] + u0, mean[:, 1] * fy / mean[:, 2] + v0
    sx, sy = W / (cube * fx / mean[:, 2]), H / (cube * fy / mean[:, 2])
    M = np.zeros((V.shape[0], 2, 3))
    M[:, 0, 0], M[:, 0, 2] = sx, W / 2.0 - sx * uc
    M[:, 1, 1], M[:, 1, 2] = sy, H / 2.0 - sy * vc
    return np.tile(np.asarray(CAM, np.float32), (V.shape[0], 1)), M.astype(np.float32)


SIZES = ((128, 128), (32, 32), (16, 64), (1, 1))


@functools.lru_cache(maxsize=None)
def hands():
    """float32 [5, 778, 3]: surface_poses() then curl_poses()"""
    return np.concatenate([S.surface_poses().numpy(), curl_poses().numpy()])


@functools.lru_cache(maxsize=None)
def surface_faces():
    return S.faces_of(S.surface_sd())


@functools.lru_cache(maxsize=None)
def rendered(size, dtype_name="float32", with_M=True, margin=10.0):
    """raster_host of hands() in the crop_for window of `size`, with its margins -> (depth, face, occluded, stats, edge, gap), computed once"""
    v = hands()
    cam, M = crop_for(v, size)
    return raster_host(v, surface_faces(), cam, M if with_M else None, size[0], size[1], margin, None, getattr(np, dtype_name), with_margins=True)


def observed_from(depth):
    """a depth crop to compare a render with: `depth` [B, H, W] of OTHER poses (rolled by one hand), every 11th pixel NaN, every 7th 0, every 13th -5"""
    obs = np.roll(np.asarray(depth, np.float32), 1, axis=0).copy()
    flat = obs.reshape(obs.shape[0], -1)
    flat[:, 3::11] = np.nan
    flat[:, 1::7] = 0.0
    flat[:, 5::13] = -5.0
    return obs


# ----------------------------------------------------------------------------------------------------------------------------------------
# constructed scenes: identity M, camera (1, 1, 0, 0) at z = 1 puts a vertex (x, y, 1) at sx = x - 0.5
# ----------------------------------------------------------------------------------------------------------------------------------------
def _blank():
    return np.tile(np.asarray(PARKED, np.float32), (NV, 1))


def _at(c, r, z):
    """the vertex that projects exactly onto pixel (c, r) at depth z under UNIT (fx = fy = z-independent): x = (c + 0.5) z, y = (r + 0.5) z"""
    return ((c + 0.5) * z, (r + 0.5) * z, z)


UNIT = np.asarray([[1.0, 1.0, 0.0, 0.0]], np.float32)


def scene_two_plates():
    """a far plate over pixels 2..29 at 500 mm (vertices 0..3), a near plate over pixels 10..20 at 400 mm (vertices 4..7), and probe vertices in no face:
    8 and 9 on the far plate behind the near one, 10 and 11 on the far plate beside it, 12 on the near plate itself -> (verts [1, 778, 3], faces, H, W)"""
    v = _blank()
    v[0], v[1], v[2], v[3] = _at(2, 2, 500.0), _at(29, 2, 500.0), _at(29, 29, 500.0), _at(2, 29, 500.0)
    v[4], v[5], v[6], v[7] = _at(10, 10, 400.0), _at(20, 10, 400.0), _at(20, 20, 400.0), _at(10, 20, 400.0)
    v[8], v[9], v[10], v[11], v[12] = _at(15, 15, 500.0), _at(11, 19, 500.0), _at(5, 5, 500.0), _at(25, 15, 500.0), _at(15, 15, 400.0)
    faces = np.asarray([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    return v[None], faces, 32, 32


def scene_coincident():
    """faces 1 and 2 are the same triangle (another corner order, the other winding), face 0 a farther one under them, face 3 a nearer one beside them"""
    v = _blank()
    v[0], v[1], v[2] = _at(1, 1, 300.0), _at(12, 1, 300.0), _at(1, 12, 300.0)
    v[3], v[4], v[5] = _at(0, 0, 350.0), _at(14, 0, 350.0), _at(0, 14, 350.0)
    v[6], v[7], v[8] = _at(10, 10, 200.0), _at(15, 10, 200.0), _at(15, 15, 200.0)
    faces = np.asarray([[3, 4, 5], [0, 1, 2], [2, 1, 0], [6, 7, 8]], np.int32)
    return v[None], faces, 16, 16


def scene_grid():
    """a 5 x 5 lattice of vertices exactly on the pixel centres (0, 3, 6, 9, 12) at 256 mm (every product exact in float32), two triangles per cell with the
    diagonals alternating: every pixel of 0..12 lies in the mesh, those on shared edges and at shared vertices included"""
    v = _blank()
    idx = lambda i, j: i * 5 + j  # noqa: E731
    for i in range(5):
        for j in range(5):
            v[idx(i, j)] = _at(3 * j, 3 * i, 256.0)
    faces = []
    for i in range(4):
        for j in range(4):
            a, b, c, d = idx(i, j), idx(i, j + 1), idx(i + 1, j + 1), idx(i + 1, j)
            faces += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[b, c, d], [d, a, b]]
    return v[None], np.asarray(faces, np.int32), 16, 16


def scene_skipped():
    """one good face (0) and, nearer and over the same pixels, faces that must be skipped: a repeated vertex, an index of 778, an index of -1, a vertex at
    z = 0, one at z < 0, one NaN, one at infinity"""
    v = _blank()
    v[0], v[1], v[2] = _at(1, 1, 300.0), _at(12, 1, 300.0), _at(1, 12, 300.0)
    v[3], v[4], v[5] = _at(0, 0, 100.0), _at(14, 0, 100.0), _at(0, 14, 100.0)
    v[6] = (7.0, 7.0, 0.0)
    v[7] = (7.0, 7.0, -100.0)
    v[8] = (np.nan, 7.0, 100.0)
    v[9] = (7.0, np.inf, 100.0)
    faces = np.asarray([[0, 1, 2], [3, 4, 4], [3, 4, 778], [3, -1, 5], [3, 4, 6], [3, 7, 5], [8, 4, 5], [3, 4, 9]], np.int32)
    return v[None], faces, 16, 16


def scene_window():
    """face 0 half outside the window (to the left and above), face 1 entirely outside (to the right), face 2 with a vertex at z = 1e-3 mm that projects
    to about 1e9 pixels, face 3 far out on the negative side"""
    v = _blank()
    v[0], v[1], v[2] = _at(-6, -4, 300.0), _at(9, 3, 300.0), _at(2, 11, 300.0)
    v[3], v[4], v[5] = _at(20, 2, 200.0), _at(30, 2, 200.0), _at(25, 9, 200.0)
    v[6], v[7], v[8] = _at(3, 3, 250.0), _at(8, 12, 250.0), (1.0e6, 5.0e5, 1.0e-3)
    v[9], v[10], v[11] = _at(-3.0e9, -2.0e9, 100.0), _at(-3.0e9 + 4.0e3, -2.0e9, 100.0), _at(-3.0e9, -2.0e9 + 4.0e3, 100.0)
    faces = np.asarray([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]], np.int32)
    return v[None], faces, 16, 16


def scene_limits(F):
    """F faces: small triangles drawn at random over a 24 x 24 window at depths 200..300 mm from 600 random vertices (F = 2048, the most the entry takes),
    or for F = 1 one triangle over a third of the window"""
    rng = np.random.Generator(np.random.PCG64([16, F]))
    v = _blank()
    for i in range(600):
        v[i] = _at(24.0 * rng.random(), 24.0 * rng.random(), 200.0 + 100.0 * rng.random())
    order = np.argsort(v[:600, 0] / v[:600, 2] + 0.3 * v[:600, 1] / v[:600, 2])  # neighbours in the order are near in the image: small faces
    if F == 1:
        v[600], v[601], v[602] = _at(2, 3, 250.0), _at(20, 5, 260.0), _at(8, 21, 240.0)
        return v[None], np.asarray([[600, 601, 602]], np.int32), 24, 24
    start = rng.integers(0, 596, F)
    faces = np.stack([order[start], order[start + 1 + rng.integers(0, 2, F)], order[start + 3]], -1).astype(np.int32)
    return v[None], faces, 24, 24


def scene_threshold():
    """the kernel walks a face whose pixel box holds up to 64 pixels in one thread and hands a larger one to a wave: face 0 has a box of 8 x 8 = 64 pixels,
    face 1 one of 13 x 5 = 65, and face 2 (9 x 9 = 81, nearer in part) lies over face 0, so that the two paths contest the same pixels"""
    v = _blank()
    v[0], v[1], v[2] = _at(1, 1, 300.0), _at(8, 1, 300.0), _at(1, 8, 300.0)
    v[3], v[4], v[5] = _at(10, 1, 300.0), _at(22, 1, 300.0), _at(10, 5, 300.0)
    v[6], v[7], v[8] = _at(0, 0, 250.0), _at(8, 0, 350.0), _at(0, 8, 350.0)
    return v[None], np.asarray([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32), 12, 24


SCENES = {"threshold": scene_threshold, "two_plates": scene_two_plates, "coincident": scene_coincident, "grid": scene_grid, "skipped": scene_skipped, "window": scene_window,
          "one_face": lambda: scene_limits(1), "most_faces": lambda: scene_limits(2048)}


@functools.lru_cache(maxsize=None)
def scene_render(name, dtype_name="float32", margin=10.0):
    """(verts, faces, H, W, raster_host's four outputs in the dtype) of a constructed scene under UNIT and the identity map"""
    v, f, H, W = SCENES[name]()
    return v, f, H, W, raster_host(v, f, UNIT, None, H, W, margin, None, getattr(np, dtype_name))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the association with a vertex mask
# ----------------------------------------------------------------------------------------------------------------------------------------
def associate_vis_mask_host(points, weight, verts, normals, vert_mask, max_dist2, facing_min=0.0, dtype=np.float32):
    """kpf_mano_assoc_vis_mask_f32 in numpy: mano_surface_cases.associate_vis_host whose candidates also need vert_mask[v] != 0 (None: no mask).  The
    facing rule looks at a normal only through "finite, not all-zero, n . V < -facing_min |V|", so a masked vertex is restated as one with a zero normal;
    no matched point's vertex is masked, so the plane distances read the true normals."""
    if vert_mask is None:
        return S.associate_vis_host(points, weight, verts, normals, max_dist2, facing_min, dtype)
    Nm = np.ascontiguousarray(normals, dtype)
    hidden = np.where((np.asarray(vert_mask) != 0)[..., None], Nm, dtype(0))
    return S.associate_vis_host(points, weight, verts, hidden, max_dist2, facing_min, dtype)


# ----------------------------------------------------------------------------------------------------------------------------------------
# what float64 says about the mask
# ----------------------------------------------------------------------------------------------------------------------------------------
def sensor_cloud(verts, faces, size=(128, 128), N=1024, sigma=0.5, seed=47):
    """the cloud that IS the sensor's view of `verts` [B, 778, 3]: N of the covered pixels of the mesh's float64 render, back-projected, + sigma mm of
    noise -> float32 [B, N, 3] (self-occluded surface is absent from it, which one_sided_cloud's is not)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cam, M = crop_for(verts, size)
    depth, face, _, _ = raster_host(verts, faces, cam, M, size[0], size[1], 10.0, None, np.float64)
    out = np.zeros((len(verts), N, 3))
    for b in range(len(verts)):
        xyz = backproject_host(depth[b], cam[b], M[b])[face[b] >= 0]
        out[b] = xyz[rng.choice(len(xyz), N, replace=len(xyz) < N)] + sigma * rng.standard_normal((N, 3))
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def curl_inputs():
    """B = 2, the curled hands as a fit_cloud problem: the true mesh (curl_poses()), joint targets = the truth + 0.1 mm, unit weights, the start `near`
    (the truth + 0.1 in pose, shape and translation), the sensor's cloud, and the 128 x 128 crop_for camera and map"""
    import mano_cases as Mc
    gen = torch.Generator().manual_seed(48)
    aa = torch.zeros(2, 48, dtype=torch.float64)
    for i, sgn in enumerate((1.0, -1.0)):
        for chain in range(5):
            for s, ang in enumerate((0.6, 1.0, 1.0)):
                aa[i, (1 + chain * 3 + s) * 3] = sgn * ang
    tr = torch.tensor([30.0, -20.0, 600.0], dtype=torch.float64).repeat(2, 1)
    c = Mc.Case()
    c.verts = curl_poses()
    joints = S.layer(S.surface_sd(), torch.float64, aa, torch.zeros(2, 10), tr)[1]
    c.target = (joints + 0.1 * torch.randn(2, 21, 3, generator=gen, dtype=torch.float64)).float().contiguous()
    c.weight = torch.ones(2, 21)
    noise = lambda n: 0.1 * torch.randn(2, n, generator=gen, dtype=torch.float64)  # noqa: E731
    c.near = ((aa + noise(48)).float(), noise(10).float(), (tr + noise(3)).float())
    c.cloud = torch.from_numpy(sensor_cloud(c.verts.numpy(), surface_faces()))
    c.cam, c.M = (torch.from_numpy(x) for x in crop_for(c.verts.numpy(), (128, 128)))
    return c


def fit_cloud_curl_reference(masked, rounds=6, iters=50, iters_cloud=2, max_dist=20.0, size=(128, 128), margin=10.0):
    """mano_surface_cases.fit_cloud_surface_reference("plane") in float64 on curl_inputs(), with (masked) or without the z-buffer's mask on the
    association -> the mean error of all 778 vertices per hand, mm"""
    c, sd, faces = curl_inputs(), S.surface_sd(), surface_faces()
    pts, cam, M = c.cloud.numpy(), c.cam.numpy(), c.M.numpy()
    state = S.adam_joint_fit(torch.float64, sd, c.target, c.weight, c.near, iters)
    verts = S.layer(sd, torch.float64, *state)[0]
    for _ in range(rounds):
        v32 = verts.float().numpy()
        nrm = S.normals_host(v32, faces)
        mask = 1 - raster_host(v32, faces, cam, M, size[0], size[1], margin)[2] if masked else None
        a = associate_vis_mask_host(pts, None, v32, nrm, mask, max_dist * max_dist)
        out = S.fit_mesh_gn_plane_reference(torch.float64, c.target, c.weight, torch.from_numpy(a[1]), torch.from_numpy(a[2]), torch.from_numpy(nrm), state,
                                            iters_cloud, init_trans=False, sd=sd)
        state, verts = (out["pose_aa"], out["betas"], out["trans"]), out["verts"]
    return (verts.double() - c.verts.double()).norm(dim=-1).mean(1)
