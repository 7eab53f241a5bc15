"""kpf_mano_assoc_vis_f32 / ManoFitter.associate(normals=...): the association over the vertices that face the camera.  The kernel is held to the BITS of the
numpy-float32 restatement (tests/mano_surface_cases.py::associate_vis_host, checked against float64 in test_mano_surface_host.py): idx, vert_target,
vert_weight, visible and stats are compared with array_equal, never with a tolerance.  B = 3."""
import functools

import numpy as np
import pytest
import torch

import mano_cases as M
import mano_mesh_cases as MM
import mano_surface_cases as S
from test_heads_gpu import _dev

pytestmark = pytest.mark.gpu
NAMES = ("idx", "vert_target", "vert_weight", "visible", "stats")


def _assoc(dev, pts, w, verts, normals, gate2, facing=0.0, fill=None, N=None):
    """the raw entry -> (return code, cpu numpy outputs in the order of NAMES)"""
    from keypointfusion_amd import lib as L
    pts, verts, normals = torch.as_tensor(pts), torch.as_tensor(verts), torch.as_tensor(normals)
    B = pts.shape[0]
    N = pts.shape[1] if N is None else N
    p, v, nm = pts.to(dev).contiguous(), verts.to(dev).contiguous(), normals.to(dev).contiguous()
    pw = None if w is None else torch.as_tensor(w).to(dev).contiguous()
    out = [torch.empty(B, max(N, 1), device=dev, dtype=torch.int32), torch.empty(B, S.NV, 3, device=dev), torch.empty(B, S.NV, device=dev),
           torch.empty(B, S.NV, device=dev, dtype=torch.int32), torch.empty(B, 4, device=dev)]
    if fill is not None:
        for o in out:
            o.fill_(fill)
    rc = L.load().kpf_mano_assoc_vis_f32(p.data_ptr(), None if pw is None else pw.data_ptr(), v.data_ptr(), nm.data_ptr(), gate2, facing,
                                         *[o.data_ptr() for o in out], B, N, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, [o.cpu().numpy() for o in out]


def _same(got, want, what):
    for name, g, h in zip(NAMES, got, want):
        assert np.array_equal(g, h, equal_nan=True), (what, name, int((g != h).sum()))


@functools.lru_cache(maxsize=None)
def _surface():
    """the surface model's mesh at three poses, its fp32 normals, and per N a cloud on its camera side with weights (every seventh 0)"""
    verts = S.surface_poses().numpy()
    return verts, S.normals_host(verts, S.faces_of(S.surface_sd()))


@functools.lru_cache(maxsize=None)
def _cloud(N):
    verts, _ = _surface()
    pts = S.one_sided_cloud(verts, S.faces_of(S.surface_sd()), N=N, sigma=2.0, seed=50 + N).numpy()
    rng = np.random.Generator(np.random.PCG64(60 + N))
    w = (2.0 * rng.random((3, N)) + 2.0 ** -10).astype(np.float32)
    w[:, 3::7] = 0.0
    return pts, w


@pytest.mark.parametrize("facing", [0.0, 0.5])
@pytest.mark.parametrize("gate2", [400.0, 0.0, float("inf")])
@pytest.mark.parametrize("N", [1, 257, 1024])
def test_assoc_vis_is_the_host_restatement_bit_for_bit(N, gate2, facing):
    dev = _dev()
    verts, nrm = _surface()
    pts, w = _cloud(N)
    want = S.associate_vis_host(pts, w, verts, nrm, gate2, facing)
    rc, got = _assoc(dev, pts, w, verts, nrm, gate2, facing)
    assert rc == 0
    print("MANO-ASSOC-VIS N %4d gate2 %6s facing %.1f stats %s" % (N, gate2, facing, want[4].tolist()))
    _same(got, want, (N, gate2, facing))
    if N == 1024 and gate2 == 400.0:  # the case is not empty: points are matched, vertices are hidden, and fewer face the camera at 0.5
        assert bool((want[4][:, 0] > 600).all()) and bool((want[4][:, 3] < 600).all()) and bool((want[4][:, 3] > 100).all())
        assert bool((want[4][:, 2] <= want[4][:, 1]).all())


def test_assoc_vis_hand_made_cases():
    """every normal facing away; a tie won by the lower visible index; a nearer hidden vertex that loses to a farther visible one; NaN and zero-weight
    points"""
    dev = _dev()
    verts, nrm = _surface()
    verts, nrm = verts[:1].copy(), nrm[:1].copy()
    pts, w = _cloud(257)
    pts, w = pts[:1], w[:1]
    # all normals facing away (the unit vector from the camera to the vertex): nothing is visible, every idx is -1
    away = (verts / np.linalg.norm(verts, axis=-1, keepdims=True)).astype(np.float32)
    rc, got = _assoc(dev, pts, w, verts, away, float("inf"))
    assert rc == 0
    _same(got, S.associate_vis_host(pts, w, verts, away, np.inf), "away")
    assert bool((got[0] == -1).all()) and not got[3].any() and got[4][0].tolist() == [0.0, 0.0, 0.0, 0.0] and not got[1].any() and not got[2].any()
    # towards the camera everywhere: all visible
    rc, got = _assoc(dev, pts, w, verts, -away, 400.0)
    assert rc == 0 and bool((got[3] == 1).all()) and got[4][0, 3] == 778.0
    # hand-made points against three vertices put in known places
    v = verts.copy()
    n = (-away).copy()
    v[0, 700] = v[0, 701] = v[0, 702]          # a triple tie ...
    n[0, 700] = away[0, 700]                   # ... whose lowest index is hidden: 701 wins
    n[0, 12] = 0.0                             # a zero normal hides vertex 12
    n[0, 20, 1] = np.nan                       # and a NaN normal vertex 20
    p = np.zeros((1, 6, 3), np.float32)
    p[0, 0] = v[0, 700]                        # the tie
    p[0, 1] = v[0, 12]                         # exactly on the hidden 12: goes to a farther visible vertex
    p[0, 2] = v[0, 20]                         # exactly on the hidden 20: likewise
    p[0, 3] = v[0, 40]
    p[0, 3, 0] = np.nan                        # a NaN point
    p[0, 4] = v[0, 50]                         # weight 0
    p[0, 5] = v[0, 60] + np.float32(0.25)      # an ordinary point
    pw = np.array([[1.0, 2.0, 1.0, 1.0, 0.0, 3.0]], np.float32)
    want = S.associate_vis_host(p, pw, v, n, np.inf)
    rc, got = _assoc(dev, p, pw, v, n, float("inf"))
    assert rc == 0
    _same(got, want, "hand made")
    idx = got[0][0].tolist()
    assert idx[0] == 701 and idx[1] not in (-1, 12) and idx[2] not in (-1, 20) and idx[3:5] == [-1, -1] and idx[5] == 60
    assert got[3][0, [700, 12, 20]].tolist() == [0, 0, 0] and got[4][0, 0] == 4.0 and got[4][0, 3] == 775.0
    # at gate 0 only exact hits on visible vertices stay
    rc, got = _assoc(dev, p, pw, v, n, 0.0)
    assert rc == 0 and got[0][0].tolist() == [701, -1, -1, -1, -1, -1]
    _same(got, S.associate_vis_host(p, pw, v, n, 0.0), "gate 0")


def test_with_every_vertex_visible_the_bits_are_the_associations():
    """the synthetic hand's cloud and mesh of test_mano_assoc_gpu.py with normals that all face the camera: idx, targets, weights and stats[:2] are
    kpf_mano_assoc_f32's"""
    dev = _dev()
    from keypointfusion_amd.mano_fit import ManoFitter
    pts, w = MM.sized_cloud(257)
    verts = MM.true_mesh()
    toward = -(verts / verts.norm(dim=-1, keepdim=True))
    f = ManoFitter(M.model_sd(), dev)
    p, pw, v, nm = (t.to(dev).contiguous() for t in (pts, w, verts, toward))
    old = {k: t.cpu().numpy() for k, t in f.associate(p, v, pw, max_dist=20.0).items()}
    new = {k: t.cpu().numpy() for k, t in f.associate(p, v, pw, max_dist=20.0, normals=nm).items()}
    assert set(old) == {"idx", "vert_target", "vert_weight", "stats"} and set(new) == set(old) | {"visible"}
    for k in ("idx", "vert_target", "vert_weight"):
        assert np.array_equal(new[k], old[k]), k
    assert old["stats"].shape == (3, 2) and new["stats"].shape == (3, 4) and np.array_equal(new["stats"][:, :2], old["stats"])
    assert bool((new["visible"] == 1).all()) and bool((new["stats"][:, 3] == 778).all())
    _same([new[k] for k in NAMES], S.associate_vis_host(pts.numpy(), w.numpy(), verts.numpy(), toward.numpy(), 400.0), "wrapper")
    with pytest.raises(ValueError):
        f.associate(p, v, pw, normals=nm, facing_min=1.0)


@pytest.mark.parametrize("N,facing", [(0, 0.0), (4097, 0.0), (16, 1.0)])
def test_assoc_vis_refuses_and_writes_nothing(N, facing):
    dev = _dev()
    verts, nrm = _surface()
    rc, got = _assoc(dev, np.zeros((1, 4097, 3), np.float32), None, verts[:1], nrm[:1], 400.0, facing, fill=7, N=N)
    assert rc != 0
    for g in got:
        assert bool((g == 7).all())


def test_assoc_vis_rows_do_not_depend_on_the_batch_and_the_largest_cloud():
    dev = _dev()
    verts, nrm = _surface()
    pts, w = _cloud(257)
    _, all3 = _assoc(dev, pts, w, verts, nrm, 400.0, 0.5)
    for b in range(3):
        _, one = _assoc(dev, pts[b:b + 1], w[b:b + 1], verts[b:b + 1], nrm[b:b + 1], 400.0, 0.5)
        _same(one, [a[b:b + 1] for a in all3], b)
    # N = 4096, the most the entry takes: every LDS slot of the point arrays is in use
    big = S.one_sided_cloud(verts[:1], S.faces_of(S.surface_sd()), N=4096, sigma=2.0, seed=70).numpy()
    rc, got = _assoc(dev, big, None, verts[:1], nrm[:1], 400.0)
    assert rc == 0
    _same(got, S.associate_vis_host(big, None, verts[:1], nrm[:1], 400.0), "N = 4096")
