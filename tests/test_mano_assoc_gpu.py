"""kpf_mano_assoc_f32: depth points -> nearest vertex, per-vertex centroid and weight, stats.  The kernel is held to the BITS of the numpy-float32 restatement
(tests/mano_mesh_cases.py::associate_host, itself checked against float64 and hand-made cases in test_mano_mesh_host.py): idx, vert_target, vert_weight and
stats are compared with array_equal, never with a tolerance."""
import numpy as np
import pytest
import torch

import mano_mesh_cases as MM
from test_heads_gpu import _dev

pytestmark = pytest.mark.gpu
NAMES = ("idx", "vert_target", "vert_weight", "stats")


def _assoc(dev, pts, w, verts, gate2, fill=None, N=None):
    """the raw entry (max_dist2 as given; N: the count passed, if not the points') -> (return code, cpu numpy outputs in the order of NAMES)"""
    from keypointfusion_amd import lib as L
    B = pts.shape[0]
    N = pts.shape[1] if N is None else N
    p, v = pts.to(dev).contiguous(), verts.to(dev).contiguous()
    pw = None if w is None else w.to(dev).contiguous()
    n = max(N, 1)
    out = [torch.empty(B, n, device=dev, dtype=torch.int32), torch.empty(B, MM.NV, 3, device=dev), torch.empty(B, MM.NV, device=dev), torch.empty(B, 2, device=dev)]
    if fill is not None:
        for o in out:
            o.fill_(fill)
    rc = L.load().kpf_mano_assoc_f32(p.data_ptr(), None if pw is None else pw.data_ptr(), v.data_ptr(), gate2, *[o.data_ptr() for o in out], B, N,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, [o.cpu().numpy() for o in out]


def _same(got, want, what):
    for name, g, h in zip(NAMES, got, want):
        assert np.array_equal(g, h, equal_nan=True), (what, name, int((g != h).sum()))


@pytest.mark.parametrize("gate2", [400.0, 4.0, 0.0, float("inf")])
@pytest.mark.parametrize("N", [1, 257, 1024])
def test_assoc_is_the_host_restatement_bit_for_bit(N, gate2):
    """B = 3; N = 1, 257 (no multiple of the workgroup) and 1024; 2 mm of noise on vertices drawn with replacement, so vertices collect several points, and every
    seventh weight is 0; gates of 20 mm, 2 mm (about half the points fall outside), 0 (exact hits only: none here) and none"""
    dev = _dev()
    pts, w = MM.sized_cloud(N)
    verts = MM.true_mesh()
    want = MM.associate_host(pts.numpy(), w.numpy(), verts.numpy(), gate2)
    rc, got = _assoc(dev, pts, w, verts, gate2)
    assert rc == 0
    print("MANO-ASSOC N %4d gate2 %6s matched %s mean mm %s" % (N, gate2, want[3][:, 0].tolist(), want[3][:, 1].tolist()))
    _same(got, want, (N, gate2))
    if N == 1024 and gate2 == 400.0:  # the case does put several points on one vertex and leaves vertices empty
        assert float(want[2].max()) > 2.0 and int((want[2] == 0).sum()) > 0 and int((want[0] < 0).sum()) >= 3 * 146


def test_assoc_default_weights_are_ones():
    dev = _dev()
    pts, _ = MM.sized_cloud(257)
    verts = MM.true_mesh()
    rc, got = _assoc(dev, pts, None, verts, 400.0)
    assert rc == 0
    _same(got, MM.associate_host(pts.numpy(), None, verts.numpy(), 400.0), "ones")
    _same(got, _assoc(dev, pts, torch.ones(3, 257), verts, 400.0)[1], "ones given")


@pytest.mark.parametrize("gate2", [400.0, 0.0, float("inf")])
def test_assoc_hand_made_cases(gate2):
    """two points on one vertex, a gated point, a NaN point, a zero-weight point, an exact tie (the lower index wins), an exact hit"""
    dev = _dev()
    p, w, verts = MM.hand_made()
    want = MM.associate_host(p.numpy(), w.numpy(), verts.numpy(), gate2)
    rc, got = _assoc(dev, p, w, verts, gate2)
    assert rc == 0
    _same(got, want, gate2)
    assert got[0][0].tolist() == {400.0: [5, 5, -1, -1, -1, 700, 12], 0.0: [-1, -1, -1, -1, -1, 700, 12]}.get(gate2, got[0][0].tolist())
    if gate2 == float("inf"):
        assert got[0][0, 2] >= 0 and got[0][0, 3] == -1 and got[0][0, 4] == -1


@pytest.mark.parametrize("N", [0, 4097])
def test_assoc_refuses_a_point_count_outside_1_to_4096_and_writes_nothing(N):
    dev = _dev()
    pts = torch.zeros(1, 4097, 3)
    rc, got = _assoc(dev, pts, None, MM.true_mesh()[:1], 400.0, fill=7, N=N)
    assert rc != 0
    for g in got:
        assert bool((g == 7).all())


def test_assoc_rows_do_not_depend_on_the_batch():
    dev = _dev()
    pts, w = MM.sized_cloud(257)
    verts = MM.true_mesh()
    _, all3 = _assoc(dev, pts, w, verts, 400.0)
    for b in range(3):
        _, one = _assoc(dev, pts[b:b + 1], w[b:b + 1], verts[b:b + 1], 400.0)
        _same(one, [a[b:b + 1] for a in all3], b)


def test_associate_wrapper_and_the_largest_cloud():
    """ManoFitter.associate (max_dist in mm, squared inside) at N = 4096, the largest the entry takes: every LDS slot of the point arrays is in use"""
    dev = _dev()
    from keypointfusion_amd.mano_fit import ManoFitter
    import mano_cases as M
    pts, w = MM.sized_cloud(4096)
    pts, w, verts = pts[:1], w[:1], MM.true_mesh()[:1]
    out = ManoFitter(M.model_sd(), dev).associate(pts.to(dev), verts.to(dev), w.to(dev), max_dist=5.0)
    want = MM.associate_host(pts.numpy(), w.numpy(), verts.numpy(), 25.0)
    _same([out[k].cpu().numpy() for k in NAMES], want, "wrapper")
