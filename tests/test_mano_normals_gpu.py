"""kpf_mano_normals_f32 / ManoFitter.normals: area-weighted vertex normals.  The kernel is held to the BITS of the numpy-float32 restatement
(tests/mano_surface_cases.py::normals_host, itself checked against float64 in test_mano_surface_host.py): array_equal, never a tolerance.  B = 3."""
import numpy as np
import pytest
import torch

import mano_cases as M
import mano_mesh_cases as MM
import mano_surface_cases as S
from test_heads_gpu import _dev

pytestmark = pytest.mark.gpu


def _normals(dev, verts, faces, sign=1.0, fill=None, F=None):
    """the raw entry -> (return code, normals as cpu numpy)"""
    from keypointfusion_amd import lib as L
    v = torch.as_tensor(verts).to(dev).contiguous()
    f = torch.as_tensor(np.ascontiguousarray(faces, np.int32)).to(dev).contiguous()
    out = torch.empty(v.shape[0], S.NV, 3, device=dev)
    if fill is not None:
        out.fill_(fill)
    rc = L.load().kpf_mano_normals_f32(v.data_ptr(), f.data_ptr(), f.shape[0] if F is None else F, sign, out.data_ptr(), v.shape[0],
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy()


def _bits(got, want, what):
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


def test_normals_are_the_host_restatement_bit_for_bit():
    """the surface model at three poses (every vertex in six or eight faces), and the synthetic hand, whose 1538 random faces repeat vertices, cancel, and
    leave vertices out"""
    dev = _dev()
    for name, verts, faces in (("surface", S.surface_poses().numpy(), S.faces_of(S.surface_sd())), ("synthetic", MM.true_mesh().numpy(), S.faces_of(M.model_sd()))):
        want = S.normals_host(verts, faces)
        rc, got = _normals(dev, verts, faces)
        assert rc == 0
        _bits(got, want, name)
        ln = np.linalg.norm(want.astype(np.float64), axis=-1)
        zero = ~want.any(-1)
        print("MANO-NORMALS %-9s F %d zero normals %d" % (name, len(faces), int(zero.sum())))
        assert np.allclose(ln[~zero], 1, atol=1e-6)
        for sign in (-1.0,):
            rc, neg = _normals(dev, verts, faces, sign)
            assert rc == 0
            assert np.array_equal(neg, -want), (name, "sign")  # the exact negation (a zero normal stays +0)
            _bits(neg, S.normals_host(verts, faces, sign), (name, "sign, host"))
    assert int((~S.normals_host(MM.true_mesh().numpy(), S.faces_of(M.model_sd())).any(-1)).sum()) > 0  # the random faces do leave vertices out


def test_normals_hand_made_cases():
    dev = _dev()
    verts = S.surface_poses().numpy().copy()
    faces = S.faces_of(S.surface_sd())
    # F = 1: three unit normals, zeros elsewhere
    rc, got = _normals(dev, verts, faces[:1])
    assert rc == 0
    _bits(got, S.normals_host(verts, faces[:1]), "F = 1")
    used = np.zeros(S.NV, bool)
    used[faces[0]] = True
    assert not got[:, ~used].any() and bool(got[:, used].any(-1).all())
    assert np.array_equal(got[:, faces[0, 0]], got[:, faces[0, 1]]) and np.array_equal(got[:, faces[0, 0]], got[:, faces[0, 2]])
    # F = 2048, the most the entry takes: the model's faces, then repeats of them, a face with a repeated vertex, out-of-range indices
    rng = np.random.Generator(np.random.PCG64(5))
    big = np.concatenate([faces, faces[rng.integers(0, len(faces), 2048 - len(faces))]]).astype(np.int32)
    big[1600] = (5, 5, 9)         # a repeated vertex: a zero face normal, added twice to vertex 5
    big[1601] = (3, 778, 4)       # out of range: skipped
    big[1602] = (-1, 3, 4)
    big[1603] = (3, 4, 1 << 30)
    want = S.normals_host(verts, big)
    rc, got = _normals(dev, verts, big)
    assert rc == 0
    _bits(got, want, "F = 2048")
    without = np.delete(big, [1601, 1602, 1603], 0)
    _bits(S.normals_host(verts, without), want, "host: skipped faces change nothing")
    # a vertex in no face -> zeros; a NaN vertex poisons exactly the vertices of its own faces (their sums are not finite: zeros), no other
    some = faces[~(faces == 100).any(1)]
    bad = verts.copy()
    bad[1, 300, 1] = np.nan
    want = S.normals_host(bad, some)
    rc, got = _normals(dev, bad, some)
    assert rc == 0
    _bits(got, want, "NaN vertex")
    clean = S.normals_host(verts, some)
    touched = np.zeros(S.NV, bool)
    touched[np.unique(some[(some == 300).any(1)])] = True
    assert not got[:, 100].any() and not got[1, touched].any() and bool(np.isfinite(got).all())
    assert np.array_equal(got[1, ~touched], clean[1, ~touched]) and np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])


@pytest.mark.parametrize("F,sign", [(0, 1.0), (2049, 1.0), (8, 0.0)])
def test_normals_refuse_and_write_nothing(F, sign):
    dev = _dev()
    rc, got = _normals(dev, S.surface_poses()[:1], np.zeros((2049, 3), np.int32), sign, fill=7, F=F)
    assert rc != 0 and bool((got == 7).all())


def test_normals_rows_repeat_and_replay():
    """B = 1 rows against B = 3, a repeat, and ManoFitter.normals eager against a captured graph replayed twice"""
    dev = _dev()
    verts, faces = S.surface_poses(), S.faces_of(S.surface_sd())
    _, all3 = _normals(dev, verts, faces)
    _, again = _normals(dev, verts, faces)
    _bits(again, all3, "repeat")
    for b in range(3):
        _, one = _normals(dev, verts[b:b + 1], faces)
        _bits(one, all3[b:b + 1], b)
    from keypointfusion_amd.mano_fit import ManoFitter
    f = ManoFitter(S.surface_sd(), dev)
    assert f.faces.dtype == torch.int32 and tuple(f.faces.shape) == (1552, 3) and f.faces.is_cuda
    v = verts.to(dev).contiguous()
    _bits(f.normals(v).cpu().numpy(), all3, "wrapper")
    assert np.array_equal(f.normals(v, sign=-1.0).cpu().numpy(), -all3)
    with pytest.raises(ValueError):
        f.normals(v, sign=2.0)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        f.normals(v)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = f.normals(v)
    torch.cuda.current_stream(dev).wait_stream(side)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        _bits(out.cpu().numpy(), all3, "replay")
