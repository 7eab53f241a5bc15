"""Inputs for the on-device overlay (kpf_overlay_project_f32, kpf_overlay_draw_u8; overlay.FrameOverlay).  No GPU.

The yardstick is keypointfusion_amd.overlay.draw_host, the numpy-float32 restatement of both launches: the kernels are held to its bits, and it is itself
checked against hand-computed pixel sets in test_overlay_host.py.  The grid is 70 x 100: two by two tiles of 64 x 64 with partial tiles at both edges.
The hands are the synthetic hand model's three meshes with its (random) faces: tens of faces contest every pixel, and every large face crosses a seam."""
import functools

import numpy as np

import mano_cases as M
import mano_mesh_cases as MM
import mano_surface_cases as S
from keypointfusion_amd import overlay as O

H, W, F = 70, 100, 2
FRAME_INDEX = (0, 0, 1)
# hand 0 sits on the crossing of the tile seams (column 64, row 64) and runs off the bottom of the grid; hand 1 shares frame 0, overlaps hand 0 and is
# 60 mm nearer; hand 2 is alone on frame 1
CAMS = np.asarray([[180.0, 180.0, 55.0, 70.0], [180.0, 180.0, 62.0, 52.0], [200.0, 190.0, 40.0, 36.0]], np.float32)
SHIFT = np.asarray([[0.0, 0.0, 0.0], [0.0, 0.0, -60.0], [0.0, 0.0, 0.0]], np.float32)


def faces():
    return S.faces_of(M.model_sd())


@functools.lru_cache(maxsize=None)
def full_case():
    """dict of numpy arrays: rgb [2, 70, 100, 3], verts3d, normals [3, 778, 3], cam [3, 4], joints_px [3, 21, 3], depth_zero [2, 70, 100] uint16"""
    rng = np.random.Generator(np.random.PCG64(190))
    verts = (MM.true_mesh().numpy() + SHIFT[:, None]).astype(np.float32)
    joints = (M.fit_inputs().target.numpy() + SHIFT[:, None]).astype(np.float32)
    jp = np.stack([joints[..., 0] * CAMS[:, None, 0] / joints[..., 2] + CAMS[:, None, 2], joints[..., 1] * CAMS[:, None, 1] / joints[..., 2] + CAMS[:, None, 3],
                   joints[..., 2]], -1).astype(np.float32)
    return dict(rgb=rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8), verts3d=verts, normals=S.normals_host(verts, faces()), cam=CAMS.copy(), joints_px=jp,
                depth_zero=np.zeros((F, H, W), np.uint16))


def host(c, **kw):
    """draw_host on a case's arrays with the full case's frame_index, faces and defaults; kw replaces or adds arguments"""
    args = dict(rgb=c["rgb"], faces=faces(), verts3d=c["verts3d"], cam=c["cam"], normals=c["normals"], joints_px=c["joints_px"], frame_index=FRAME_INDEX)
    args.update(kw)
    return O.draw_host(**args)


@functools.lru_cache(maxsize=None)
def full_host():
    """draw_host of the full case, computed once and left unchanged"""
    return host(full_case())


def subset(c, rows):
    """the case's per-hand arrays restricted to `rows`"""
    out = dict(c)
    for k in ("verts3d", "normals", "cam", "joints_px"):
        out[k] = np.ascontiguousarray(c[k][list(rows)])
    return out


OUTPUTS = ("image", "label", "owner", "prim", "depth")
PROJECT = ("sx", "sy", "iz", "shade", "ok", "rect")


def same(got, want, what, names=OUTPUTS):
    """bit equality of every named output: floats are compared through their bits, so that signed zeros and the last bit count; a NaN (launch 1's sx of a
    NaN vertex: no drawn output can hold one) must face a NaN, its payload is not part of the rule"""
    for k in names:
        g, h = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == h.dtype and g.shape == h.shape, (what, k, g.dtype, h.dtype, g.shape, h.shape)
        if g.dtype == np.float32:
            nan = np.isnan(g) & np.isnan(h)
            g, h = np.where(nan, 0, g.view(np.uint32)), np.where(nan, 0, h.view(np.uint32))
        assert np.array_equal(g, h), (what, k, int((g != h).sum()))
