// What the two z-buffer renders share (kpf_mano_surface.hip: kpf_mano_raster_f32, one hand into its crop; kpf_overlay.hip: kpf_overlay_draw_u8, every hand
// of a frame into 64 x 64 tiles): the edge function, a face ready to be walked, and the inside rule with the depth at a pixel.  Private to csrc; everything
// is in an unnamed namespace.  Every operation individually rounded: tests/mano_raster_cases.py::raster_host gives the same bits.
#pragma once
#include <math.h>

#include "kpf_common.h"

namespace {

constexpr int RASTER_NV = 778;
constexpr unsigned long long RASTER_EMPTY = ~0ull;
constexpr int RASTER_SMALL = 64;  // a face whose pixel box holds up to this many pixels is walked by its own thread, a larger one by a whole wave

// One directed edge a -> b, always evaluated from the lower vertex index: e = (sx[hi] - sx[lo]) (py - sy[lo]) - (sy[hi] - sy[lo]) (px - sx[lo]), negated
// if a > b.  The two faces at an edge get the same number with opposite signs, so with an inclusive test a pixel centre on the edge belongs to one of them.
struct RasterEdge {
  float dx, dy, ox, oy;
  bool neg;
  __device__ __forceinline__ void set(const float* sx, const float* sy, int a, int b) {
#pragma clang fp contract(off)
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    dx = __fsub_rn(sx[hi], sx[lo]);
    dy = __fsub_rn(sy[hi], sy[lo]);
    ox = sx[lo];
    oy = sy[lo];
    neg = a > b;
  }
  __device__ __forceinline__ float at(float px, float py) const {
#pragma clang fp contract(off)
    const float e = __fsub_rn(__fmul_rn(dx, __fsub_rn(py, oy)), __fmul_rn(dy, __fsub_rn(px, ox)));
    return neg ? -e : e;
  }
};

// One face ready to be walked: its three edges (w0, w1, w2 are the weights of v0, v1, v2), the vertices' 1 / z, the sign of its area, its vertex indices
// and its pixel box
struct RasterFace {
  RasterEdge e0, e1, e2;
  float iz0, iz1, iz2;
  bool pos;
  int i0, i1, i2;
  int x0, x1, y0, y1;
  // false: the face is skipped (an index outside 0..777, a repeated one, a vertex that is not finite or has z <= 0, no area, no pixel).  The pixel box is
  // clamped to the window [xlo, xhi] x [ylo, yhi]: the whole grid for the crop render, one tile for the overlay.
  template <class OkT>
  __device__ __forceinline__ bool set(const int* faces, int k, const float* sx, const float* sy, const float* iz, const OkT* ok, int xlo, int xhi, int ylo,
                                      int yhi) {
#pragma clang fp contract(off)
    i0 = faces[k * 3 + 0]; i1 = faces[k * 3 + 1]; i2 = faces[k * 3 + 2];
    if ((unsigned)i0 >= (unsigned)RASTER_NV || (unsigned)i1 >= (unsigned)RASTER_NV || (unsigned)i2 >= (unsigned)RASTER_NV) return false;
    if (i0 == i1 || i1 == i2 || i0 == i2) return false;
    if (!(ok[i0] && ok[i1] && ok[i2])) return false;
    e0.set(sx, sy, i1, i2);
    e1.set(sx, sy, i2, i0);
    e2.set(sx, sy, i0, i1);
    const float area = e2.at(sx[i2], sy[i2]);
    if (area == 0.0f || !isfinite(area)) return false;  // a finite area: every sx, sy of the face is finite
    // the pixel box, clamped to the window in float: a vertex at z = 1e-3 mm projects to 1e9
    const float x0f = fmaxf(ceilf(fminf(fminf(sx[i0], sx[i1]), sx[i2])), (float)xlo), x1f = fminf(floorf(fmaxf(fmaxf(sx[i0], sx[i1]), sx[i2])), (float)xhi);
    const float y0f = fmaxf(ceilf(fminf(fminf(sy[i0], sy[i1]), sy[i2])), (float)ylo), y1f = fminf(floorf(fmaxf(fmaxf(sy[i0], sy[i1]), sy[i2])), (float)yhi);
    if (!(x0f <= x1f && y0f <= y1f)) return false;
    x0 = (int)x0f; x1 = (int)x1f; y0 = (int)y0f; y1 = (int)y1f;  // inside the window
    iz0 = iz[i0]; iz1 = iz[i1]; iz2 = iz[i2];
    pos = area > 0.0f;
    return true;
  }
  // the three edge functions at pixel (c, r), sampled at ((float)c, (float)r): true iff the pixel centre is inside (two-sided: MANO is open at the wrist)
  __device__ __forceinline__ bool inside(int c, int r, float& w0, float& w1, float& w2) const {
    const float px = (float)c, py = (float)r;
    w0 = e0.at(px, py); w1 = e1.at(px, py); w2 = e2.at(px, py);
    return pos ? (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) : (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);
  }
  // true iff the face has a candidate at pixel (c, r): the centre is inside and the perspective-correct depth d there is finite and > 0
  __device__ __forceinline__ bool depth_at(int c, int r, float& d) const {
#pragma clang fp contract(off)
    float w0, w1, w2;
    if (!inside(c, r, w0, w1, w2)) return false;
    const float sum = __fadd_rn(__fadd_rn(w0, w1), w2);
    const float izp = __fadd_rn(__fadd_rn(__fmul_rn(__fdiv_rn(w0, sum), iz0), __fmul_rn(__fdiv_rn(w1, sum), iz1)), __fmul_rn(__fdiv_rn(w2, sum), iz2));
    d = __fdiv_rn(1.0f, izp);
    return isfinite(d) && d > 0.0f;
  }
  // a per-vertex quantity s interpolated at pixel (c, r) with the screen-space weights: ((w0/sum) s0 + (w1/sum) s1) + (w2/sum) s2
  __device__ __forceinline__ float interpolate(int c, int r, float s0, float s1, float s2) const {
#pragma clang fp contract(off)
    float w0, w1, w2;
    inside(c, r, w0, w1, w2);
    const float sum = __fadd_rn(__fadd_rn(w0, w1), w2);
    return __fadd_rn(__fadd_rn(__fmul_rn(__fdiv_rn(w0, sum), s0), __fmul_rn(__fdiv_rn(w1, sum), s1)), __fmul_rn(__fdiv_rn(w2, sum), s2));
  }
};

// pixel (c, r) of a face's box: its depth there enters the z-buffer word `slot` under `tag` (the face, or hand and face) by an integer min -- a positive
// float's bits order as the float does, so the smallest depth wins and among equal depths the lowest tag, whatever the order of arrival
__device__ __forceinline__ void raster_min(const RasterFace& f, int c, int r, unsigned tag, unsigned long long* slot) {
  float d;
  if (f.depth_at(c, r, d)) atomicMin(slot, ((unsigned long long)__float_as_uint(d) << 32) | tag);
}

}  // namespace
